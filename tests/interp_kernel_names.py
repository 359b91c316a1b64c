"""The interpolator kernels of interp_variant.h by meaning: a mangled kernel name -> (path, L, WPW, flags).

path "valu" (K5) | "wave" (K5w); L = log2 of the ratio; WPW = waves per workgroup (None for K5); flags = an OR of the IV_* bits of
sdrdaemon_amd/csrc/interp_pick.h, 0 for the plain kernels interp_kernel<L> / interp_wave_kernel<L, WPW>.  The twin of a kernel is
the kernel of the same (path, L, WPW) with other flags."""
import re

GATHER, COUNT, S8, TABLE = 1, 2, 4, 8

# <length><name>I<template arguments>E: Li<n>E an int argument, Lj<n>E an unsigned one (the flag word)
_NAME = re.compile(r"\d+interp_(wave_)?(variant_)?kernelI((?:L[ij]\d+E)+)EEv")


def parse(mangled):
    """(path, L, WPW, flags) of an interpolator kernel's mangled name, None for any other kernel"""
    m = _NAME.search(mangled)
    if not m:
        return None
    wave, variant = bool(m.group(1)), bool(m.group(2))
    args = re.findall(r"L([ij])(\d+)E", m.group(3))
    kinds, values = "".join(k for k, _ in args), [int(v) for _, v in args]
    assert kinds == ("ii" if wave else "i") + ("j" if variant else ""), mangled
    flags = values[-1] if variant else 0
    assert (flags != 0) == variant, mangled
    return ("wave" if wave else "valu", values[0], values[1] if wave else None, flags)


def by_meaning(names):
    """{(path, L, WPW, flags): mangled name} of the interpolator kernels among names"""
    out = {}
    for n in names:
        k = parse(n)
        if k is not None:
            assert k not in out, (k, n, out[k])
            out[k] = n
    return out
