#!/usr/bin/env python3
"""VALU ledger of the bit-sliced FFT encoder (gf_encode128_bs.h) beside the table form (gf_encode128_fft.h): cross-compiles
gf_kernels.hip for gfx950 (CPU only), counts the VALU instructions of each kernel by class -- both block-half variants, the code is
straight-line, so the static count is the per-workgroup count of two of its four waves -- and prints registers and scratch from
the code object's metadata.  usage: python tools/bs_ledger.py [--hipcc /opt/rocm/bin/hipcc]"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"table": "gf_encode128_fft_kernel", "bitslice": "gf_encode128_bs_kernel"}
CLASSES = [("perm (table lookups)", ("v_perm_b32",)), ("xor3 / bitop3", ("v_bitop3_b32", "v_xor3_b32")), ("xor", ("v_xor_b32",)),
           ("bfi (bit transposes)", ("v_bfi_b32",)), ("and", ("v_and_b32",)), ("shifts", ("v_lshrrev_b32", "v_lshlrev_b32"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    src = os.path.join(ROOT, "sdrdaemon_amd", "csrc", "gf_kernels.hip")
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "gf.s")
        subprocess.check_call([args.hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                               "--cuda-device-only", "-S", "-o", asm, src])
        lines = open(asm).read().split("\n")
    text = "\n".join(lines)
    res = {}
    for form, k in KERNELS.items():
        sym = next(l.split(":")[0] for l in lines if l.startswith("_Z") and re.search(r"\d" + k + "ENS[^:]*:", l))
        i = next(n for n, l in enumerate(lines) if l.startswith(sym + ":"))
        j = next(n for n in range(i, len(lines)) if "s_endpgm" in lines[n])
        ops = collections.Counter(l.split()[0].split("_e32")[0].split("_e64")[0] for l in lines[i:j] if l.strip().startswith("v_"))
        meta = text[text.index(".name:           " + sym):][:2000]
        vg = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        scr = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        res[form] = (ops, vg, spill, scr)
    print("%-24s %10s %10s" % ("VALU class", "table", "bitslice"))
    for name, pre in CLASSES:
        print("%-24s %10d %10d" % (name, *(sum(v for o, v in res[f][0].items() if o.startswith(pre)) for f in KERNELS)))
    print("%-24s %10d %10d" % ("all VALU", *(sum(res[f][0].values()) for f in KERNELS)))
    for lbl, idx in (("VGPRs", 1), ("VGPR spills", 2), ("scratch bytes", 3)):
        print("%-24s %10d %10d" % (lbl, *(res[f][idx] for f in KERNELS)))
    print("\nmodel per 4-byte column and workgroup wave pair (DESIGN.md K3f): table multiplications ~10 VALU per 4 bytes; a plane")
    print("multiplication ~18 VALU per 32 bytes (xor3 trees of the constant's 8 x 8 matrix); a bit transpose 48 VALU per 8 dwords")
    print("(3 delta-swap stages x 4 register pairs x 2 shifts + 2 v_bfi).  Bit-sliced in this mapping: inverse stages 3..5, the t5 / t6")
    print("folds, stage 4 and the first stage of each size-16 transform -- 23 + 10 plane multiplications replace 184 + 80 table ones")
    print("per column; 10 octet transposes per wave (8 in, 2 out) are the price.")


if __name__ == "__main__":
    main()
