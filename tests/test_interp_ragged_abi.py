"""CPU-side checks of the sample-fed ragged interpolator entry (sdrhip_interpolate_ragged, sdrhip_interpolators_last_plan): declared
in include/sdrhip.h with the documented prototypes and rules, exported, bound in Python, refused for a NULL handle and loudly without
a GPU; and K5c (interp_ragged_kernels.hip, a translation unit of its own) compiles for gfx950 with no scratch and within the
registers, LDS and occupancy of its IV_COUNT twins of interp_kernels.hip, which still compiles to its 74 kernels."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import interp_kernel_names as ikn
import test_iq8_abi as iq8

built = iq8.built
SRC = "interp_ragged_kernels.hip"
NAMES = ["sdrhip_interpolate_ragged", "sdrhip_interpolators_last_plan"]


def _norm(s):
    return re.sub(r"\s+", " ", s)


def test_declared_exported_and_bound(built):
    src = _norm(re.sub(r"/\*.*?\*/", "", iq8._header(), flags=re.S))
    lib = built.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in built.EXPORTS, n
    assert ("int sdrhip_interpolate_ragged(sdrhip_interpolators *p, int log2interp, const int16_t *iq_in, const size_t *n_in, size_t in_stride, "
            "int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);") in src
    assert "int sdrhip_interpolators_last_plan(const sdrhip_interpolators *p, sdrhip_interp_plan *out);" in src
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    assert lib.sdrhip_interpolate_ragged.argtypes == [vp, i, vp, C.POINTER(sz), sz, vp, sz, C.POINTER(sz), i]
    assert lib.sdrhip_interpolators_last_plan.argtypes == [vp, C.POINTER(built.InterpPlan)]
    # the Python structure is the header's
    m = re.search(r"typedef struct sdrhip_interp_plan \{(.*?)\} sdrhip_interp_plan;", src)
    fields = [(t.strip(), [x.strip() for x in names.split(",")]) for t, names in re.findall(r"(int|size_t) ([^;]+);", m.group(1))]
    flat = [(n, C.c_int if t == "int" else C.c_size_t) for t, ns in fields for n in ns]
    assert flat == list(built.InterpPlan._fields_)


def test_header_states_the_contract():
    h = iq8._header()
    at = h.index("int sdrhip_interpolate_ragged")
    comment = h[h.rindex("/*", 0, at):at].replace("\n * ", " ")
    for cite in ("Interpolators.h:38-43", "Upsampler.cpp:52-84", "Interpolators.cpp:363-606"):  # the lines sdrhip_interpolate cites
        assert cite in comment, cite
        assert cite in h[h.rindex("/*", 0, h.index("int sdrhip_interpolate(")):h.index("int sdrhip_interpolate(")], cite
    for word in ("n_out[s] = n_in[s] << log2interp", "host arrays of nstreams entries", "ignored for one stream", "byte for byte", "one-stream bank",
                 "keeps its six filter histories", "launches nothing", "compact", "only n_in[s] samples of row s are read", "only n_out[s] written",
                 '"h2d_bytes"', '"d2h_bytes"', "the alignment rules of sdrhip_interpolate", "No byte of row s past n_out[s]",
                 "read no sample of stream s past n_in[s]", "SDRHIP_EINVAL", "nothing consumed", "SDRHIP_EALIGN", "2^31"):
        assert word in _norm(comment), word


def test_python_surface(built):
    import sdrdaemon_amd as sd

    p = inspect.signature(sd.Interpolators.interpolate_ragged).parameters
    assert list(p) == ["self", "log2interp", "iq", "counts", "out"] and p["out"].default is None
    assert list(inspect.signature(sd.Interpolators.last_plan).parameters) == ["self"]
    assert "sdrhip_interpolate_ragged" in inspect.getsource(sd.Interpolators.interpolate_ragged)
    assert "sdrhip_interpolators_last_plan" in inspect.getsource(sd.Interpolators.last_plan)


def test_null_handles_are_refused(built):
    lib = built.lib()
    n_in, n_out = (C.c_size_t * 2)(5, 7), (C.c_size_t * 2)(11, 13)
    buf = (C.c_int16 * 64)()
    assert lib.sdrhip_interpolate_ragged(None, 4, buf, n_in, 8, buf, 128, n_out, 0) == -1
    assert b"NULL" in lib.sdrhip_last_error()
    assert list(n_out) == [11, 13]  # (nothing written)
    plan = built.InterpPlan(9, 9, 9, 9, 9, 9)
    assert lib.sdrhip_interpolators_last_plan(None, C.byref(plan)) == -1
    assert b"NULL" in lib.sdrhip_last_error() and plan.path == 9 and plan.entries == 9


def test_no_gpu_means_loud_failure(built):
    import numpy as np

    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        return
    with pytest.raises(sd.SdrHipError) as e:  # (no GPU: no context, no bank -- never a quiet host path)
        sd.Interpolators(sd.Context(0), 2).interpolate_ragged(4, np.zeros((2, 8, 2), np.int16), [8, 3])
    assert e.value.code == -3


def _compile(tmp_path, src):
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(iq8.CSRC, src), "-o", str(tmp_path / (src + ".o"))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = iq8._resources(r.stderr)
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(lds) == len(res)
    return {n: v + (l,) for (n, v), l in zip(res.items(), lds)}  # VGPRs, scratch, occupancy, LDS bytes


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """the resource reports of the new file and of interp_kernels.hip (its twins), compiled once"""
    d = tmp_path_factory.mktemp("k5c")
    return _compile(d, SRC), _compile(d, "interp_kernels.hip")


_MAPPED = re.compile(r"\d+interp_(wave_)?mapped_kernelI((?:Li\d+E)+)EEv")


def _mapped(res):
    """{(path, L, WPW): mangled name} of the mapped kernels"""
    out = {}
    for n in res:
        m = _MAPPED.search(n)
        if m:
            a = [int(x) for x in re.findall(r"Li(\d+)E", m.group(2))]
            assert len(a) == (2 if m.group(1) else 1), n
            out[("wave" if m.group(1) else "valu", a[0], a[1] if m.group(1) else None)] = n
    return out


def test_no_scratch_and_the_kernels_that_are_there(resources):
    res, base = resources
    k = _mapped(res)
    assert sorted(x for x in k if x[0] == "valu") == [("valu", L, None) for L in range(1, 7)]
    assert sorted(x for x in k if x[0] == "wave") == [("wave", L, w) for L in range(2, 7) for w in (1, 4)]
    assert len(res) == 6 + 10 + 1, sorted(res)
    assert not ikn.by_meaning(res)  # (none of them reads as a kernel of interp_variant.h)
    for n, (vg, sc, occ, lds) in sorted(res.items()):
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        if n not in k.values():  # the x1 copy: no LDS, full occupancy
            assert "interp1_mapped_kernel" in n and lds == 0 and vg <= 64 and occ == 8, (n, vg, lds, occ)
    # interp_kernels.hip is what it was
    assert len(ikn.by_meaning(base)) == len(base) == 74, sorted(base)


@pytest.mark.parametrize("path,L", [(p, L) for p in ("valu", "wave") for L in range(2 if p == "wave" else 1, 7)])
def test_kernels_compile_within_their_count_twins_resources(resources, path, L):
    """Every mapped kernel against the IV_COUNT kernel of the same (path, L, WPW) -- K5r, the same body behind a per-stream count --:
    K5w no more VGPRs, K5 no more 8-register allocation units and no lower occupancy, none more LDS; the counts are printed."""
    res, base = resources
    twins = ikn.by_meaning(base)
    seen = 0
    for (p, l, wpw), n in sorted(_mapped(res).items(), key=str):
        if (p, l) != (path, L):
            continue
        seen += 1
        vg, _, occ, lds = res[n]
        tv, _, tocc, tl = base[twins[(path, L, wpw, ikn.COUNT)]]
        print(n, "VGPRs", vg, "twin", tv, "LDS", lds, "twin", tl, "occupancy", occ, "twin", tocc)
        assert lds <= tl, "%s: %d bytes of LDS, its twin %d" % (n, lds, tl)
        if path == "wave":
            assert vg <= tv, "%s: %d VGPRs, its twin %d" % (n, vg, tv)
        else:
            assert (vg + 7) // 8 <= (tv + 7) // 8, "%s: %d VGPRs, its twin %d" % (n, vg, tv)
        assert occ >= tocc, "%s: occupancy %d, its twin %d" % (n, occ, tocc)
    assert seen == (2 if path == "wave" else 1)


def test_lives_in_a_translation_unit_of_its_own():
    """the file takes the bodies, not interp_variant.h; the Makefile builds it; the bank's one launcher keeps its one call site"""
    text = open(os.path.join(iq8.CSRC, SRC)).read()
    incs = re.findall(r'^#include "([^"]+)"', text, flags=re.M)
    assert "interp_variant.h" not in incs and "interp_body.h" in incs and "interp_wave.h" in incs
    assert "interp_segment<L, true, IQF_S16>" in text and "interp_wave_segment<L, false, IQF_S16>" in text
    assert SRC in open(os.path.join(iq8.CSRC, "Makefile")).read()
    for f in sorted(os.listdir(iq8.CSRC)):
        if f.endswith(".hip") and f != SRC:
            assert "mapped_kernel" not in open(os.path.join(iq8.CSRC, f)).read(), f
    host = open(os.path.join(iq8.CSRC, "sdrhip_interp.cpp")).read()
    assert host.count("launch_interp_mapped(") == 1 and host.count("launch_interpolate(") == 1
    assert "map_tab.upload(" in host  # (the per-call table goes through the version rotation of dev_buffers.h)
