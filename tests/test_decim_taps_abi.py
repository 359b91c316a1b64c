"""CPU-side checks of the decimator taps (sdrhip_decimate_taps, K1t): the entry and its structure stand in include/sdrhip.h as the
binding has them, the header states the contract and cites the reference, the call is refused loudly without a GPU, the ten K1t
kernels compile for gfx950 without scratch and with no fewer waves per SIMD than their K1r twins, and every existing decimator kernel
keeps the registers, the scratch and the waves per SIMD it had before K1t (decim_kernel_resources_parent.json: the same compile of
the parent commit's files)."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from test_iq8_abi import _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from sdrdaemon_amd import _lib

    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "sdrhip.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


PROTOTYPE = ("int sdrhip_decimate_taps(sdrhip_decimators *d, unsigned tap_mask, unsigned sampleSize, const int16_t *iq_in, "
             "const size_t *n_in, size_t in_stride, sdrhip_decim_taps *taps, size_t *n_used, int mem);")
STRUCT = ("typedef struct sdrhip_decim_taps { int16_t *iq_out[SDRHIP_DECIM_TAP_SLOTS]; size_t out_stride[SDRHIP_DECIM_TAP_SLOTS]; "
          "unsigned sample_size[SDRHIP_DECIM_TAP_SLOTS]; } sdrhip_decim_taps;")


def test_declared_exported_and_bound(built):
    src = _squash(_code())
    assert PROTOTYPE in src
    assert STRUCT in src
    assert re.search(r"#define SDRHIP_DECIM_TAP_SLOTS 7\b", src)
    assert src.index("sdrhip_decimate_ragged_bits(") < src.index("sdrhip_decim_taps {") < src.index("sdrhip_decimate_taps(") < src.index("sdrhip_interpolators_create(")
    lib = built.lib()
    assert "sdrhip_decimate_taps" in built.EXPORTS and hasattr(lib, "sdrhip_decimate_taps")
    vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert list(lib.sdrhip_decimate_taps.argtypes) == [vp, u, u, vp, C.POINTER(sz), sz, C.POINTER(built.DecimTaps), C.POINTER(sz), i]
    # the Python structure is the header's: names, order, element types and counts
    ctype_of = {"int16_t *": vp, "size_t ": sz, "unsigned ": u}
    fields = re.findall(r"(int16_t \*|size_t |unsigned )(\w+)\[SDRHIP_DECIM_TAP_SLOTS\];", STRUCT)
    assert len(fields) == 3 and built.DECIM_TAP_SLOTS == 7
    assert [(n, t._type_, t._length_) for n, t in built.DecimTaps._fields_] == [(n, ctype_of[t], 7) for t, n in fields]
    assert C.sizeof(built.DecimTaps) == 7 * 8 + 7 * 8 + 7 * 4 + 4  # (padded to the pointers' alignment, as the C compiler pads it)


def test_header_states_the_contract():
    h = _header()
    doc = h[h.index("/* Decimators bank, taps"):h.index("#define SDRHIP_DECIM_TAP_SLOTS")]
    doc = _squash(re.sub(r"\n \*", "\n", doc))  # (the comment's text without its line starts)
    for cite in ("Decimators.h:38-53", "Decimators.cpp:94-120", "Decimators.cpp:173-213", "Decimators.cpp:403-516", "Decimators.cpp:902-1305",
                 "Downsampler.cpp:74-162"):
        assert cite in doc, cite
    for phrase in ("byte for byte", "n_used[s] >> k", "nothing consumed", '"h2d_bytes"', '"d2h_bytes"', "16-byte aligned",
                   "multiples of 4 samples", "No byte", "SDRHIP_EINVAL", "SDRHIP_EALIGN", "Not covered"):
        assert phrase in doc, phrase


def test_python_surface(built):
    import sdrdaemon_amd as sd

    sig = inspect.signature(sd.Decimators.decimate_taps)
    assert list(sig.parameters) == ["self", "taps", "sample_size", "iq", "counts", "out"]
    assert sig.parameters["counts"].default is None and sig.parameters["out"].default is None


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    lib = built.lib()
    t, n = built.DecimTaps(), (C.c_size_t * 1)(64)
    assert lib.sdrhip_decimate_taps(None, 0x14, 16, None, n, 64, C.byref(t), n, 0) == -1  # (a NULL handle: SDRHIP_EINVAL, GPU or not)
    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(sd.SdrHipError):
        sd.Decimators(sd.Context(0), 1).decimate_taps([2, 4], 16, np.zeros((64, 2), np.int16))


def _variant(name, kernel):
    """(L, first stage packed int16) of an instantiation of `kernel`: decim_taps_kernel<L, PACK16> / decim_ragged_kernel<L, 2, PACK16>"""
    m = re.search(r"%sILi(\d)E(?:Li2E)?Lb([01])E" % kernel, name)
    return (int(m.group(1)), m.group(2) == "1") if m else None


def test_taps_kernels_compile_lean(tmp_path):
    res = _compile(tmp_path, "decim_taps_kernels.hip")
    taps = {_variant(n, "decim_taps_kernel"): n for n in res}
    assert len(res) == 10 and sorted(taps) == [(L, p) for L in range(2, 7) for p in (False, True)], sorted(res)
    twins = _compile(tmp_path, "rx_ragged_kernels.hip")
    twin = {_variant(n, "decim_ragged_kernel"): n for n in twins if "decim_ragged_kernel" in n and "Li2ELb" in n}
    for key, n in sorted(taps.items()):
        vg, sc, occ = res[n]
        tv, _, tocc = twins[twin[key]]
        print("K1t L=%d pack16=%d: %3d VGPRs, scratch %d, %d waves/SIMD; K1r twin %3d VGPRs, %d waves/SIMD" % (key + (vg, sc, occ, tv, tocc)))
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        assert occ >= tocc, "%s: %d waves per SIMD, its K1r twin %d" % (n, occ, tocc)


@pytest.mark.parametrize("src", ["decim_kernels.hip", "rx_ragged_kernels.hip", "decim_mfma.hip"])
def test_existing_decimator_kernels_untouched(tmp_path, src):
    parent = json.load(open(os.path.join(HERE, "decim_kernel_resources_parent.json")))[src]
    res = _compile(tmp_path, src)
    assert sorted(res) == sorted(parent), sorted(set(res) ^ set(parent))
    for n, want in sorted(parent.items()):
        assert list(res[n]) == want, "%s: (VGPRs, scratch, waves per SIMD) %s, the parent commit's %s" % (n, res[n], want)
