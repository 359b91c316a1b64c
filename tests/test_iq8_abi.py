"""CPU-side checks of the 8-bit IQ formats (sdrhip_rx_set_input_format, sdrhip_tx_set_output_format, the h2d / d2h byte counters):
declared in include/sdrhip.h, exported by libsdrhip.so, refused loudly without a GPU, and the new kernels -- the widening / narrowing
pass and every 8-bit interpolator instantiation -- compile for gfx950 without scratch and with no more registers than their int16
twins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import interp_kernel_names as ikn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sdrhip_rx_set_input_format", "sdrhip_tx_set_output_format"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from sdrdaemon_amd import _lib

    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "sdrhip.h")).read()


def test_declared_and_exported(built):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = built.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in built.EXPORTS, n
    for name, value in (("SDRHIP_IQ_S16", 0), ("SDRHIP_IQ_U8", 1), ("SDRHIP_IQ_S8", 2), ("SDRHIP_K_CONVERT", 4)):
        assert re.search(r"#define %s %d\b" % (name, value), src), name
    assert (built.IQ_S16, built.IQ_U8, built.IQ_S8) == (0, 1, 2)


def test_header_cites_the_reference():
    h = _header()
    for cite in ("RtlSdrSource.cpp:542-553", "HackRFSource.cpp:661-674", "HackRFSink.cpp:671-672", "sdrdaemonrx.cpp:619-643"):
        assert cite in h, cite
    assert '"h2d_bytes"' in h and '"d2h_bytes"' in h


def test_python_surface(built):
    import inspect

    import sdrdaemon_amd as sd

    assert "input_format" in inspect.signature(sd.RxPipe.__init__).parameters
    assert "output_format" in inspect.signature(sd.TxPipe.__init__).parameters
    assert hasattr(sd.RxPipe, "set_input_format") and hasattr(sd.TxPipe, "set_output_format")
    assert sd.engine.K_CONVERT == 4


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    assert lib.sdrhip_rx_set_input_format(None, 1) == -1
    assert lib.sdrhip_tx_set_output_format(None, 2) == -1
    v = C.c_uint64(7)
    assert lib.sdrhip_ctx_get_counter(None, b"h2d_bytes", C.byref(v)) == -1
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 1, input_format="u8").process(np.zeros((64, 2), np.uint8))
    with pytest.raises(sd.SdrHipError):
        sd.TxPipe(sd.Context(0), 1, output_format="s8")


def test_python_rejects_bad_formats_and_dtypes(built):
    import sdrdaemon_amd as sd
    from sdrdaemon_amd import engine

    with pytest.raises(ValueError):
        engine._iq_format("u8", ("s16", "s8"))  # (U8 is an input format only)
    with pytest.raises(ValueError):
        engine._iq_format("s12", ("s16", "u8", "s8"))
    with pytest.raises(TypeError):
        engine._bank_view(np.zeros((4, 2), np.int16), 1, np.uint8)
    with pytest.raises(TypeError):
        engine._bank_view(np.zeros((4, 2), np.int8), 1, np.uint8)
    x, _, squeeze = engine._bank_view(np.arange(16, dtype=np.uint8), 1, np.uint8)  # flat interleaved
    assert x.shape == (1, 8, 2) and squeeze and x[0, 3, 1] == 7
    x, _, _ = engine._bank_view(np.zeros((3, 20), np.int8), 3, np.int8)
    assert x.shape == (3, 10, 2) and engine._stride_samples(x) == 10
    assert sd.SdrHipError


def _resources(stderr):
    names = re.findall(r"Function Name: (\S+)", stderr)
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", stderr)]
    occupancy = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", stderr)]
    assert len(names) == len(vgprs) == len(scratch) == len(occupancy)
    return {n: (v, s, o) for n, v, s, o in zip(names, vgprs, scratch, occupancy)}  # VGPRs, scratch bytes per lane, waves per SIMD


def _compile(tmp_path, src):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return _resources(r.stderr)


def test_convert_kernels_compile_without_scratch(tmp_path):
    res = _compile(tmp_path, "convert_kernels.hip")
    assert len(res) == 3, sorted(res)  # widen U8 / S8, narrow
    assert any("iq8_widen_kernel" in n for n in res) and any("iq8_narrow_kernel" in n for n in res)
    for n, (vg, sc, _) in res.items():
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)


def test_s8_interpolators_compile_without_scratch(tmp_path):
    res = _compile(tmp_path, "interp_kernels.hip")
    kernels = ikn.by_meaning(res)  # (path, L, WPW, flags) -> name
    s8 = {k: n for k, n in kernels.items() if k[3] & ikn.S8}
    # K5 (interpolate2 .. 64) and K5w (interpolate4 .. 64, one or four waves per workgroup), uniform and per-stream counts
    for flags in (ikn.S8, ikn.S8 | ikn.COUNT):
        assert len([k for k in s8 if k[0] == "valu" and k[3] == flags]) == 6 and len([k for k in s8 if k[0] == "wave" and k[3] == flags]) == 10, flags
    assert len(s8) == 2 * (6 + 10), sorted(s8.values())
    for (path, L, wpw, flags), n in s8.items():
        vg, sc, occ = res[n]
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        t = kernels[(path, L, wpw, flags & ~ikn.S8)]  # the int16 twin: the plain kernel, or the count variant
        if path == "wave":  # K5w: exact
            assert vg <= res[t][0], "%s: %d VGPRs, its int16 twin %d" % (n, vg, res[t][0])
        else:  # K5: x64 reports 70 against 68: the same allocation of 8-register units and the same occupancy
            assert (vg + 7) // 8 <= (res[t][0] + 7) // 8, "%s: %d VGPRs, its int16 twin %d" % (n, vg, res[t][0])
            assert occ >= res[t][2], "%s: occupancy %d, its int16 twin %d" % (n, occ, res[t][2])
