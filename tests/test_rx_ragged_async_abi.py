"""CPU-side checks of the asynchronous ragged Rx entry (sdrhip_rx_submit_ragged, sdrhip_rx_collect_ragged): declared in
include/sdrhip.h with the documented prototypes, exported by libsdrhip.so and reachable from Python, refused loudly without a GPU,
and the new kernels (rx_async_kernels.hip: K0p and the frame gather) compile for gfx950 without scratch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "sdrhip_rx_submit_ragged": "int sdrhip_rx_submit_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, "
                               "const uint32_t *tv_sec, const uint32_t *tv_usec);",
    "sdrhip_rx_collect_ragged": "int sdrhip_rx_collect_ragged(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, "
                                "size_t max_frames, size_t *n_frames, int wait);",
}
built = iq8.built


def _norm(s):
    return re.sub(r"\s+", " ", s).replace("( ", "(").strip()


def test_declared_with_the_documented_prototypes_and_exported(built):
    raw = open(os.path.join(ROOT, "include", "sdrhip.h")).read()
    assert re.search(r"#define SDRHIP_PACKED 0\b", raw)
    src = _norm(re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    lib = built.lib()
    for name, proto in PROTOS.items():
        assert _norm(proto) in src, name
        assert hasattr(lib, name), name
        assert name in built.EXPORTS, name


def test_python_surface():
    import sdrdaemon_amd as sd

    for m in ("submit_ragged", "collect_ragged"):
        assert hasattr(sd.RxPipe, m), m


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    n = (C.c_size_t * 2)(4, 0)
    t = (C.c_uint32 * 2)(0, 0)
    nf = (C.c_size_t * 2)()
    # NULL handle, NULL count / stamp arrays, NULL n_frames: SDRHIP_EINVAL
    assert lib.sdrhip_rx_submit_ragged(None, None, n, 0, t, t) == -1
    assert lib.sdrhip_rx_collect_ragged(None, None, 0, 0, nf, 1) == -1
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 2).submit_ragged(np.zeros((2, 64, 2), np.int16), [64, 3])


def test_async_kernels_compile_without_scratch(tmp_path):
    res = iq8._compile(tmp_path, "rx_async_kernels.hip")
    unpack = {n: v for n, v in res.items() if "unpack_packed_kernel" in n}
    gather = {n: v for n, v in res.items() if "frame_gather_kernel" in n}
    assert len(unpack) == 3, sorted(res)  # int16, U8, S8
    assert len(gather) == 1 and len(res) == 4, sorted(res)
    for n, (vg, sc, occ) in res.items():
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        assert occ >= 8, "%s: occupancy %d waves per SIMD" % (n, occ)


def test_async_kernels_move_16_bytes_per_lane(tmp_path):
    """K0p and the gather copy with 16-byte vector loads and stores, as K0 does"""
    hipcc = iq8.HIPCC
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    import subprocess

    out = tmp_path / "k.s"
    r = subprocess.run([hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(iq8.CSRC, "rx_async_kernels.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    bodies = re.split(r"\n(?=_ZN\S+:)", asm)
    seen = 0
    for body in bodies:
        m = re.match(r"(_ZN\S+):", body)
        if not m or not ("unpack_packed_kernel" in m.group(1) or "frame_gather_kernel" in m.group(1)):
            continue
        seen += 1
        assert "global_load_dwordx4" in body, m.group(1)
        assert "global_store_dwordx4" in body, m.group(1)
    assert seen == 4
