"""CPU-side checks of the Rx pipe fed datagrams (sdrhip_rx_process_datagrams, sdrhip_rx_collector, sdrhip_rx_carry): declared in
include/sdrhip.h with the documented prototypes, exported by libsdrhip.so, refused loudly without a GPU, and the join's kernels
(rx_join_kernels.hip: the remainder kernel KJ and the collector's delivery passes with per-stream row offsets) compile for gfx950
without scratch; the passes take no more registers than the bank's own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "sdrhip_rx_process_datagrams": "int sdrhip_rx_process_datagrams(sdrhip_rx *rx, const uint8_t *dgrams, const size_t *n_dgrams, "
                                   "size_t dgram_stride_bytes, const uint32_t *tv_sec, const uint32_t *tv_usec, size_t max_released, "
                                   "uint8_t *frames_out, size_t frame_stride_bytes, sdrhip_fecbuf_frame *info_out, "
                                   "size_t *n_released, size_t *n_frames, int mem);",
    "sdrhip_rx_collector": "int sdrhip_rx_collector(sdrhip_rx *rx, sdrhip_fecbuf **out);",
    "sdrhip_rx_carry": "int sdrhip_rx_carry(const sdrhip_rx *rx, size_t *carry);",
}
built = iq8.built


def _norm(s):
    return re.sub(r"\s+", " ", s).replace("( ", "(").strip()


def test_declared_with_the_documented_prototypes_and_exported(built):
    src = _norm(re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrhip.h")).read(), flags=re.S))
    lib = built.lib()
    for name, proto in PROTOS.items():
        assert _norm(proto) in src, name
        assert hasattr(lib, name), name
        assert name in built.EXPORTS, name


def test_python_surface(built):
    import inspect

    import sdrdaemon_amd as sd

    for m in ("process_datagrams", "collector_stats", "carry"):
        assert hasattr(sd.RxPipe, m), m
    assert list(inspect.signature(sd.RxPipe.process_datagrams).parameters)[1:] == ["dgrams_per_stream", "tv_sec", "tv_usec", "max_released"]


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    assert lib.sdrhip_rx_process_datagrams(None, None, None, 0, None, None, 0, None, 0, None, None, None, 0) == -1
    h = C.c_void_p()
    assert lib.sdrhip_rx_collector(None, C.byref(h)) == -1 and not h.value
    assert lib.sdrhip_rx_carry(None, None) == -1
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 4).process_datagrams([np.zeros((0, 512), np.uint8)] * 4)


def test_null_arguments_are_refused_with_a_gpu(built):
    """(the same refusal where a handle can be made: NULL count and stamp arrays, nothing consumed)"""
    import sdrdaemon_amd as sd

    if sd.device_count() == 0:
        pytest.skip("no GPU")
    rx = sd.RxPipe(sd.Context(0), 2)
    assert built.lib().sdrhip_rx_process_datagrams(rx.h, None, None, 0, None, None, 0, None, 0, None, None, None, 0) == -1
    assert list(rx.carry()) == [0, 0]


def test_join_kernels_compile_without_scratch(tmp_path):
    res = iq8._compile(tmp_path, "rx_join_kernels.hip")
    assert len(res) == 3, sorted(res)  # KJ, the scatter and the copy pass with row offsets

    def pick(d, name):
        k = "%d%s" % (len(name), name)
        return [v for n, v in d.items() if k in n]

    for n, (vg, sc, occ) in res.items():
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
    (vg, sc, occ), = pick(res, "rx_join_carry_kernel")
    assert sc == 0 and occ == 8, (vg, sc, occ)
    (tmp_path / "b").mkdir()
    bank = iq8._compile(tmp_path / "b", "fecbuf_kernels.hip")
    for name, base in (("fecbuf_scatter_rows_kernel", "fecbuf_scatter_kernel"), ("fecbuf_copy_rows_kernel", "fecbuf_copy_kernel")):
        (vg, _, occ), = pick(res, name)
        (vb, _, ob), = pick(bank, base)
        assert (vg + 7) // 8 <= (vb + 7) // 8 and occ >= ob, (name, vg, vb, occ, ob)
