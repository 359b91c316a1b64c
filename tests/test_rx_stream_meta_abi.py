"""CPU-side checks of the per-stream meta values of an Rx bank (sdrhip_rx_set_stream_meta / sdrhip_rx_get_stream_meta): declared
in include/sdrhip.h with their citations, exported by libsdrhip.so, present in the Python surface, refused loudly without a GPU --
and the kernels that gained the per-stream table keep their resources: every kernel of the five translation units that form a meta
record compiles for gfx950 with no scratch where it had none, no more VGPRs and no lower occupancy than before the feature."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sdrhip_rx_set_stream_meta", "sdrhip_rx_get_stream_meta"]
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


def test_header_cites_the_reference():
    h = _header()
    at = h.index("int sdrhip_rx_set_stream_meta")
    comment = h[h.rindex("/*", 0, at):at]
    for cite in ("UDPSink.h:93-96", "sdrdaemonrx.cpp:597", "UDPSinkFEC.cpp:160-165"):
        assert cite in comment, cite
    for word in ("sdrhip_rx_reconfigure does not clear", "never synchronises", "NULL = that field is bank-wide"):
        assert word in comment, word


def test_python_surface(built):
    import sdrdaemon_amd as sd

    sig = inspect.signature(sd.RxPipe.set_stream_meta).parameters
    assert list(sig)[1:] == ["center_frequency_khz", "sample_rate"] and all(sig[k].default is None for k in list(sig)[1:])
    assert list(inspect.signature(sd.RxPipe.stream_meta).parameters)[1:] == ["stream"]
    assert list(inspect.signature(sd.RxPipe.follow_testsource).parameters)[1:] == ["ts"]


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    fc, sr = (C.c_uint32 * 2)(1, 2), C.c_uint32(0)
    assert lib.sdrhip_rx_set_stream_meta(None, fc, fc) == -1
    assert lib.sdrhip_rx_get_stream_meta(None, 0, C.byref(sr), C.byref(sr)) == -1
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 2).set_stream_meta([1, 2], [3, 4])
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 1).process(np.zeros((64, 2), np.int16))


# (VGPRs, scratch bytes per lane, waves per SIMD) of every kernel of the five translation units at the commit named here, the
# parent of the per-stream table: that commit's sources compiled with _compile()'s command
PARENT_COMMIT = "f1f515ac7e8eecf6d30e04e21a33bc5544623b4e"
PARENT = {
    "decim_mfma.hip": {
        "_ZN6sdrhip12_GLOBAL__N_115rx_fused_kernelILi2ELb1EEEvNS_9DecimArgsENS_10Enc128ArgsENS0_10FusedRolesE": (126, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_115rx_fused_kernelILi2ELb0EEEvNS_9DecimArgsENS_10Enc128ArgsENS0_10FusedRolesE": (126, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_115rx_fused_kernelILi3ELb1EEEvNS_9DecimArgsENS_10Enc128ArgsENS0_10FusedRolesE": (168, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_115rx_fused_kernelILi3ELb0EEEvNS_9DecimArgsENS_10Enc128ArgsENS0_10FusedRolesE": (168, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_115rx_fused_kernelILi4ELb1EEEvNS_9DecimArgsENS_10Enc128ArgsENS0_10FusedRolesE": (161, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_115rx_fused_kernelILi4ELb0EEEvNS_9DecimArgsENS_10Enc128ArgsENS0_10FusedRolesE": (157, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi2ELb1ELi4ELb1EEEvNS_9DecimArgsE": (127, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi2ELb0ELi4ELb1EEEvNS_9DecimArgsE": (127, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi2ELb1ELi4ELb0EEEvNS_9DecimArgsE": (127, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi2ELb0ELi4ELb0EEEvNS_9DecimArgsE": (127, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi3ELb1ELi4ELb1EEEvNS_9DecimArgsE": (169, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi3ELb0ELi4ELb1EEEvNS_9DecimArgsE": (169, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi3ELb1ELi4ELb0EEEvNS_9DecimArgsE": (170, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi3ELb0ELi4ELb0EEEvNS_9DecimArgsE": (170, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb1ELi3ELb1EEEvNS_9DecimArgsE": (214, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb0ELi3ELb1EEEvNS_9DecimArgsE": (214, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb1ELi3ELb0EEEvNS_9DecimArgsE": (211, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb0ELi3ELb0EEEvNS_9DecimArgsE": (211, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb1ELi2ELb1EEEvNS_9DecimArgsE": (241, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb0ELi2ELb1EEEvNS_9DecimArgsE": (241, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb1ELi2ELb0EEEvNS_9DecimArgsE": (231, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb0ELi2ELb0EEEvNS_9DecimArgsE": (231, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb1ELi4ELb1EEEvNS_9DecimArgsE": (223, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb0ELi4ELb1EEEvNS_9DecimArgsE": (223, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb1ELi4ELb0EEEvNS_9DecimArgsE": (215, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi4ELb0ELi4ELb0EEEvNS_9DecimArgsE": (215, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi5ELb1ELi4ELb1EEEvNS_9DecimArgsE": (184, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi5ELb0ELi4ELb1EEEvNS_9DecimArgsE": (184, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi5ELb1ELi4ELb0EEEvNS_9DecimArgsE": (184, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi5ELb0ELi4ELb0EEEvNS_9DecimArgsE": (184, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi6ELb1ELi4ELb1EEEvNS_9DecimArgsE": (204, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi6ELb0ELi4ELb1EEEvNS_9DecimArgsE": (204, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi6ELb1ELi4ELb0EEEvNS_9DecimArgsE": (201, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_117decim_mfma_kernelILi6ELb0ELi4ELb0EEEvNS_9DecimArgsE": (201, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi2ELb1ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (122, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi2ELb0ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (122, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi2ELb1ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (127, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi2ELb0ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (127, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi3ELb1ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (158, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi3ELb0ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (158, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi3ELb1ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (170, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi3ELb0ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (170, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb1ELi3ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (159, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb0ELi3ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (160, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb1ELi3ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (210, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb0ELi3ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (210, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb1ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (159, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb0ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (160, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb1ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (214, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi4ELb0ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (214, 0, 1),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi5ELb1ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (182, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi5ELb0ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (182, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi5ELb1ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (184, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi5ELb0ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (184, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi6ELb1ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (236, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi6ELb0ELi4ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (197, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi6ELb1ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (201, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_124decim_mfma_ragged_kernelILi6ELb0ELi4ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (200, 0, 2),
    },
    "decim_kernels.hip": {
        "_ZN6sdrhip19decim_simple_kernelEiiPKsmPsmmii": (21, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi1ELi2ELb1EEEvNS_9DecimArgsE": (64, 0, 7),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi1ELi2ELb0EEEvNS_9DecimArgsE": (89, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi2ELi2ELb1EEEvNS_9DecimArgsE": (83, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi2ELi2ELb0EEEvNS_9DecimArgsE": (91, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi3ELi2ELb1EEEvNS_9DecimArgsE": (85, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi3ELi2ELb0EEEvNS_9DecimArgsE": (93, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi4ELi2ELb1EEEvNS_9DecimArgsE": (85, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi4ELi2ELb0EEEvNS_9DecimArgsE": (93, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi5ELi2ELb1EEEvNS_9DecimArgsE": (85, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi5ELi2ELb0EEEvNS_9DecimArgsE": (93, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi6ELi2ELb1EEEvNS_9DecimArgsE": (85, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi6ELi2ELb0EEEvNS_9DecimArgsE": (93, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi3ELi0ELb0EEEvNS_9DecimArgsE": (147, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi4ELi0ELb0EEEvNS_9DecimArgsE": (151, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi5ELi0ELb0EEEvNS_9DecimArgsE": (153, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi6ELi0ELb0EEEvNS_9DecimArgsE": (153, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi3ELi1ELb0EEEvNS_9DecimArgsE": (147, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi4ELi1ELb0EEEvNS_9DecimArgsE": (151, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi5ELi1ELb0EEEvNS_9DecimArgsE": (153, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_112decim_kernelILi6ELi1ELb0EEEvNS_9DecimArgsE": (153, 0, 3),
    },
    "gf_kernels.hip": {
        "_ZN6sdrhip12_GLOBAL__N_119gf_encode128_kernelENS_10Enc128ArgsE": (113, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_123gf_encode128_fft_kernelENS_10Enc128ArgsE": (96, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_122gf_encode128_bs_kernelENS_10Enc128ArgsE": (96, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_128gf_encode128_fft_half_kernelENS_10Enc128ArgsE": (96, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_124gf_encode128_pack_kernelENS_10Enc128ArgsENS_9FrameArgsEj": (113, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_128gf_encode128_fft_pack_kernelENS_10Enc128ArgsENS_9FrameArgsEj": (96, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_127gf_encode128_bs_pack_kernelENS_10Enc128ArgsENS_9FrameArgsEj": (96, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_120block_scatter_kernelEPKhmiiPhmiiPKsii": (9, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_117fec_header_kernelEPKhmPhmiiiPKii": (8, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_121gf_decode_plan_kernelENS0_11DecPlanArgsE": (58, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_119gf_decode128_kernelENS0_10Dec128ArgsE": (128, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_123gf_decode128_fft_kernelENS0_10Dec128ArgsE": (128, 64, 4),
        "_ZN6sdrhip12_GLOBAL__N_115gf_apply_kernelILi4EEEvNS_6GfArgsE": (52, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_115gf_apply_kernelILi6EEEvNS_6GfArgsE": (61, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_115gf_apply_kernelILi8EEEvNS_6GfArgsE": (83, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_128gf_decode128_fft_plan_kernelILb1EEEvNS0_10Dec128ArgsE": (103, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_128gf_decode128_fft_plan_kernelILb0EEEvNS0_10Dec128ArgsE": (126, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_122gf_decode_apply_kernelILi4EEEvNS0_12DecApplyArgsE": (61, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_122gf_decode_apply_kernelILi6EEEvNS0_12DecApplyArgsE": (79, 0, 6),
    },
    "frame_kernels.hip": {
        "_ZN6sdrhip12_GLOBAL__N_117frame_pack_kernelENS_9FrameArgsE": (26, 0, 8),
    },
    "rx_ragged_kernels.hip": {
        "_ZN6sdrhip12_GLOBAL__N_126decim_simple_ragged_kernelEiiPKsmPsmiiPKNS_9RaggedRowE": (21, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_124frame_pack_ragged_kernelENS_9FrameArgsEPKNS_9RaggedRowE": (26, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi1ELi2ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (64, 0, 7),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi1ELi2ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (89, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi2ELi2ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (83, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi2ELi2ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (91, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi3ELi2ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (85, 0, 5),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi3ELi2ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (93, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi4ELi2ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (85, 0, 4),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi4ELi2ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (93, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi5ELi2ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (85, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi5ELi2ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (93, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi6ELi2ELb1EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (85, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi6ELi2ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (93, 0, 2),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi3ELi0ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (147, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi4ELi0ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (151, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi5ELi0ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (153, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi6ELi0ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (153, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi3ELi1ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (147, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi4ELi1ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (151, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi5ELi1ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (153, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_119decim_ragged_kernelILi6ELi1ELb0EEEvNS_9DecimArgsEPKNS_9RaggedRowE": (153, 0, 3),
        "_ZN6sdrhip12_GLOBAL__N_123iq8_widen_ragged_kernelILi1EEEvPKhmPsmPKNS_9RaggedRowE": (27, 0, 8),
        "_ZN6sdrhip12_GLOBAL__N_123iq8_widen_ragged_kernelILi2EEEvPKhmPsmPKNS_9RaggedRowE": (27, 0, 8),
    },
}


def _resources(stderr):
    names = re.findall(r"Function Name: (\S+)", stderr)
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", stderr)]
    occupancy = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", stderr)]
    assert len(names) == len(vgprs) == len(scratch) == len(occupancy)
    return {n: (v, s, o) for n, v, s, o in zip(names, vgprs, scratch, occupancy)}


def _compile(tmp_path, src):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return _resources(r.stderr)


@pytest.mark.parametrize("src", sorted(PARENT))
def test_kernels_keep_their_resources(tmp_path, src):
    """the shared-record path got no new registers: no kernel of the parent uses scratch where it used none, more VGPRs or runs at a
    lower occupancy; the feature added no kernel (its reads ride in the existing ones)"""
    res = _compile(tmp_path, src)
    parent = PARENT[src]
    assert not set(parent) - set(res), "kernels of the parent are gone: %s" % sorted(set(parent) - set(res))
    assert not set(res) - set(parent), "new kernels need a twin to be held against: %s" % sorted(set(res) - set(parent))
    for n, (vg, sc, occ) in res.items():
        pv, ps, po = parent[n]
        assert sc <= ps, "%s: %d bytes of scratch, the parent %d" % (n, sc, ps)
        assert vg <= pv, "%s: %d VGPRs, the parent %d" % (n, vg, pv)
        assert occ >= po, "%s: occupancy %d, the parent %d" % (n, occ, po)
