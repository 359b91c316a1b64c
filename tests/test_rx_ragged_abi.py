"""CPU-side checks of the ragged Rx bank (sdrhip_decimate_ragged, sdrhip_rx_process_ragged, sdrhip_rx_frames_view_ragged): declared
in include/sdrhip.h with the documented prototypes, exported by libsdrhip.so, refused loudly without a GPU, and the new kernels
(rx_ragged_kernels.hip) compile for gfx950 without scratch and with no more VGPRs than their uniform twins."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "sdrhip_decimate_ragged": "int sdrhip_decimate_ragged(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, "
                              "const int16_t *iq_in, const size_t *n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, "
                              "size_t *n_out, int mem);",
    "sdrhip_rx_process_ragged": "int sdrhip_rx_process_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, "
                                "const uint32_t *tv_sec, const uint32_t *tv_usec, uint8_t *frames_out, size_t frame_stride_bytes, "
                                "size_t *n_frames, int mem);",
    "sdrhip_rx_frames_view_ragged": "int sdrhip_rx_frames_view_ragged(const sdrhip_rx *rx, const uint8_t **base, "
                                    "size_t *stream_stride_bytes, size_t *first_slot, size_t *n_frames);",
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
    import sdrdaemon_amd as sd

    for m in ("process_ragged", "process_view_ragged", "frames_view_ragged"):
        assert hasattr(sd.RxPipe, m), m
    assert hasattr(sd.Decimators, "decimate_ragged")
    from sdrdaemon_amd import engine

    assert list(engine._counts([3, 0, 5], 3, 5)) == [3, 0, 5]
    for bad in ([1, 2], [1, 2, 6], [-1, 0, 0]):
        with pytest.raises(ValueError):
            engine._counts(bad, 3, 5)


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    n = (C.c_size_t * 1)(4)
    assert lib.sdrhip_rx_process_ragged(None, None, n, 4, None, None, None, 0, None, 0) == -1
    assert lib.sdrhip_rx_frames_view_ragged(None, None, None, None, None) == -1
    ss = C.c_uint(16)
    assert lib.sdrhip_decimate_ragged(None, 4, 2, C.byref(ss), None, n, 4, None, 4, n, 0) == -1
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 2).process_ragged(np.zeros((2, 64, 2), np.int16), [64, 3])


def test_ragged_kernels_compile_without_scratch_and_within_their_twins(tmp_path):
    rag = iq8._compile(tmp_path, "rx_ragged_kernels.hip")
    (tmp_path / "u").mkdir()
    uni = iq8._compile(tmp_path / "u", "decim_kernels.hip")
    (tmp_path / "f").mkdir()
    uni.update(iq8._compile(tmp_path / "f", "frame_kernels.hip"))
    (tmp_path / "c").mkdir()
    uni.update(iq8._compile(tmp_path / "c", "convert_kernels.hip"))
    k1r = {n: v for n, v in rag.items() if "decim_ragged_kernel" in n}
    assert len(k1r) == 6 * 2 + 4 + 4, sorted(k1r)  # cen 1..6 x packed / not, inf 3..6, sup 3..6
    assert len(rag) == len(k1r) + 4, sorted(rag)  # + K0r U8 / S8, K2r, the filter-less kernel

    def twin(n):
        """the uniform kernel of the same instantiation (mangled names: the ragged ones take the table as an extra argument)"""
        n = n.replace("PKNS_9RaggedRowE", "")
        n = n.replace("19decim_ragged_kernel", "12decim_kernel").replace("24frame_pack_ragged_kernel", "17frame_pack_kernel")
        n = n.replace("23iq8_widen_ragged_kernelILi1EEEvPKhmPsm", "16iq8_widen_kernelILi1EEEvPKhmPsmm")
        n = n.replace("23iq8_widen_ragged_kernelILi2EEEvPKhmPsm", "16iq8_widen_kernelILi2EEEvPKhmPsmm")
        return n.replace("_ZN6sdrhip12_GLOBAL__N_126decim_simple_ragged_kernelEiiPKsmPsmii", "_ZN6sdrhip19decim_simple_kernelEiiPKsmPsmmii")

    for n, (vg, sc, occ) in rag.items():
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        t = twin(n)
        assert t in uni, (n, t)
        assert vg <= uni[t][0], "%s: %d VGPRs, its uniform twin %d" % (n, vg, uni[t][0])
        assert occ >= uni[t][2], "%s: occupancy %d, its uniform twin %d" % (n, occ, uni[t][2])


def test_ragged_matrix_core_kernels_within_their_twins(tmp_path):
    """K1mr (decim_mfma.hip): every instantiation without scratch, no more VGPRs and no lower occupancy than its uniform twin"""
    res = iq8._compile(tmp_path, "decim_mfma.hip")
    rag = {n: v for n, v in res.items() if "decim_mfma_ragged_kernel" in n}
    assert len(rag) == 24, sorted(rag)  # decimate4 .. 64 x packed / not x frame / stream order, + decimate16 with the ring of 3
    for n, (vg, sc, occ) in rag.items():
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        t = n.replace("24decim_mfma_ragged_kernel", "17decim_mfma_kernel").replace("PKNS_9RaggedRowE", "")
        assert t in res, (n, t)
        assert occ >= res[t][2], "%s: occupancy %d, its uniform twin %d" % (n, occ, res[t][2])
        if "ILi6ELb1ELi4ELb1E" in n:  # decimate64, packed first stage, frame-layout stores: 236 against 204, both two waves per SIMD
            assert vg <= 256, "%s: %d VGPRs" % (n, vg)  # (the one instantiation above its twin)
        else:
            assert vg <= res[t][0], "%s: %d VGPRs, its uniform twin %d" % (n, vg, res[t][0])
