"""CPU-side checks of the asynchronous datagram-fed Tx entry (sdrhip_tx_submit_datagrams, sdrhip_tx_collect_datagrams): declared
in include/sdrhip.h with the documented prototypes, exported by libsdrhip.so and reachable from Python, refused loudly without a
GPU, and the new kernels (tx_async_kernels.hip, the packed instantiations of fecbuf_kernels.hip) compile for gfx950 without scratch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "sdrhip_tx_submit_datagrams": "int sdrhip_tx_submit_datagrams(sdrhip_tx *tx, const uint8_t *dgrams, const size_t *n_dgrams, "
                                  "size_t dgram_stride_bytes);",
    "sdrhip_tx_collect_datagrams": "int sdrhip_tx_collect_datagrams(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t max_frames, "
                                   "uint8_t *block0_out, sdrhip_fecbuf_frame *info_out, size_t *n_frames, int wait);",
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


def test_python_surface():
    import sdrdaemon_amd as sd

    for m in ("submit_datagrams", "collect_datagrams"):
        assert hasattr(sd.TxPipe, m), m


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    nd, nf = (C.c_size_t * 1)(0), (C.c_size_t * 1)()
    # NULL handle / NULL counts: SDRHIP_EINVAL; a handle cannot be made without a GPU: SDRHIP_EDEVICE
    assert lib.sdrhip_tx_submit_datagrams(None, None, nd, 0) == -1
    assert lib.sdrhip_tx_collect_datagrams(None, None, 0, 0, None, None, nf, 1) == -1
    with pytest.raises(sd.SdrHipError) as e:
        sd.TxPipe(sd.Context(0), 2).submit_datagrams([np.zeros((1, 512), np.uint8)] * 2)
    assert e.value.code == -3  # SDRHIP_EDEVICE


def test_new_kernels_compile_without_scratch(tmp_path):
    """the shadow check, the delivery gather and the packed instantiations of the collector's passes (fecbuf_passes.h): no scratch,
    and no more registers than the FEC buffer bank's own kernels"""
    res = iq8._compile(tmp_path, "tx_async_kernels.hip")
    assert len(res) == 5, sorted(res)
    for n, (vg, sc, occ) in res.items():
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
    bank = iq8._compile(tmp_path, "fecbuf_kernels.hip")

    def pick(d, name):
        k = "%d%s" % (len(name), name)
        return [v for n, v in d.items() if k in n]

    assert len(pick(res, "fecbuf_shadow_check_kernel")) == len(pick(res, "delivery_gather_kernel")) == 1
    for name, base in (("fecbuf_classify_packed_kernel", "fecbuf_classify_kernel"), ("fecbuf_scatter_packed_kernel", "fecbuf_scatter_kernel"),
                       ("fecbuf_copy_guarded_kernel", "fecbuf_copy_kernel")):
        (vg, _, _), = pick(res, name)
        (vb, _, _), = pick(bank, base)
        assert vg <= vb, (name, vg, vb)
