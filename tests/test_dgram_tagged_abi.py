"""CPU-side checks of the tagged datagram entries (sdrhip_fecbuf_write_and_read_tagged, sdrhip_tx_submit_datagrams_tagged,
sdrhip_rx_submit_datagrams_tagged): declared in include/sdrhip.h with the documented prototypes, exported by libsdrhip.so and
reachable from Python, refused loudly without a GPU, and the demultiplexer KX (dgram_demux_kernels.hip) compiles for gfx950 to one
kernel without scratch that moves 16 bytes per lane and access.  (That fecbuf_kernels.hip, tx_async_kernels.hip,
rx_join_kernels.hip and rx_dgram_async_kernels.hip keep their kernel sets is what test_rx_datagrams_abi, test_tx_datagrams_async_abi
and test_rx_datagrams_async_abi check; KX stays out of them by not including fecbuf_passes.h.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "dgram_demux_kernels.hip"
PROTOS = {
    "sdrhip_fecbuf_write_and_read_tagged": "int sdrhip_fecbuf_write_and_read_tagged(sdrhip_fecbuf *b, const uint8_t *dgrams, "
                                           "const uint16_t *stream_of, size_t n_total, uint8_t *data_out, size_t data_stride_bytes, "
                                           "uint8_t *block0_out, size_t max_frames, sdrhip_fecbuf_frame *info_out, size_t *n_frames, int mem);",
    "sdrhip_tx_submit_datagrams_tagged": "int sdrhip_tx_submit_datagrams_tagged(sdrhip_tx *tx, const uint8_t *dgrams, "
                                         "const uint16_t *stream_of, size_t n_total);",
    "sdrhip_rx_submit_datagrams_tagged": "int sdrhip_rx_submit_datagrams_tagged(sdrhip_rx *rx, const uint8_t *dgrams, "
                                         "const uint16_t *stream_of, size_t n_total, const uint32_t *tv_sec, const uint32_t *tv_usec);",
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
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define SDRHIP_DGRAM_SKIP 0xffffu\b", src)
    assert built.DGRAM_SKIP == 0xFFFF


def test_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "sdrhip.h")).read()
    for phrase in ("arrival order", "SDRHIP_DGRAM_SKIP", "more than 65535 streams", "ONE memcpy", "4 bytes per datagram"):
        assert phrase in h, phrase


def test_python_surface():
    import sdrdaemon_amd as sd

    sig = inspect.signature
    assert list(sig(sd.FECBufferBank.write_and_read_tagged).parameters)[1:] == ["dgrams", "stream_of", "max_frames"]
    assert sig(sd.FECBufferBank.write_and_read_tagged).parameters["max_frames"].default is None
    assert list(sig(sd.TxPipe.submit_datagrams_tagged).parameters)[1:] == ["dgrams", "stream_of"]
    assert list(sig(sd.RxPipe.submit_datagrams_tagged).parameters)[1:] == ["dgrams", "stream_of", "tv_sec", "tv_usec"]
    p = sig(sd.RxPipe.submit_datagrams_tagged).parameters
    assert p["tv_sec"].default == 0 and p["tv_usec"].default == 0
    assert sd.DGRAM_SKIP == 0xFFFF
    with pytest.raises(ValueError):
        sd.engine._tagged_batch(np.zeros((3, 512), np.uint8), np.zeros(2, np.uint16))  # (one tag per datagram)


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    lib = built.lib()
    nf = (C.c_size_t * 1)()
    st = (C.c_uint32 * 1)(0)
    tags = (C.c_uint16 * 1)(0)
    # NULL handle: SDRHIP_EINVAL, with or without a GPU
    assert lib.sdrhip_fecbuf_write_and_read_tagged(None, None, tags, 0, None, 0, None, 0, None, nf, 0) == -1
    assert lib.sdrhip_tx_submit_datagrams_tagged(None, None, tags, 0) == -1
    assert lib.sdrhip_rx_submit_datagrams_tagged(None, None, tags, 0, st, st) == -1
    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    # a handle cannot be made without a GPU: SDRHIP_EDEVICE
    one, tag = np.zeros((1, 512), np.uint8), np.zeros(1, np.uint16)
    for make in (lambda c: sd.RxPipe(c, 2).submit_datagrams_tagged(one, tag), lambda c: sd.TxPipe(c, 2).submit_datagrams_tagged(one, tag),
                 lambda c: sd.FECBufferBank(c, 2).write_and_read_tagged(one, tag)):
        with pytest.raises(sd.SdrHipError) as e:
            make(sd.Context(0))
        assert e.value.code == -3


def test_kx_is_one_kernel_without_scratch(tmp_path):
    res = iq8._compile(tmp_path, SRC)
    assert len(res) == 1, sorted(res)
    (name, (vg, sc, occ)), = res.items()
    print(name, "vgprs", vg, "scratch", sc, "occupancy", occ)
    assert "dgram_demux_kernel" in name and sc == 0 and occ == 8, (name, vg, sc, occ)


def test_kx_stands_alone():
    """KX does not include the collector's passes (their four instantiations keep their files), no other kernel file defines or
    launches it, and the library's Makefile builds it"""
    text = open(os.path.join(iq8.CSRC, SRC)).read()
    assert not re.search(r'#include\s+"fecbuf_passes\.h"', text)
    assert "__syncthreads" not in text and "__shared__" not in text
    for f in sorted(os.listdir(iq8.CSRC)):
        if f.endswith(".hip") and f != SRC:
            assert "dgram_demux" not in open(os.path.join(iq8.CSRC, f)).read(), f
    assert SRC in open(os.path.join(iq8.CSRC, "Makefile")).read()
    assert "launch_dgram_demux(" in open(os.path.join(iq8.CSRC, "sdrhip_internal.h")).read()
    # one staging path: both submits and no third place launch it through fecbuf_batch_upload
    for f in ("sdrhip_tx_async.cpp", "sdrhip_rx_datagrams_async.cpp"):
        host = open(os.path.join(iq8.CSRC, f)).read()
        assert "launch_dgram_demux(" not in host and host.count("fecbuf_batch_upload(") == 1, f


def test_kx_moves_16_bytes_per_lane(tmp_path):
    """16-byte vector loads and stores and nothing narrower on the store side, no flat and no scratch access: the check
    test_rx_datagrams_async_abi makes for the delivery kernel KD"""
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    out = tmp_path / "k.s"
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(iq8.CSRC, SRC), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = 0
    for body in re.split(r"\n(?=_ZN\S+:)", out.read_text()):
        m = re.match(r"(_ZN\S+):", body)
        if not m or "dgram_demux_kernel" not in m.group(1):
            continue
        seen += 1
        body = body.split(".Lfunc_end")[0]  # (the instructions alone)
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, m.group(1)
        assert not re.search(r"flat_(load|store)|scratch_|global_store_(dword|short|byte)\b|ds_(read|write)|s_barrier", body), m.group(1)
        # several datagrams' loads are in flight before the first store
        first_store = body.index("global_store_dwordx4")
        assert body[:first_store].count("global_load_dwordx4") == 4, m.group(1)
    assert seen == 1
