"""CPU-side checks of the asynchronous datagram-fed Rx entry (sdrhip_rx_submit_datagrams, sdrhip_rx_collect_datagrams): declared
in include/sdrhip.h with the documented prototypes, exported by libsdrhip.so and reachable from Python, refused loudly without a
GPU, and the new kernels (rx_dgram_async_kernels.hip: the packed instantiations of the collector's scatter and copy passes with
per-stream row offsets, and the delivery kernel KD) compile for gfx950 without scratch, the passes within the registers and
occupancy of the bank's own kernels; KD, the one delivery launch of a batch, moves 16 bytes per lane and access."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "sdrhip_rx_submit_datagrams": "int sdrhip_rx_submit_datagrams(sdrhip_rx *rx, const uint8_t *dgrams, const size_t *n_dgrams, "
                                  "size_t dgram_stride_bytes, const uint32_t *tv_sec, const uint32_t *tv_usec);",
    "sdrhip_rx_collect_datagrams": "int sdrhip_rx_collect_datagrams(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, "
                                   "size_t max_frames, size_t max_released, sdrhip_fecbuf_frame *info_out, size_t *n_released, "
                                   "size_t *n_frames, int wait);",
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

    assert list(inspect.signature(sd.RxPipe.submit_datagrams).parameters)[1:] == ["dgrams_per_stream", "tv_sec", "tv_usec"]
    assert list(inspect.signature(sd.RxPipe.collect_datagrams).parameters)[1:] == ["wait", "max_frames", "max_released"]
    p = inspect.signature(sd.RxPipe.submit_datagrams).parameters
    assert p["tv_sec"].default == 0 and p["tv_usec"].default == 0
    p = inspect.signature(sd.RxPipe.collect_datagrams).parameters
    assert p["wait"].default is True and p["max_frames"].default is None and p["max_released"].default is None


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    nd, nr, nf = (C.c_size_t * 1)(0), (C.c_size_t * 1)(), (C.c_size_t * 1)()
    st = (C.c_uint32 * 1)(0)
    # NULL handle: SDRHIP_EINVAL; a handle cannot be made without a GPU: SDRHIP_EDEVICE
    assert lib.sdrhip_rx_submit_datagrams(None, None, nd, 0, st, st) == -1
    assert lib.sdrhip_rx_collect_datagrams(None, None, 0, 0, 0, None, nr, nf, 1) == -1
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 2).submit_datagrams([np.zeros((1, 512), np.uint8)] * 2)


def _pick(d, name):
    k = "%d%s" % (len(name), name)
    return [v for n, v in d.items() if k in n]


def test_new_kernels_compile_without_scratch(tmp_path):
    """the fourth instantiation of fecbuf_passes.h (packed datagrams in, payloads behind a per-stream row offset) and KD: three
    kernels, no scratch; the passes take no more VGPR granules and have no less occupancy than the bank's own scatter / copy kernels"""
    res = iq8._compile(tmp_path, "rx_dgram_async_kernels.hip")
    assert len(res) == 3, sorted(res)
    (vg, sc, occ), = _pick(res, "rx_deliver_kernel")
    assert occ == 8, (vg, sc, occ)
    for n, (vg, sc, occ) in res.items():
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
    (tmp_path / "b").mkdir()
    bank = iq8._compile(tmp_path / "b", "fecbuf_kernels.hip")
    for name, base in (("fecbuf_scatter_packed_rows_kernel", "fecbuf_scatter_kernel"), ("fecbuf_copy_guarded_rows_kernel", "fecbuf_copy_kernel")):
        (vg, _, occ), = _pick(res, name)
        (vb, _, ob), = _pick(bank, base)
        print(name, "vgprs", vg, "occupancy", occ, "| bank", vb, ob)
        assert (vg + 7) // 8 <= (vb + 7) // 8 and occ >= ob, (name, vg, vb, occ, ob)


def test_the_other_kernel_files_keep_their_kernel_sets():
    """the new instantiation lives in its own file: no other file includes the passes with both FB_PACKED and FB_ROWS set"""
    both = []
    for f in sorted(os.listdir(iq8.CSRC)):
        if not f.endswith(".hip"):
            continue
        t = open(os.path.join(iq8.CSRC, f)).read()
        if re.search(r"#define FB_PACKED 1", t) and re.search(r"#define FB_ROWS 1", t):
            both.append(f)
    assert both == ["rx_dgram_async_kernels.hip"]


def test_delivery_moves_16_bytes_per_lane(tmp_path):
    """the one delivery launch of a batch (frames from the sliding windows, then the records): 16-byte vector loads and stores and
    nothing narrower, as the ragged batches' gathers"""
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    host = open(os.path.join(iq8.CSRC, "sdrhip_rx_datagrams_async.cpp")).read()
    assert host.count("launch_rx_deliver(") == 1 and "launch_frame_gather(" not in host and "launch_delivery_gather(" not in host
    out = tmp_path / "k.s"
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(iq8.CSRC, "rx_dgram_async_kernels.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = 0
    for body in re.split(r"\n(?=_ZN\S+:)", out.read_text()):
        m = re.match(r"(_ZN\S+):", body)
        if not m or "rx_deliver_kernel" not in m.group(1):
            continue
        seen += 1
        body = body.split(".Lfunc_end")[0]  # (the instructions alone)
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, m.group(1)
        assert not re.search(r"flat_(load|store)|scratch_|global_store_(dword|short|byte)\b", body), m.group(1)
    assert seen == 1
