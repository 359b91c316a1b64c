"""CPU-side checks of the departure-order egress (sdrhip_rx_set_egress / sdrhip_rx_collect_egress / sdrhip_rx_release_egress):
declared in include/sdrhip.h with the signatures the issue gives, exported, bound in Python, refused loudly without a GPU; the
kernel that serves round robin (KR, rx_runs_kernels.hip) compiles for gfx950 to one kernel without scratch whose global traffic is
16 bytes per lane and instruction; KE is gone, and each remaining delivery kernel has its one launch in sdrhip_rx_egress.cpp."""
import ctypes as C
import glob
import inspect
import os
import re
import subprocess

import pytest

from test_iq8_abi import CSRC, HIPCC, ROOT, _compile, _header, built  # noqa: F401

NAMES = ["sdrhip_rx_set_egress", "sdrhip_rx_collect_egress", "sdrhip_rx_release_egress"]


def test_declared_exported_and_bound(built):
    src = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    lib = built.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in built.EXPORTS, n
    assert "int sdrhip_rx_set_egress(sdrhip_rx *rx, int order);" in src
    assert ("int sdrhip_rx_collect_egress(sdrhip_rx *rx, sdrhip_rx_egress *out, size_t *n_frames, size_t max_released, "
            "sdrhip_fecbuf_frame *info_out, size_t *n_released, int wait);") in src
    assert "int sdrhip_rx_release_egress(sdrhip_rx *rx);" in src
    assert re.search(r"#define SDRHIP_EGRESS_OFF 0\b", src) and re.search(r"#define SDRHIP_EGRESS_ROUND_ROBIN 1\b", src)
    assert ("typedef struct { const uint8_t *dgrams; const uint16_t *stream_of; size_t n_dgrams; size_t blocks_per_frame; } "
            "sdrhip_rx_egress;") in src
    assert (built.EGRESS_OFF, built.EGRESS_ROUND_ROBIN) == (0, 1)
    sz, vp = C.c_size_t, C.c_void_p
    assert lib.sdrhip_rx_set_egress.argtypes == [vp, C.c_int]
    assert lib.sdrhip_rx_collect_egress.argtypes == [vp, C.POINTER(built.RxEgress), C.POINTER(sz), sz, vp, C.POINTER(sz), C.c_int]
    assert lib.sdrhip_rx_release_egress.argtypes == [vp]
    assert [f[0] for f in built.RxEgress._fields_] == ["dgrams", "stream_of", "n_dgrams", "blocks_per_frame"]
    assert C.sizeof(built.RxEgress) == 2 * C.sizeof(vp) + 2 * C.sizeof(sz)


def test_header_cites_the_reference_and_states_the_rules():
    h = _header()
    for cite in ("UDPSinkFEC.cpp:259-282", "sdrdaemonrx.cpp:607-613"):
        assert cite in h, cite
    for word in ("sdrhip_rx_release_egress", "lent", "SDRHIP_EBUSY", '"d2h_bytes"'):
        assert word in h[h.index("Rx egress"):], word


def test_python_surface(built):
    import sdrdaemon_amd as sd

    assert list(inspect.signature(sd.RxPipe.set_egress).parameters) == ["self", "order"]
    assert inspect.signature(sd.RxPipe.set_egress).parameters["order"].default == "round_robin"
    p = inspect.signature(sd.RxPipe.collect_egress).parameters
    assert list(p) == ["self", "wait", "max_released", "copy"]
    assert (p["wait"].default, p["max_released"].default, p["copy"].default) == (True, None, True)
    assert list(inspect.signature(sd.RxPipe.release_egress).parameters) == ["self"]


def test_null_handle_and_no_gpu(built):
    import sdrdaemon_amd as sd

    lib = built.lib()
    eg = built.RxEgress()
    nf = (C.c_size_t * 1)()
    assert lib.sdrhip_rx_set_egress(None, 1) == -1
    assert lib.sdrhip_rx_collect_egress(None, C.byref(eg), nf, 0, None, None, 1) == -1
    assert lib.sdrhip_rx_release_egress(None) == -1
    if sd.device_count() > 0:
        return
    with pytest.raises(sd.SdrHipError):  # (no GPU: no context, no pipe -- never a quiet host path)
        sd.RxPipe(sd.Context(0), 2, nb_fec=8).set_egress("round_robin")


def test_ke_compiles_to_one_lean_kernel(tmp_path):
    """round-robin batches of equal frames are KR's now: one kernel (rx_runs_kernel), no scratch, occupancy 8, dwordx4 global
    traffic alone, at least 8 nt loads, no flat / scratch / LDS / buffer / barrier instruction -- the list KE was held against"""
    from test_rx_stream_fec_abi import KR, check_kr_is_one_lean_kernel

    assert KR == "rx_runs_kernels.hip"
    check_kr_is_one_lean_kernel(tmp_path)


def test_the_kernel_and_its_launch_live_in_the_new_files():
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")):
        text = open(path).read()
        assert "rx_egress_kernel" not in text and "launch_rx_egress" not in text, path
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "rx_egress_kernels.hip" not in mk and "sdrhip_rx_egress.cpp" in mk
    for launch in ("launch_rx_runs(", "launch_rx_paced("):
        calls = {os.path.basename(p): open(p).read().count(launch) for p in glob.glob(os.path.join(CSRC, "*.cpp"))}
        assert {k: v for k, v in calls.items() if v} == {"sdrhip_rx_egress.cpp": 1}, launch
    # each launch path reaches it through one branch
    for name in ("sdrhip_rx_datagrams_async.cpp", "sdrhip_rx_async.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert text.count("rx_egress_launch(") == 1 and text.count("rx_egress_room(") == 1, name
