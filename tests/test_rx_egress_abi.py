"""CPU-side checks of the departure-order egress (sdrhip_rx_set_egress / sdrhip_rx_collect_egress / sdrhip_rx_release_egress):
declared in include/sdrhip.h with the signatures the issue gives, exported, bound in Python, refused loudly without a GPU; KE
(rx_egress_kernels.hip) compiles for gfx950 to one kernel without scratch whose global traffic is 16 bytes per lane and
instruction; the new kernel and its one launch live in the new files alone."""
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
    res = _compile(tmp_path, "rx_egress_kernels.hip")
    assert len(res) == 1 and "rx_egress_kernel" in list(res)[0], sorted(res)
    (_, scratch, occ), = res.values()
    assert scratch == 0 and occ == 8, res
    r = subprocess.run([HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(CSRC, "rx_egress_kernels.hip"),
                        "-o", str(tmp_path / "k.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    code = [ln.split("//")[0].split(";")[0].strip() for ln in open(str(tmp_path / "k.s"))]
    ops = [ln.split()[0] for ln in code if ln and not ln.startswith(".") and not ln.endswith(":")]
    assert ops.count("global_load_dwordx4") >= 8 and ops.count("global_store_dwordx4") >= 8  # (four per lane: frames, records)
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dwordx4"}
    assert {o for o in ops if o.startswith("global_load")} == {"global_load_dwordx4"}  # (a frame's run comes through the scalar cache)
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "ds_", "buffer_", "s_barrier"))]
    loads = [ln for ln in code if ln.startswith("global_load_dwordx4")]
    assert len([ln for ln in loads if " nt" in ln]) >= 8, loads  # (every frame and record load; the record places are a table)


def test_the_kernel_and_its_launch_live_in_the_new_files():
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        if os.path.basename(path) != "rx_egress_kernels.hip":
            assert "rx_egress" not in open(path).read(), path
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "rx_egress_kernels.hip" in mk and "sdrhip_rx_egress.cpp" in mk
    calls = {os.path.basename(p): open(p).read().count("launch_rx_egress(") for p in glob.glob(os.path.join(CSRC, "*.cpp"))}
    assert {k: v for k, v in calls.items() if v} == {"sdrhip_rx_egress.cpp": 1}
    # each launch path reaches it through one branch
    for name in ("sdrhip_rx_datagrams_async.cpp", "sdrhip_rx_async.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert text.count("rx_egress_launch(") == 1 and text.count("rx_egress_room(") == 1, name
