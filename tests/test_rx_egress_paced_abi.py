"""CPU-side checks of the paced departure order (SDRHIP_EGRESS_PACED): the define, the Python constant and the name RxPipe.set_egress
takes, the contract written into include/sdrhip.h, NULL handle and no-GPU behaviour as for the other orders; KP
(rx_paced_kernels.hip) compiles for gfx950 to one kernel without scratch and without LDS whose datagram traffic is 16 bytes per lane
and instruction; the kernel and its one launch live where the issue puts them."""
import glob
import inspect
import os
import re
import subprocess

import pytest

from test_iq8_abi import CSRC, HIPCC, ROOT, _compile, _header, built  # noqa: F401


def test_define_constant_and_name(built):
    src = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    assert re.search(r"#define SDRHIP_EGRESS_PACED 2\b", src)
    assert re.search(r"#define SDRHIP_EGRESS_OFF 0\b", src) and re.search(r"#define SDRHIP_EGRESS_ROUND_ROBIN 1\b", src)
    assert built.EGRESS_PACED == 2 and (built.EGRESS_OFF, built.EGRESS_ROUND_ROBIN) == (0, 1)
    lines = open(os.path.join(ROOT, "sdrdaemon_amd", "_lib.py")).read().splitlines()
    assert "EGRESS_PACED = 2" in lines  # (a line of its own: the round-robin pair stays as it was)
    # the three entry points and the struct keep their signatures
    assert "int sdrhip_rx_set_egress(sdrhip_rx *rx, int order);" in src
    assert ("typedef struct { const uint8_t *dgrams; const uint16_t *stream_of; size_t n_dgrams; size_t blocks_per_frame; } "
            "sdrhip_rx_egress;") in src


def test_header_states_the_contract():
    h = _header()
    h = h[h.index("Rx egress"):]
    for word in ("SDRHIP_EGRESS_PACED", "(2 j + 1) / (2 D_s)", "ties by ascending stream", "floor(D_t / D_s) or ceil(D_t / D_s)",
                 "exactly the round-robin array", "(i + 1/2) / n", '"h2d_bytes"', "4 bytes per datagram", "sdrhip_rx_submit_ragged",
                 "sdrhip_rx_submit_datagrams_tagged"):
        assert word in h, word
    assert "other orders" not in h
    assert "other orders" not in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "KP: paced egress" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "SDRHIP_EGRESS_PACED" in open(os.path.join(ROOT, "README.md")).read()


def test_python_surface(built):
    import sdrdaemon_amd as sd
    from sdrdaemon_amd import engine

    assert inspect.signature(sd.RxPipe.set_egress).parameters["order"].default == "round_robin"
    assert "paced" in sd.RxPipe.set_egress.__doc__
    # "paced" reaches the library as 2: the name is looked up before anything touches the handle
    seen = []

    class Lib:
        @staticmethod
        def sdrhip_rx_set_egress(h, order):
            seen.append((h, order))
            return 0

    class Ctx:
        lib = Lib

    class Pipe:
        ctx, h = Ctx, 77

    for name, value in (("paced", 2), ("round_robin", 1), ("off", 0), (None, 0)):
        engine.RxPipe.set_egress(Pipe, name)
        assert seen[-1] == (77, value), name


def test_null_handle_and_no_gpu(built):
    import sdrdaemon_amd as sd

    lib = built.lib()
    assert lib.sdrhip_rx_set_egress(None, 2) == -1
    if sd.device_count() > 0:
        return
    with pytest.raises(sd.SdrHipError):  # (no GPU: no context, no pipe -- never a quiet host path)
        sd.RxPipe(sd.Context(0), 2, nb_fec=8).set_egress("paced")


def test_kp_compiles_to_one_lean_kernel(tmp_path):
    res = _compile(tmp_path, "rx_paced_kernels.hip")
    assert len(res) == 1 and "rx_paced_kernel" in list(res)[0], sorted(res)
    (_, scratch, occ), = res.values()
    assert scratch == 0 and occ == 8, res
    r = subprocess.run([HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(CSRC, "rx_paced_kernels.hip"),
                        "-o", str(tmp_path / "k.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(str(tmp_path / "k.s")).read()
    assert re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", text) == ["0"]      # no LDS
    assert re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text) == ["0"]    # no scratch
    code = [ln.split("//")[0].split(";")[0].strip() for ln in text.splitlines()]
    ops = [ln.split()[0] for ln in code if ln and not ln.startswith(".") and not ln.endswith(":")]
    assert ops.count("global_load_dwordx4") >= 8 and ops.count("global_store_dwordx4") >= 8  # (four per lane: datagrams, records)
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dwordx4"}
    # the table: one dword per datagram, four per lane; everything else moves 16 bytes
    assert {o for o in ops if o.startswith("global_load")} == {"global_load_dwordx4", "global_load_dword"}
    assert ops.count("global_load_dword") == 4
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "ds_", "buffer_", "s_barrier"))]
    loads = [ln for ln in code if ln.startswith("global_load_dwordx4")]
    assert len([ln for ln in loads if " nt" in ln]) >= 8, loads  # (every datagram and record load; the record places are a table)
    # the four table entries first, then all four datagram loads in flight before the first store behind them
    table = [i for i, o in enumerate(ops) if o == "global_load_dword"]
    assert "global_store_dwordx4" not in ops[table[0]:table[-1]] and "global_load_dwordx4" not in ops[table[0]:table[-1]]
    store = table[-1] + ops[table[-1]:].index("global_store_dwordx4")
    assert ops[table[-1]:store].count("global_load_dwordx4") == 4


def test_the_kernel_and_its_launch_live_in_the_new_files():
    text = open(os.path.join(CSRC, "rx_paced_kernels.hip")).read()
    assert text.count("__global__") == 1 and text.count("hipError_t launch_") == 1
    assert "rx_paced_order.h" not in [ln.split()[1].strip('"') for ln in text.splitlines() if ln.startswith("#include")]
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        if os.path.basename(path) != "rx_paced_kernels.hip":
            assert "rx_paced" not in open(path).read(), path
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "rx_paced_kernels.hip" in mk
    calls = {os.path.basename(p): open(p).read().count("launch_rx_paced(") for p in glob.glob(os.path.join(CSRC, "*.cpp"))}
    assert {k: v for k, v in calls.items() if v} == {"sdrhip_rx_egress.cpp": 1}
    # the host side of the order lives in that file alone
    for p in glob.glob(os.path.join(CSRC, "*.cpp")):
        if os.path.basename(p) != "sdrhip_rx_egress.cpp":
            assert "EGRESS_PACED" not in open(p).read() and "RxPacedOrder" not in open(p).read(), p
