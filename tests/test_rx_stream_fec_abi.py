"""CPU-side checks of the per-stream fecblk (sdrhip_rx_set_stream_fec / sdrhip_rx_get_stream_fec / sdrhip_rx_egress_stream_blocks):
declared in include/sdrhip.h with their citations, exported, bound in Python, refused loudly without a GPU; the property of CM256
the design rests on (recovery row r does not depend on the recovery count), on the oracle and on the independent statement of the
code; the departure order of frames of different lengths (sdrdaemon_amd/csrc/rx_depart_order.h) against a literal simulation of
the rounds, both from Python through rounds() of tests/test_gpu_rx_egress.py's definition and as a stand-alone program built with
the address and undefined-behaviour sanitizers; KR (rx_runs_kernels.hip) compiles for gfx950 to one lean kernel."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cm256_spec
from test_iq8_abi import CSRC, HIPCC, ROOT, _compile, _header, built  # noqa: F401

NAMES = ["sdrhip_rx_set_stream_fec", "sdrhip_rx_get_stream_fec", "sdrhip_rx_egress_stream_blocks"]
CXX = os.path.join(ROOT, "tests", "cxx", "rx_depart_order_test.cpp")
KR = "rx_runs_kernels.hip"


def test_declared_exported_and_bound(built):
    src = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    lib = built.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in built.EXPORTS, n
    assert "int sdrhip_rx_set_stream_fec(sdrhip_rx *rx, const int *nb_fec);" in src
    assert "int sdrhip_rx_get_stream_fec(const sdrhip_rx *rx, int stream, int *nb_fec, int *slot_blocks);" in src
    assert "int sdrhip_rx_egress_stream_blocks(const sdrhip_rx *rx, size_t *blocks);" in src
    sz, vp, ip = C.c_size_t, C.c_void_p, C.POINTER(C.c_int)
    assert lib.sdrhip_rx_set_stream_fec.argtypes == [vp, ip]
    assert lib.sdrhip_rx_get_stream_fec.argtypes == [vp, C.c_int, ip, ip]
    assert lib.sdrhip_rx_egress_stream_blocks.argtypes == [vp, C.POINTER(sz)]


def test_header_cites_the_reference_and_states_the_rules():
    h = _header()
    at = h.index("int sdrhip_rx_set_stream_fec")
    comment = re.sub(r"\s+", " ", h[h.rindex("/*", 0, at):at])
    for cite in ("sdrdaemonrx.cpp:599-605", "UDPSinkFEC.cpp:160-165", "UDPSinkFEC.cpp:228-256"):
        assert cite in comment, cite
    for word in ("0..128", "NULL = bank-wide again", "byte for byte", "sdrhip_rx_reconfigure", "sdrhip_rx_reset_streams", "ONE slot pitch",
                 "slot_blocks = 128 + max_s nb_fec[s]", "sdrhip_rx_set_pipelined(1)", "departure order only", "sdrhip_rx_set_egress",
                 "blocks_per_frame is 0", "Not covered", "KD"):
        assert word in comment, word


def test_python_surface(built):
    import sdrdaemon_amd as sd

    p = inspect.signature(sd.RxPipe.set_stream_fec).parameters
    assert list(p) == ["self", "nb_fec"] and p["nb_fec"].default is None
    assert list(inspect.signature(sd.RxPipe.stream_fec).parameters) == ["self", "stream"]
    assert "last_stream_blocks" in inspect.getsource(sd.RxPipe.collect_egress)


def test_null_handle_and_no_gpu(built):
    import sdrdaemon_amd as sd

    lib = built.lib()
    r, sb = C.c_int(0), C.c_int(0)
    blocks = (C.c_size_t * 2)()
    fec = (C.c_int * 2)(4, 32)
    assert lib.sdrhip_rx_set_stream_fec(None, fec) == -1
    assert lib.sdrhip_rx_set_stream_fec(None, None) == -1
    assert lib.sdrhip_rx_get_stream_fec(None, 0, C.byref(r), C.byref(sb)) == -1
    assert lib.sdrhip_rx_egress_stream_blocks(None, blocks) == -1
    assert b"NULL" in lib.sdrhip_last_error()
    if sd.device_count() > 0:
        return
    with pytest.raises(sd.SdrHipError):  # (no GPU: no context, no pipe -- never a quiet host path)
        sd.RxPipe(sd.Context(0), 2, nb_fec=8).set_stream_fec([4, 32])


# ------------------------------------------------------------------------------------------------ the property of CM256
ROWS = [(r, R) for r in (1, 12, 13, 32, 33, 127) for R in sorted({r, 32, 128}) if R >= r]


def test_recovery_rows_do_not_depend_on_the_count_oracle(oracle):
    """oracle.frame_encode(f, R)[:r] == oracle.frame_encode(f, r): a frame encoded with R >= r rows carries the r-row encoding"""
    rs = np.random.RandomState(5)
    frame = rs.randint(0, 256, (128, 512)).astype(np.uint8)
    enc = {R: oracle.frame_encode(frame, R) for R in sorted({R for _, R in ROWS} | {r for r, _ in ROWS})}
    for r, R in ROWS:
        assert enc[R].shape == (R, 512) and np.array_equal(enc[R][:r], enc[r]), (r, R)


def test_recovery_rows_do_not_depend_on_the_count_spec():
    """the same on the independent statement of the code (tests/cm256_spec.py): the matrix rows and an encoding"""
    spec = cm256_spec.field()
    rs = np.random.RandomState(6)
    x = rs.randint(0, 256, (128, 24)).astype(np.uint8)
    mats = {R: cm256_spec._matrix(spec, 128, R) for R in sorted({R for _, R in ROWS} | {r for r, _ in ROWS})}
    enc128 = cm256_spec._encode(spec, x, 128)
    for r, R in ROWS:
        assert np.array_equal(mats[R][:r], mats[r]), (r, R)
    for r in (1, 13, 33):
        assert np.array_equal(enc128[:r], cm256_spec._encode(spec, x, r)), r


# ------------------------------------------------------------------------------------------------ the order
def rounds(per_stream):
    """the definition, literally (rounds() of tests/test_gpu_rx_egress.py, which needs a GPU to import): per stream an (n_s, B_s,
    512) array in wire order -> (datagrams (N, 512), tags (N,))"""
    rows = [np.asarray(f).reshape(-1, 512) for f in per_stream]
    out, tags, j = [], [], 0
    while True:
        live = [s for s, r in enumerate(rows) if r.shape[0] > j]
        if not live:
            break
        for s in live:
            out.append(rows[s][j])
            tags.append(s)
        j += 1
    return (np.stack(out) if out else np.zeros((0, 512), np.uint8)), np.asarray(tags, np.uint16)


def test_rounds_is_the_gpu_suites_definition():
    """the copy above is tests/test_gpu_rx_egress.py's rounds(), line for line"""
    theirs = open(os.path.join(ROOT, "tests", "test_gpu_rx_egress.py")).read()
    body = theirs[theirs.index("def rounds(per_stream):"):theirs.index("def same_as_twin")]
    mine = inspect.getsource(rounds)
    code = lambda s: [ln.strip() for ln in s.split('"""')[-1].splitlines() if ln.strip()]  # noqa: E731
    assert code(mine) == code(body)


def test_order_header_stands_alone():
    """rx_depart_order.h is C++11 and pulls in neither HIP nor a library header: standard headers, and the constants it shares with
    rx_paced_order.h (rx_egress_limits.h, which includes two standard headers and nothing else)"""
    with open(os.path.join(CSRC, "rx_depart_order.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(incs) == ['"rx_egress_limits.h"', "<algorithm>", "<cstddef>", "<cstdint>", "<vector>"]
    with open(os.path.join(CSRC, "rx_egress_limits.h")) as f:
        assert sorted(ln.split()[1] for ln in f if ln.startswith("#include")) == ["<cstddef>", "<cstdint>"]
    with open(CXX) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"rx_depart_order.h"']


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    """tests/cxx/rx_depart_order_test.cpp, built once with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path_factory.mktemp("depart") / "rx_depart_order_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, CXX, "-o", exe], check=True)
    return exe


def test_order_equals_rounds_over_labelled_datagrams(replay):
    """the array as the class orders it against rounds() over datagrams that carry their own (stream, index): PLAN's frame counts
    with B = [128, 129, 160, 255, 256] and with the hub's [128, 129, 160, 255, 132]; equal counts; one stream alone"""
    plan = json.loads(re.search(r"PLAN = (\[\[.*?\]\])", open(os.path.join(ROOT, "tests", "test_gpu_rx_egress.py")).read()).group(1))
    cases = [(F, B) for F in plan for B in ([128, 129, 160, 255, 256], [128, 129, 160, 255, 132], [160] * 5)] + [([3], [129]), ([0, 2], [256, 128])]
    for F, B in cases:
        per = []
        for s, (f, b) in enumerate(zip(F, B)):
            a = np.zeros((f, b, 512), np.uint8)
            j = np.arange(f * b, dtype=np.uint32).reshape(f, b)
            a[:, :, 0], a[:, :, 1], a[:, :, 2] = s, j & 255, j >> 8
            per.append(a)
        dg, tags = rounds(per)
        r = subprocess.run([replay, "dump", str(len(F))] + [str(x) for x in F + B], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        got = np.array([ln.split() for ln in r.stdout.split("\n") if ln], dtype=np.int64).reshape(-1, 2)
        assert got.shape[0] == dg.shape[0] == sum(f * b for f, b in zip(F, B)), (F, B)
        assert np.array_equal(got[:, 0], tags) and np.array_equal(got[:, 0], dg[:, 0]), (F, B)
        assert np.array_equal(got[:, 1], dg[:, 1].astype(np.int64) | dg[:, 2].astype(np.int64) << 8), (F, B)


def test_order_matches_a_simulation_of_the_rounds(replay):
    """positions, tags, totals, run count <= sum F + S (S - 1), every run inside one frame, 16-byte alignment; equal counts
    reproduce the closed form base_f + b A_f + r_f(s) and the equal-frames plan; B = [128, 129, 160, 255, 256] over PLAN; F = 0 first / middle / last; one stream; cuts at a frame's
    first and last datagram and at offsets 1, 31, 32, 33"""
    src = open(CXX).read()
    plan = re.search(r"PLAN = (\[\[.*?\]\])", open(os.path.join(ROOT, "tests", "test_gpu_rx_egress.py")).read()).group(1)
    assert plan.replace("[", "{").replace("]", "}") in src  # (the frame counts are that file's PLAN rows)
    r = subprocess.run([replay], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ KR
def check_kr_is_one_lean_kernel(tmp_path):
    """(tests/test_rx_egress_abi.py holds the kernel that serves round robin against the same list)"""
    res = _compile(tmp_path, KR)
    assert len(res) == 1 and "rx_runs_kernel" in list(res)[0], sorted(res)
    (_, scratch, occ), = res.values()
    assert scratch == 0 and occ == 8, res
    r = subprocess.run([HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(CSRC, KR),
                        "-o", str(tmp_path / "k.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(str(tmp_path / "k.s")).read()
    assert re.search(r"\.group_segment_fixed_size:\s*0\b", text) or re.search(r"\.amdhsa_group_segment_fixed_size 0\b", text)  # no LDS
    code = [ln.split("//")[0].split(";")[0].strip() for ln in text.splitlines()]
    ops = [ln.split()[0] for ln in code if ln and not ln.startswith(".") and not ln.endswith(":")]
    assert ops.count("global_load_dwordx4") >= 8 and ops.count("global_store_dwordx4") >= 8  # (four per lane: runs, records)
    assert {o for o in ops if o.startswith("global_store")} == {"global_store_dwordx4"}
    assert {o for o in ops if o.startswith("global_load")} == {"global_load_dwordx4"}  # (a run comes through the scalar cache)
    assert not [o for o in ops if o.startswith(("flat_", "scratch_", "ds_", "buffer_", "s_barrier"))]
    loads = [ln for ln in code if ln.startswith("global_load_dwordx4")]
    assert len([ln for ln in loads if " nt" in ln]) >= 8, loads  # (every frame and record load; the record places are a table)


def test_kr_compiles_to_one_lean_kernel(tmp_path):
    check_kr_is_one_lean_kernel(tmp_path)


def test_the_kernel_and_its_launch_live_in_the_new_files():
    import glob

    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        if os.path.basename(path) != KR:
            assert "rx_runs" not in open(path).read(), path
    assert KR in open(os.path.join(CSRC, "Makefile")).read()
    calls = {os.path.basename(p): open(p).read().count("launch_rx_runs(") for p in glob.glob(os.path.join(CSRC, "*.cpp"))}
    assert {k: v for k, v in calls.items() if v} == {"sdrhip_rx_egress.cpp": 1}
