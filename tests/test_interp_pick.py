"""The interpolator bank's choice of kernel (sdrdaemon_amd/csrc/interp_pick.h: the x1 copy, K6n, K6x, or one variant of K5 / K5w in
workgroups of one or four waves) on a CPU: tests/cxx/interp_pick_test.cpp walks every combination of ratio, path option, gathered
input, count table, bank-wide format, format table and grid size and compares each pick with a transcription of the if-chain and the
twelve launch functions the bank had before -- as a stand-alone program built with the address and undefined-behaviour sanitizers.
No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "interp_pick_test.cpp")


def test_header_stands_alone():
    """interp_pick.h is C++11 and pulls in neither HIP nor a library header: one standard header and nothing else"""
    with open(os.path.join(CSRC, "interp_pick.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert incs == ["<cstddef>"]
    with open(SRC) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"interp_pick.h"']


def test_every_combination_picks_what_the_chain_launched(tmp_path):
    exe = str(tmp_path / "interp_pick_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
