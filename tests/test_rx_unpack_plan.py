"""K0x's table (sdrdaemon_amd/csrc/rx_unpack_plan.h: the rows and segments of a batch whose streams differ in input format) on a
CPU: tests/cxx/rx_unpack_plan_test.cpp checks it against a literal walk of the packed bytes -- every row sample at the byte the walk
gives, segments tiling each row, workgroup prefixes covering each row once, the upload's size, the 32-bit limits -- as a stand-alone
program built with the address and undefined-behaviour sanitizers.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "rx_unpack_plan_test.cpp")


def test_header_stands_alone():
    """rx_unpack_plan.h is C++11 and pulls in neither HIP nor a library header: two standard headers and nothing else"""
    with open(os.path.join(CSRC, "rx_unpack_plan.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(incs) == ["<cstddef>", "<cstdint>"]
    with open(SRC) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"rx_unpack_plan.h"']


def test_table_matches_a_walk_of_the_packed_bytes(tmp_path):
    exe = str(tmp_path / "rx_unpack_plan_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
