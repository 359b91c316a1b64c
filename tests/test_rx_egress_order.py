"""The departure order of an egress batch of equal frames (the equal-frames form of sdrdaemon_amd/csrc/rx_depart_order.h) on a CPU:
tests/cxx/rx_egress_order_test.cpp checks the closed form, the tags and KR's run table -- one run per delivered frame -- against a
literal simulation of the rounds, as a stand-alone program built with the address and undefined-behaviour sanitizers.  No GPU, no
library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "rx_egress_order_test.cpp")


def test_header_stands_alone():
    """rx_depart_order.h is C++11 and pulls in neither HIP nor a library header: standard headers, and the shared constants of
    rx_egress_limits.h, which includes two standard headers and nothing else."""
    with open(os.path.join(CSRC, "rx_depart_order.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(incs) == ['"rx_egress_limits.h"', "<algorithm>", "<cstddef>", "<cstdint>", "<vector>"]
    with open(os.path.join(CSRC, "rx_egress_limits.h")) as f:
        assert sorted(ln.split()[1] for ln in f if ln.startswith("#include")) == ["<cstddef>", "<cstdint>"]
    with open(SRC) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"rx_depart_order.h"']


def test_order_matches_a_simulation_of_the_rounds(tmp_path):
    exe = str(tmp_path / "rx_egress_order_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
