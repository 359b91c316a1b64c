"""The paced departure order of an egress batch (sdrdaemon_amd/csrc/rx_paced_order.h) on a CPU: tests/cxx/rx_paced_order_test.cpp
checks the closed form, the tags and KP's table against a literal sort by the exact keys, the equal-count case against the
round-robin order, the gap guarantee and every refusal, as a stand-alone program built with the address and undefined-behaviour
sanitizers.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "rx_paced_order_test.cpp")


def test_header_stands_alone():
    """rx_paced_order.h is C++11 and pulls in neither HIP nor a library header: standard headers and nothing else; it states the
    gap guarantee and never reaches for floating point"""
    with open(os.path.join(CSRC, "rx_paced_order.h")) as f:
        text = f.read()
    incs = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(incs) == ['"rx_egress_limits.h"', "<algorithm>", "<cstddef>", "<cstdint>", "<vector>"]  # (constants alone)
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "double" not in code and "float" not in code
    assert "floor(D_t / D_s) or ceil(D_t / D_s)" in text and "round-robin array" in text
    with open(SRC) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"rx_depart_order.h"', '"rx_paced_order.h"']


def test_order_matches_a_literal_sort(tmp_path):
    exe = str(tmp_path / "rx_paced_order_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
