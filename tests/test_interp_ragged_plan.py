"""The table of the sample-fed ragged interpolator launch (sdrdaemon_amd/csrc/interp_ragged_plan.h: one segment length per launch,
each stream's own segments, one entry per (stream, segment)) on a CPU: tests/cxx/interp_ragged_plan_test.cpp sweeps banks of 1..9
streams over counts around every block and macro-cycle edge, every ratio, both routes and the span overrides -- as a stand-alone
program built with the address and undefined-behaviour sanitizers.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "interp_ragged_plan_test.cpp")


def test_header_stands_alone(tmp_path):
    """interp_ragged_plan.h is C++11 on standard headers and interp_pick.h alone, and compiles on its own"""
    with open(os.path.join(CSRC, "interp_ragged_plan.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert incs == ["<cstddef>", "<cstdint>", '"interp_pick.h"']
    with open(SRC) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"interp_ragged_plan.h"']
    one = tmp_path / "alone.cpp"
    one.write_text('#include "interp_ragged_plan.h"\nint main() { return sizeof(sdrhip::InterpMapRow) == 24 ? 0 : 1; }\n')
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(one), "-o", str(tmp_path / "alone")], check=True)
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0


def test_every_bank_gets_every_segment_once(tmp_path):
    exe = str(tmp_path / "interp_ragged_plan_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
