"""The Rx step planner (sdrdaemon_amd/csrc/rx_step_plan.h) on a CPU: tests/cxx/rx_step_plan_test.cpp runs the planner and a
transcription of the decisions it replaced in sdrhip_rx_process and rx_ragged over the cross product of their inputs, as a
stand-alone program built with the address and undefined-behaviour sanitizers.  No GPU, no library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "rx_step_plan_test.cpp")


def test_header_stands_alone():
    """rx_step_plan.h is C++11 and pulls in neither HIP nor a handle type: two standard headers and decim_plan.h, itself host-only."""
    with open(os.path.join(CSRC, "rx_step_plan.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(incs) == ['"decim_plan.h"', "<cstddef>", "<cstdint>"]
    with open(os.path.join(CSRC, "decim_plan.h")) as f:
        assert sorted(ln.split()[1] for ln in f if ln.startswith("#include")) == ["<cstddef>", "<cstdint>"]
    with open(SRC) as f:  # (and the program that compiles it as C++11 below includes nothing of the library beside it)
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"rx_step_plan.h"']


def test_planner_matches_the_code_it_replaced(tmp_path):
    exe = str(tmp_path / "rx_step_plan_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    assert int(re.search(r"uniform cases: (\d+)", r.stdout).group(1)) > 2000000


def test_the_step_reads_the_arrangement_options_in_one_place():
    """sdrhip_rx.cpp reads rx_fused and rx_direct only where it fills the planner's inputs, asks the decimator's planner once per
    step, and leaves the encoder's form to the planner's groups; rx_ragged takes at most 8 parameters"""
    host = open(os.path.join(CSRC, "sdrhip_rx.cpp")).read()
    fill = host[host.index("static RxStepIn rx_step_inputs(const sdrhip_rx *rx)\n{"):host.index("// the encode that a pipelined call left")]
    rest = host.replace(fill, "")
    for word in ("rx_fused", "opt.rx_direct", "rx_encode_form("):
        assert word not in rest, word
    assert host.count("decimate_mfma_applies(") == 1
    sig = re.search(r"int sdrhip::rx_ragged\(([^)]*)\)", host).group(1)
    assert len(sig.split(",")) <= 8
