"""The decimator planners and the path rule (sdrdaemon_amd/csrc/decim_plan.h) on a CPU: tests/cxx/decim_plan_test.cpp runs the
three planners, K1r's per-call geometry and the path rule against a transcription of the code they replaced, and every accepted
plan against what the kernels rely on without checking (coverage, the register ring's read-ahead, the 32-bit lane offsets, the
dealing of the pieces over the workgroups), as a stand-alone program built with the address and undefined-behaviour sanitizers.
No GPU, no library."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "decim_plan_test.cpp")


def _includes(path):
    with open(path) as f:
        return [ln.split()[1] for ln in f if ln.startswith("#include")]


def test_header_stands_alone():
    """decim_plan.h is C++11 and includes standard headers only: neither HIP nor the kernels' argument structs; the program that
    compiles it as C++11 below includes nothing of the library beside it"""
    incs = _includes(os.path.join(CSRC, "decim_plan.h"))
    assert incs and all(i.startswith("<") for i in incs), incs
    assert set(incs) <= {"<cstddef>", "<cstdint>"}, incs
    assert [i for i in _includes(SRC) if i.startswith('"')] == ['"decim_plan.h"']


def test_planners_live_in_the_header_alone():
    """the kernel units keep kernels and launch_* functions, sdrhip_internal.h no planner's declaration; the shared constants are
    the header's names there, not literal copies"""
    for f in ("decim_kernels.hip", "decim_mfma.hip", "rx_ragged_kernels.hip", "sdrhip_internal.h"):
        text = open(os.path.join(CSRC, f)).read()
        assert not re.search(r"\bplan_decimate\w*\s*\(int ", text), f
    assert re.search(r"constexpr int P0 = DECIM_PASS;", open(os.path.join(CSRC, "decim_body.h")).read())
    mfma = open(os.path.join(CSRC, "decim_mfma.hip")).read()
    assert "constexpr bool mf_dma_applies" not in mfma and "mf_dma_applies(" in mfma
    assert "static_assert((size_t)D * 32 <= MF_READ_AHEAD" in mfma and "MF_TAIL_SEG % P0 == 0" in mfma


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decim_plan") / "decim_plan_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_plans_match_the_code_they_replaced_and_hold_the_kernels_bounds(output):
    """every case agreed with the transcription and held the invariants, and the sweep reached the cases it is there for (the
    program refuses to say OK otherwise)"""
    for what in ("uniform plans accepted", "uniform plans refused", "wave groups given to the tail for the read-ahead", "plans of one wave group",
                 "sizes on the planner's own span", "spans refused at the lane-offset limit", "plans with early piece workgroups", "dealings simulated",
                 "dealings in closed form", "path rule admitted", "path rule refused by size", "path rule refused by the planner", "ragged plans accepted",
                 "ragged plans refused", "streams at count 0", "streams shorter than the head", "streams of one wave group",
                 "streams with a wave group given to the tail", "equal-count scripts on the uniform geometry", "K1r grids", "calls without a K1r grid"):
        n = re.search(r"%s: (\d+)" % re.escape(what), output)
        assert n and int(n.group(1)) > 0, what
