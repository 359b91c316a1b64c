"""What owns device memory, pinned memory, events and the context reference in the host layer (sdrdaemon_amd/csrc/dev_buffers.h) on a
CPU: tests/cxx/dev_buffers_test.cpp defines the HIP functions the header calls itself, over malloc and with a ledger of what is
live, and checks seeded scripts of reserve / grow / move / swap / release / scope exit, every allocation refused in turn, that a
pinned block never goes before its upload was waited for, the table rotation against the one it replaces and a ring of batches --
as a stand-alone program built with the address and undefined-behaviour sanitizers.  No GPU, no HIP library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "dev_buffers_test.cpp")


def test_header_stands_alone():
    """dev_buffers.h is C++11 and pulls in standard headers, the HIP runtime API and the public header (the error codes): nothing
    else of the library, which it uses by declaration only"""
    with open(os.path.join(CSRC, "dev_buffers.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert sorted(incs) == ['"../../include/sdrhip.h"', "<cstddef>", "<cstring>", "<hip/hip_runtime_api.h>", "<mutex>", "<utility>", "<vector>"]
    with open(SRC) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"dev_buffers.h"']


def test_owners_release_once_and_wait_first(tmp_path):
    exe = str(tmp_path / "dev_buffers_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
