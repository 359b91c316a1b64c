"""The Rx bank's per-stream settings and the counts of a ragged step (sdrdaemon_amd/csrc/rx_stream_settings.h) on a CPU:
tests/cxx/rx_stream_settings_test.cpp replays seeded scripts of setter calls, bank-value changes, ragged steps and datagram joins
through the type and through a transcription of the code it replaced, as a stand-alone program built with the address and
undefined-behaviour sanitizers; the records it prints are formed here a third way.  No GPU, no library."""
import os
import re
import struct
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "rx_stream_settings_test.cpp")


def test_header_stands_alone():
    """rx_stream_settings.h is C++11 and pulls in neither HIP nor a library header: standard headers, and the frame area beside it
    (which test_rx_frame_area.py holds to the same rule) for the counts of a ragged step."""
    with open(os.path.join(CSRC, "rx_stream_settings.h")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert [i for i in incs if not i.startswith("<")] == ['"rx_frame_area.h"']
    std = {"<algorithm>", "<cstddef>", "<cstdint>", "<cstring>", "<functional>", "<new>", "<tuple>", "<utility>", "<vector>"}
    assert set(i for i in incs if i.startswith("<")) <= std, incs
    with open(SRC) as f:  # (and the program that compiles it as C++11 below includes nothing of the library beside it)
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"rx_stream_settings.h"']


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rx_stream_settings") / "rx_stream_settings_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_settings_and_counts_match_the_code_they_replaced(output):
    """every script agreed, and reached the cases it is there for (the program refuses to say OK otherwise)"""
    for what in ("streams at count 0", "completing no frame", "several frames", "windows inside an open frame", "joins of unit 4", "setters refused",
                 "records formed", "kept", "steps with differing fecblk", "with equal fecblk"):
        n = re.search(r"%s: (\d+)" % what, output)
        assert n and int(n.group(1)) > 0, what


def test_printed_records_are_the_reference_records(output):
    """MetaDataFEC with a zero stamp (UDPSinkFEC.cpp:87-132), formed with struct and zlib: centre frequency and sample rate, the
    sampleBytes / sampleBits the decimated size gives (sdrdaemonrx.cpp:639-643; a decimateN adds log2decim bits up to 16), 128,
    nbFECBlocks, eight zero bytes, and boost::crc_32_type = zlib.crc32 over the first 20 bytes"""
    recs = re.findall(r"RECORD log2decim (\d+) fc (\d+) rate (\d+) nb_fec (\d+) bits (\d+) : ([0-9a-f]{48})", output)
    assert len(recs) == 16 and {r[0] for r in recs} == {"0", "2", "4", "6"}
    for L, fc, rate, fec, bits, hexed in recs:
        L, fc, rate, fec, bits = int(L), int(fc), int(rate), int(fec), int(bits)
        got = bytes.fromhex(hexed)
        ssd = bits if L == 0 else min(bits + L, 16)
        head = struct.pack("<IIBBBB8x", fc, rate, (ssd - 1) // 8 + 1, ssd, 128, fec)
        assert got[8:12] == head[8:12], (L, bits, fec, got[8:12])
        assert got[:20] == head
        assert struct.unpack("<I", got[20:])[0] == zlib.crc32(got[:20]) == zlib.crc32(head), (L, fc, rate, fec, bits)
