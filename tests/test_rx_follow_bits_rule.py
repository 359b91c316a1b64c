"""The rule of sdrhip_rx_set_follow_bits on a CPU: tests/cxx/rx_follow_bits_rule_test.cpp runs the arithmetic KFb runs
(sdrdaemon_amd/csrc/rx_stream_settings.h: one text for host and device) for every log2decim 0..6 and every value 0..255 of the
incoming sampleBits byte, as a stand-alone program built with the address and undefined-behaviour sanitizers; what it prints is
held here against the decimators themselves (the C restatement, and the compiled reference where it is built) and against a
record formed with struct and zlib.  No GPU, no library."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from oracle_lib import Reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cxx", "rx_follow_bits_rule_test.cpp")
CASE = re.compile(r"CASE L (\d+) byte (\d+) admitted 1 norm (\d+) trunk (\d+) bits (\d+) w2 ([0-9a-f]{8}) fc (\d+) rate (\d+) crc ([0-9a-f]{8})")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rx_follow_bits_rule") / "rx_follow_bits_rule_test")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def cases(output):
    return [tuple(int(x, 16) if i in (5, 8) else int(x) for i, x in enumerate(m)) for m in CASE.findall(output)]


def test_program_includes_the_settings_header_alone():
    with open(SRC) as f:
        assert [ln.split()[1] for ln in f if ln.startswith('#include "')] == ['"rx_stream_settings.h"']


def test_admitted_iff_1_to_16(output, cases):
    """every (log2decim, byte) was run; a byte is an incoming size iff it is 1..16 (the program also checks that nothing is formed
    otherwise, that only byte 1 of the incoming word is read and that bytes 2 and 3 of the row's word stay)"""
    seen = {(int(L), int(b)): int(a) for L, b, a in re.findall(r"CASE L (\d+) byte (\d+) admitted (\d)", output)}
    assert sorted(seen) == [(L, b) for L in range(7) for b in range(256)]
    for (L, b), a in seen.items():
        assert a == (1 if 1 <= b <= 16 else 0), (L, b)
    assert len(cases) == 7 * 16
    for what, n in (("admitted", 112), ("refused", 7 * 240), ("crcs held against rx_meta_record", 224)):
        assert re.search(r"%s: %d\n" % (what, n), output), what


def test_third_word_and_crc_are_the_reference_record(cases):
    """bytes 8 and 9 = (b' - 1) / 8 + 1 and b', bytes 10 and 11 kept (128 and a fecblk), and the CRC that of MetaDataFEC with a zero
    stamp (UDPSinkFEC.cpp:87-132; boost::crc_32_type = zlib.crc32 over the first 20 bytes)"""
    for L, b, norm, trunk, ssd, w2, fc, rate, crc in cases:
        assert ssd == (b if L == 0 else min(b + L, 16)), (L, b)
        sb, bits, nbo, fec = struct.unpack("<BBBB", struct.pack("<I", w2))
        assert (sb, bits, nbo) == ((ssd - 1) // 8 + 1, ssd, 128) and fec in (32, 0, 128, 7), (L, b)
        assert crc == zlib.crc32(struct.pack("<III8x", fc, rate, w2)), (L, b)


def _yardsticks(oracle):
    made = [("oracle", oracle.decimators)]
    if Reference.available("eo1"):
        made.append(("reference", Reference("eo1").decimators))
    return made


def test_pair_and_size_are_the_decimators_own(oracle, cases):
    """for every admitted (log2decim, b): the decimators return b' for sampleSize b, and their samples are `acc << norm >> trunk`
    truncated to int16 with the pair the rule gives -- acc read from a decimator asked at the size with norm = trunk = 0 (16 -
    log2decim), on an input small enough for acc to fit int16 (|x| <= 16: at most 16 * 2^6 * the half-bands' overshoot)."""
    for name, make in _yardsticks(oracle):
        for fcpos in (0, 2):
            acc = {}
            for L in range(7):
                x = np.random.RandomState(7 * L + fcpos).randint(-16, 17, size=(96 << L, 2)).astype(np.int16)
                y, ss = make().decimate(L, fcpos, 16 - L, x)
                assert ss == 16 and np.abs(y.astype(np.int32)).max() < 16384, (name, L)
                acc[L] = (x, y.astype(np.int64))
            for L, b, norm, trunk, ssd, *_ in cases:
                x, a = acc[L]
                y, ss = make().decimate(L, fcpos, b, x)
                assert ss == ssd, (name, fcpos, L, b, ss, ssd)
                want = (((a << norm) >> trunk) & 0xffff).astype(np.uint16).view(np.int16)
                assert np.array_equal(y, want), (name, fcpos, L, b, norm, trunk)
