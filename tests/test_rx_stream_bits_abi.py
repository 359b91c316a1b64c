"""CPU-side checks of the per-stream sample size (sdrhip_rx_set_stream_bits / sdrhip_rx_get_stream_bits / sdrhip_decimate_ragged_bits):
declared in include/sdrhip.h with their citations, exported, bound in Python, refused loudly without a GPU; and the property of the
reference decimators the design rests on -- the sample size enters a cascade only through the shift in front of the int16
truncation, never the filter histories -- on the oracle and, where built, on the compiled reference."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from oracle_lib import Reference
from test_iq8_abi import _header, built  # noqa: F401

NAMES = ["sdrhip_rx_set_stream_bits", "sdrhip_rx_get_stream_bits", "sdrhip_decimate_ragged_bits"]


def test_declared_exported_and_bound(built):
    src = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    lib = built.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in built.EXPORTS, n
    assert "int sdrhip_rx_set_stream_bits(sdrhip_rx *rx, const unsigned *sample_bits);" in src
    assert "int sdrhip_rx_get_stream_bits(const sdrhip_rx *rx, int stream, unsigned *sample_bits, unsigned *frame_bits);" in src
    assert ("int sdrhip_decimate_ragged_bits(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in, "
            "const size_t *n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);") in src
    sz, vp, i, up = C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_uint)
    assert lib.sdrhip_rx_set_stream_bits.argtypes == [vp, up]
    assert lib.sdrhip_rx_get_stream_bits.argtypes == [vp, i, up, up]
    assert lib.sdrhip_decimate_ragged_bits.argtypes == [vp, i, i, up, vp, C.POINTER(sz), sz, vp, sz, C.POINTER(sz), i]
    assert lib.sdrhip_decimate_ragged_bits.argtypes == lib.sdrhip_decimate_ragged.argtypes


def test_header_cites_the_reference_and_states_the_rules():
    h = _header()
    at = h.index("int sdrhip_rx_set_stream_bits")
    comment = re.sub(r"\s+", " ", h[h.rindex("/*", 0, at):at])
    for cite in ("sdrdaemonrx.cpp:619-620, 639-640", "sdrdaemonrx.cpp:622-623, 642-643", "RtlSdrSource.cpp:549", "HackRFSource.cpp:669",
                 "Decimators.cpp:27-32, 43-44, 52-53, 62", "UDPSinkFEC.cpp:160-165"):
        assert cite in comment, cite
    for word in ("1..16", "NULL = bank-wide again", "byte for byte", "sdrhip_rx_reconfigure", "sdrhip_rx_reset_streams", "frame_bits",
                 "sdrhip_rx_set_pipelined(1)", "nothing is enqueued", "sdrhip_rx_collect_egress", "Not covered",
                 "sdrhip_rx_set_input_format", "the Tx pipe"):
        assert word in comment, word
    at = h.index("int sdrhip_decimate_ragged_bits")
    comment = re.sub(r"\s+", " ", h[h.rindex("/*", 0, at):at])
    for cite in ("sdrdaemonrx.cpp:619-620", "Decimators.cpp:27-32"):
        assert cite in comment, cite


def test_python_surface(built):
    import sdrdaemon_amd as sd

    p = inspect.signature(sd.RxPipe.set_stream_bits).parameters
    assert list(p) == ["self", "bits"] and p["bits"].default is None
    assert list(inspect.signature(sd.RxPipe.stream_bits).parameters) == ["self", "stream"]
    src = inspect.getsource(sd.Decimators.decimate_ragged)
    assert "sdrhip_decimate_ragged_bits" in src and "sdrhip_decimate_ragged," in src  # (a sequence: the new entry; a scalar: today's)


def test_null_handle_and_no_gpu(built):
    import sdrdaemon_amd as sd

    lib = built.lib()
    b, fb = C.c_uint(0), C.c_uint(0)
    bits = (C.c_uint * 2)(8, 12)
    n = (C.c_size_t * 2)(0, 0)
    assert lib.sdrhip_rx_set_stream_bits(None, bits) == -1
    assert lib.sdrhip_rx_set_stream_bits(None, None) == -1
    assert lib.sdrhip_rx_get_stream_bits(None, 0, C.byref(b), C.byref(fb)) == -1
    assert lib.sdrhip_decimate_ragged_bits(None, 1, 2, bits, None, n, 0, None, 0, n, 0) == -1
    assert b"NULL" in lib.sdrhip_last_error()
    assert list(bits) == [8, 12]
    if sd.device_count() > 0:
        return
    with pytest.raises(sd.SdrHipError):  # (no GPU: no context, no pipe -- never a quiet host path)
        sd.RxPipe(sd.Context(0), 2).set_stream_bits([8, 12])
    with pytest.raises(sd.SdrHipError):
        sd.Decimators(sd.Context(0), 2).decimate_ragged(1, 2, [8, 12], np.zeros((2, 8, 2), np.int16), [8, 8])


# ------------------------------------------------------------------------------------------------ the property of the decimators
def _yardsticks(oracle):
    made = [("oracle", oracle.decimators)]
    if Reference.available("eo1"):
        ref = Reference("eo1")
        made.append(("reference", ref.decimators))
    return made


CASES = [(L, fc) for L in range(1, 7) for fc in (0, 1, 2)]


@pytest.mark.parametrize("L,fc", CASES)
def test_the_sample_size_enters_only_the_output_shift(oracle, L, fc):
    """one Decimators object fed calls whose sampleSize alternates gives, per call, the samples (and the returned size) of separate
    objects -- one per size -- fed the same input history and asked at that call's size: no size leaves a trace in the histories"""
    sizes = [8, 16, 12, max(16 - L - 1, 1), 16 - L, min(16 - L + 1, 16), 8, 16]
    rs = np.random.RandomState(100 * L + fc)
    blocks = [rs.randint(-32768, 32768, size=((37 + 11 * k) << L, 2)).astype(np.int16) for k in range(len(sizes))]
    for name, make in _yardsticks(oracle):
        mixed = make()
        apart = {b: make() for b in sorted(set(sizes))}
        for k, (b, x) in enumerate(zip(sizes, blocks)):
            y, ss = mixed.decimate(L, fc, b, x)
            for b2, d in apart.items():  # (every object sees every block: the same input history; only the asked size differs)
                y2, ss2 = d.decimate(L, fc, b2, x)
                if b2 == b:
                    assert ss == ss2 and np.array_equal(y, y2), (name, L, fc, k, b)


@pytest.mark.parametrize("L,fc", CASES)
def test_two_sizes_below_the_target_differ_by_the_left_shift(oracle, L, fc):
    """for two sizes a < b below 16 - L (no truncation shift: trunk = 0, norm = 16 - L - size) the outputs are the same 32-bit values
    shifted left by b - a more for the smaller size: out_a = out_b << (b - a) mod 2^16"""
    pairs = [(a, b) for a, b in ((1, 16 - L - 1), (8, 16 - L - 1), (4, 8), (8, 9)) if a < b < 16 - L]
    assert pairs
    rs = np.random.RandomState(200 * L + fc)
    x = rs.randint(-32768, 32768, size=(300 << L, 2)).astype(np.int16)
    for name, make in _yardsticks(oracle):
        for a, b in pairs:
            ya, sa = make().decimate(L, fc, a, x)
            yb, sb = make().decimate(L, fc, b, x)
            assert (sa, sb) == (a + L, b + L), (name, L, fc, a, b, sa, sb)
            exp = ((yb.astype(np.int64) & 0xffff) << (b - a)) & 0xffff
            assert np.array_equal(ya.astype(np.int64) & 0xffff, exp), (name, L, fc, a, b)
