"""Every variant of the wave interpolator in both workgroup forms.  One rule (interp_pick.h: nseg * nstreams >= 4096) puts K5w in
workgroups of four waves, for the plain kernel and for every variant of interp_variant.h alike; the plain and the table kernels
have four-wave tests of their own (test_gpu_interp_wave.py, test_gpu_tx_stream_format.py), here are the others: bank-wide 8-bit
output, per-stream counts (datagram-fed) with int16 output, 8-bit output and a format table, and gathered input.

17 streams x 2 frames with interp_path = wave and interp_span = 128: 2 x 16 129 inputs are 253 one-block segments per stream, 4301 in
the grid, and 253 is no multiple of four, so every stream's last workgroup has an empty wave.  The same at 3 streams (759 segments):
one wave per workgroup.  Bit-exact against the oracle's interpolators (>> 8 for 8-bit output, HackRFSink.cpp:671-672) behind, for
the datagram-fed calls, the reference's own SDRdaemonFECBuffer (test_gpu_tx_datagrams.RefChain)."""
import numpy as np
import pytest
import torch

import sdrdaemon_amd as sd
import test_gpu_iq8 as iq8
import test_gpu_tx_datagrams as tdg

pytestmark = pytest.mark.gpu

NF = 16129  # samples per frame
F = 2
NSEG = (F * NF + 127) // 128
SHAPES = [17, 3]
RATIOS = [2, 6]
reflib = tdg.reflib


def test_the_shapes_straddle_the_rule():
    assert NSEG == 253 and NSEG % 4 and NSEG * 17 >= 4096 > NSEG * 3


@pytest.fixture(scope="module")
def ctx():
    assert sd.device_count() > 0, "GPU tests need a GPU and libsdrhip.so"
    c = sd.Context(0)
    c.set_option("interp_path", "wave")
    c.set_option("interp_span", 128)
    c.set_option("dec_strict", 1)  # (the reference's copy-back holes, as test_gpu_tx_datagrams)
    yield c
    c.set_option("interp_path", "auto")
    c.set_option("interp_span", 0)
    c.set_option("dec_strict", 0)


_cache = {}


def once(key, make):
    """a reference computed once per module and shared (never written to)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frames(oracle):
    """three distinct streams of F received frames and their payload samples; stream s of a bank is stream s % 3 of these"""
    return once("frames", lambda: iq8.tx_batch(oracle, np.random.RandomState(71), 3, F))


def interpolated(oracle, L):
    """the oracle's int16 output of the three streams"""
    return once(("frames", L), lambda: [oracle.interpolators().interpolate(L, y) for y in frames(oracle)[1]])


def dgrams(oracle):
    """One datagram stream (frames A and B with losses, then a datagram of a third frame) cut into a first call and three kinds of a
    second.  The first call is frame A: it releases the buffer's initial slot.  The second is nothing, or B's first datagram (it
    releases A), or all that is left (it releases A and B): 0, 1 and 2 frames"""
    def make():
        d = np.asarray(tdg.stream_dgrams(oracle, np.random.RandomState(72), 2, 32), np.uint8).reshape(-1, 512)
        index = d[:, 0].astype(int) | d[:, 1].astype(int) << 8  # the frame index of the super block header
        a_end = int(np.argmax(index != index[0]))
        return d[:a_end], [d[:0], d[a_end:a_end + 1], d[a_end:]]
    return once("dgrams", make)


def chained(oracle, reflib, L):
    """the reference chain's int16 output of the first call and of the three kinds of second call behind it"""
    def make():
        first, seconds = dgrams(oracle)
        chains = [tdg.RefChain(reflib, oracle) for _ in seconds]
        return [c.feed(first, L) for c in chains][0], [c.feed(d, L) for c, d in zip(chains, seconds)]
    return once(("dgrams", L), make)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("L", RATIOS)
def test_bank_wide_s8(ctx, oracle, L, S):
    rx, exp = frames(oracle)[0], interpolated(oracle, L)
    got = sd.TxPipe(ctx, S, L, output_format="s8").process(torch.from_numpy(np.ascontiguousarray(rx[np.arange(S) % 3])).cuda())
    ctx.synchronize()
    got = host(got)
    assert got.dtype == np.int8 and got.shape == (S, (F * NF) << L, 2)
    for s in range(S):
        assert np.array_equal(got[s], iq8.narrow(exp[s % 3])), (L, s)


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("out", ["s16", "s8", "table"])
@pytest.mark.parametrize("L", RATIOS)
def test_per_stream_counts(ctx, oracle, reflib, L, out, S):
    """streams of 0, 1 and 2 frames in one call (stream s: s % 3), behind a call of one frame each: the grid is the largest stream's,
    every other stream ends inside it"""
    (first, seconds), (exp1, exp2) = dgrams(oracle), chained(oracle, reflib, L)
    assert exp1.shape[0] == NF << L and [e.shape[0] for e in exp2] == [0, NF << L, (2 * NF) << L]
    fmts = [("s8" if s % 2 else "s16") if out == "table" else out for s in range(S)]
    p = sd.TxPipe(ctx, S, L, output_format="s8" if out == "s8" else "s16")
    if out == "table":
        p.set_stream_formats(fmts)

    def same(got, exp, frames, where):
        assert p.last_n_frames == frames, where
        for s in range(S):
            g, e = host(got[s][0]), exp(s)
            assert g.dtype == (np.int8 if fmts[s] == "s8" else np.int16) and g.shape == e.shape, (L, out, where, s, g.dtype, g.shape)
            assert np.array_equal(g, iq8.narrow(e) if fmts[s] == "s8" else e), (L, out, where, s)

    got = p.process_datagrams([torch.from_numpy(first).cuda()] * S)
    ctx.synchronize()
    same(got, lambda s: exp1, [1] * S, "first")
    got = p.process_datagrams([torch.from_numpy(seconds[s % 3]).cuda() for s in range(S)])
    ctx.synchronize()
    same(got, lambda s: exp2[s % 3], [s % 3 for s in range(S)], "second")


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("L", RATIOS)
def test_gathered_input(ctx, oracle, L, S):
    """tx_gather = 1 with dec_max_rows <= 32 (test_gpu_pipes.py's no-copy route): the decoder leaves a position map, K5w reads through it"""
    rx, exp = frames(oracle)[0], interpolated(oracle, L)
    ctx.set_option("dec_max_rows", 32)
    ctx.set_option("tx_gather", 1)
    try:
        got = sd.TxPipe(ctx, S, L).process(torch.from_numpy(np.ascontiguousarray(rx[np.arange(S) % 3])).cuda())
        ctx.synchronize()
    finally:
        ctx.set_option("tx_gather", 0)
        ctx.set_option("dec_max_rows", 128)
    got = host(got)
    assert got.dtype == np.int16 and got.shape == (S, (F * NF) << L, 2)
    for s in range(S):
        assert np.array_equal(got[s], exp[s % 3]), (L, s)
