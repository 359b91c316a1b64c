"""dec_max_rows = auto on the GPU: the batched CM256 decoder decides per frame, from the frame's own block indices, between the
one-launch decoder (stage A: at most 32 recovery blocks, all of rows 0..31) and the general chain restricted to a device-side list of
the other frames (stage B).  Whatever the batch, auto delivers the bytes of dec_max_rows = 128; every decodable frame gives back the
framer's originals; the counter "dec_deferred" grows by exactly the frames the rule names and "dec_rows_exceeded" does not move."""
import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu

NF = 32  # frames of material: one framer run and one 128-row encode each, shared by every test of the module


@pytest.fixture(scope="module")
def ctx():
    import sdrdaemon_amd as sd

    assert sd.device_count() > 0
    return sd.Context(0)


@pytest.fixture(scope="module")
def material(oracle):
    """(x, frames, allb): noise, the framer's frames, and per frame the 128 originals + recovery rows 0..127 (read-only)"""
    x = signals.noise(NF * 16129, 4711)
    frames = oracle.framer(nb_fec_blocks=127).write(x)
    frames[:, :, 3] = 0
    assert frames.shape[0] == NF
    allb = np.stack([np.concatenate([frames[f], oracle.frame_encode(frames[f], 128)]) for f in range(NF)])
    for a in (x, frames, allb):
        a.setflags(write=False)
    return x, frames, allb


KINDS = ["none", "24_low", "32_low", "1_row0",                                  # served by stage A
         "32_rows1_32", "33", "1_row40", "5_block0_high", "64", "96",            # deferred
         "dup_original", "dup_recovery", "too_few", "shuffled"]                 # deferred and hostile (rows >= 32)


def _order(kind, rs, strict):
    """-> (arrival order of 128 block indices, decodable)"""
    def lose(n, rows, with0=False):
        lost = sorted(rs.choice(np.arange(1, 128), n - (1 if with0 else 0), replace=False).tolist() + ([0] if with0 else []))
        got = [i for i in range(128) if i not in lost]
        rs.shuffle(got)  # originals in any order, recovery blocks last
        return got + [128 + r for r in rows]

    if kind == "none":
        return lose(0, []), True
    if kind == "24_low":
        return lose(24, sorted(rs.choice(32, 24, replace=False).tolist())), True
    if kind == "32_low":
        return lose(32, list(range(32))), True
    if kind == "1_row0":
        return lose(1, [0]), True
    if kind == "32_rows1_32":
        return lose(32, list(range(1, 33))), True
    if kind == "33":
        return lose(33, list(range(33))), True
    if kind == "1_row40":
        return lose(1, [40]), False  # cm256's DecodeM1 XORs whatever the row: wrong bytes, mirrored
    if kind == "5_block0_high":
        return lose(5, sorted(rs.choice(np.arange(32, 64), 5, replace=False).tolist()), with0=True), True
    if kind == "64":
        return lose(64, list(range(64))), True
    if kind == "96":
        return lose(96, sorted(rs.choice(128, 96, replace=False).tolist())), True
    def hostile():  # 12 originals lost, rows 30..63 with row 63 among them
        return lose(12, sorted(rs.choice(np.arange(30, 63), 11, replace=False).tolist()) + [63])

    o = hostile()
    if kind == "dup_original":
        o[3] = o[4]
        return o, False
    if kind == "dup_recovery":
        o[-1] = o[-2]
        return o, False
    if kind == "too_few":
        o[-2:] = o[:2]  # two recovery blocks replaced by repeats of originals: blocks missing for good
        return o, False
    assert kind == "shuffled"
    rs.shuffle(o)  # recovery blocks anywhere in arrival order: strict mode's holes
    return o, not strict


def _rule(idx):
    """the frames the header's rule defers, from the block indices alone: N > 32 or maxrow >= 32"""
    idx = np.asarray(idx).astype(int)
    n = (idx >= 128).sum(axis=-1)
    maxrow = np.where(n > 0, idx.max(axis=-1) - 128, -1)
    return (n > 32) | (maxrow >= 32)


def _batch(material, kinds, seed, strict=0, first=0):
    _, _, allb = material
    rs = np.random.RandomState(seed)
    rx = np.zeros((len(kinds), 128, 512), np.uint8)
    dec = np.zeros(len(kinds), bool)
    for i, k in enumerate(kinds):
        o, dec[i] = _order(k, rs, strict)
        assert len(o) == 128
        rx[i] = allb[first + i][o]
    return rx, dec


def _originals(material, got, f, src):
    x, frames, _ = material
    payload, b0 = got
    assert np.array_equal(payload[f].view(np.int16).reshape(-1, 2), x[src * 16129:(src + 1) * 16129]), (f, src)
    assert np.array_equal(b0[f], frames[src, 0, 4:]), (f, src)


class _Counters:
    def __init__(self, ctx):
        self.ctx, self.d, self.e = ctx, ctx.counter("dec_deferred"), ctx.counter("dec_rows_exceeded")

    def delta(self):
        d, e = self.ctx.counter("dec_deferred"), self.ctx.counter("dec_rows_exceeded")
        r = (d - self.d, e - self.e)
        self.d, self.e = d, e
        return r


def _decode(ctx, mode, rx, indices=None):
    import sdrdaemon_amd as sd

    ctx.set_option("dec_max_rows", mode)
    try:
        return sd.fec_decode_frames(ctx, rx, indices=indices, want_block0=True)
    finally:
        ctx.set_option("dec_max_rows", 128)


def test_the_option_takes_auto_and_still_refuses_nonsense(ctx):
    import sdrdaemon_amd as sd

    ctx.set_option("dec_max_rows", "auto")  # (raises on a library without the mode)
    ctx.set_option("dec_max_rows", 128)
    for bad in ("0", "129", "automatic", ""):
        with pytest.raises(sd.SdrHipError):
            ctx.set_option("dec_max_rows", bad)
    assert ctx.counter("dec_deferred") >= 0


@pytest.mark.parametrize("strict", [0, 1])
def test_auto_equals_128_on_every_kind_of_frame(ctx, material, strict):
    kinds = [k for k in KINDS for _ in range(2)]
    assert len(kinds) <= NF
    rx, decodable = _batch(material, kinds, 900 + strict, strict)
    idx = np.ascontiguousarray(rx[:, :, 2])
    deferred = _rule(idx)
    for i, k in enumerate(kinds):
        assert deferred[i] == (KINDS.index(k) >= 4), (k, "the batch must hold what its kinds say")
    rx_blind = rx.copy()
    rx_blind[:, :, 2] = 0  # (with the `indices` array the headers' byte 2 must not be read)
    ctx.set_option("dec_strict", strict)
    try:
        cnt = _Counters(ctx)
        for name, data, ind in (("headers", rx, None), ("indices", rx_blind, idx)):
            ref = _decode(ctx, 128, data, ind)
            assert cnt.delta() == (0, 0), name
            got = _decode(ctx, "auto", data, ind)
            d, e = cnt.delta()
            print(name, "strict", strict, "deferred", d, "of", len(kinds), "rows exceeded", e)
            for k in (0, 1):
                bad = [(f, kinds[f]) for f in range(len(kinds)) if not np.array_equal(got[k][f], ref[k][f])]
                assert not bad, (name, ("payload", "block0")[k], bad)
            for f in range(len(kinds)):
                if decodable[f]:
                    _originals(material, got, f, f)
            assert d == int(deferred.sum()), name
            assert e == 0, name
    finally:
        ctx.set_option("dec_strict", 0)


@pytest.mark.parametrize("opt,val,back", [("dec_plan", "kernel", "fused"), ("dec_path", "dense", "syndrome")])
def test_auto_reads_as_128_where_the_one_launch_decoder_is_not_in_play(ctx, material, opt, val, back):
    kinds = ["24_low", "33", "5_block0_high", "64", "dup_recovery", "shuffled", "none"]
    rx, decodable = _batch(material, kinds, 77)
    ref = _decode(ctx, 128, rx)
    cnt = _Counters(ctx)
    ctx.set_option(opt, val)
    try:
        got = _decode(ctx, "auto", rx)
    finally:
        ctx.set_option(opt, back)
    assert cnt.delta() == (0, 0)
    for k in (0, 1):
        assert np.array_equal(got[k], ref[k]), ("payload", "block0")[k]
    for f in range(len(kinds)):
        if decodable[f]:
            _originals(material, got, f, f)


SERVED, DEFER = "24_low", ("33", "5_block0_high", "64", "32_rows1_32")  # (33 and 64: the dense kernel's frames; the others: the syndrome kernel's)


def _edge_kinds(n, deferred):
    return [DEFER[i % len(DEFER)] if i in deferred else SERVED for i in range(n)]


@pytest.mark.parametrize("n,deferred", [(1, {0}), (1, set()), (8, {0}), (8, {7}), (8, {1, 4, 6}), (8, set(range(8)))],
                         ids=["one-deferred", "one-served", "first", "last", "odd-count", "all"])
def test_list_edges(ctx, material, n, deferred):
    rx, decodable = _batch(material, _edge_kinds(n, deferred), 31 + n + len(deferred))
    assert decodable.all() and set(np.flatnonzero(_rule(rx[:, :, 2])).tolist()) == deferred
    cnt = _Counters(ctx)
    got = _decode(ctx, "auto", rx)
    assert cnt.delta() == (len(deferred), 0)
    for f in range(n):
        _originals(material, got, f, f)


def test_three_calls_in_a_row_leave_no_stale_list(ctx, material):
    """8 frames all deferred, then 3 frames none deferred, then 2 frames one deferred, on one context: a list or a count left over
    from the first call would send the second call's frames 0..2 (and frames it does not have) through stage B again"""
    import torch

    import sdrdaemon_amd as sd

    calls = [(8, set(range(8)), 0), (3, set(), 8), (2, {1}, 11)]
    batches = [_batch(material, _edge_kinds(n, d), 5 + n, first=first)[0] for n, d, first in calls]
    cnt = _Counters(ctx)
    ctx.set_option("dec_max_rows", "auto")
    try:
        # device memory: the three calls are queued back to back, nothing synchronises in between
        outs = [sd.fec_decode_frames(ctx, torch.from_numpy(rx).cuda(), want_block0=True) for rx in batches]
        ctx.synchronize()
    finally:
        ctx.set_option("dec_max_rows", 128)
    assert cnt.delta() == (8 + 0 + 1, 0)
    for (n, d, first), (p, b0) in zip(calls, outs):
        got = (p.cpu().numpy(), b0.cpu().numpy())
        for f in range(n):
            _originals(material, got, f, first + f)


def _tx_batch(material, kinds2, seed, first):
    """(2, 3, 128, 512): two streams of three frames"""
    return np.stack([_batch(material, kinds2[s], seed + s, first=first + 3 * s)[0] for s in range(2)])


def _tx_run(ctx, mode, form, batches):
    import sdrdaemon_amd as sd

    ctx.set_option("dec_max_rows", mode)
    try:
        if form == "immediate":
            tx = sd.TxPipe(ctx, 2, 2)
            return [tx.process(b).copy() for b in batches]
        if form in ("overlap1", "overlap0"):
            ctx.set_option("tx_overlap", 1 if form == "overlap1" else 0)
            try:
                tx = sd.TxPipe(ctx, 2, 2, pipelined=True)
                outs = [tx.process(b).copy() for b in batches]
                assert outs[0].shape[1] == 0
                return outs[1:] + [tx.flush().copy()]
            finally:
                ctx.set_option("tx_overlap", 1)
        assert form == "async"
        tx = sd.TxPipe(ctx, 2, 2)
        tx.set_async(4)
        for b in batches:
            tx.submit(b)
        return [tx.collect().copy() for _ in batches]
    finally:
        ctx.set_option("dec_max_rows", 128)


@pytest.mark.parametrize("form", ["immediate", "overlap1", "overlap0", "async"])
def test_tx_pipe_samples_under_auto_equal_those_under_128(ctx, material, form):
    """2 streams x 3 frames, interpolation by 4, one deferred frame per stream; three batches, the middle one without a deferred
    frame (in the asynchronous form all three are in flight at once)"""
    with_d = [[SERVED, "33", "none"], ["5_block0_high", SERVED, SERVED]]
    without = [[SERVED, "none", "32_low"], ["1_row0", SERVED, SERVED]]
    batches = [_tx_batch(material, with_d, 40, 0), _tx_batch(material, without, 50, 6), _tx_batch(material, with_d[::-1], 60, 12)]
    ref = _tx_run(ctx, 128, form, batches)
    cnt = _Counters(ctx)
    got = _tx_run(ctx, "auto", form, batches)
    assert cnt.delta() == (4, 0)
    assert len(got) == len(ref) == 3
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape == (2, (3 * 16129) << 2, 2), (i, g.shape, r.shape)
        assert np.array_equal(g, r), (form, i)
