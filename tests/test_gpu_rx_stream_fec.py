"""Per-stream fecblk (sdrhip_rx_set_stream_fec / sdrhip_rx_get_stream_fec / sdrhip_rx_egress_stream_blocks).  The yardstick is always
S one-stream twins, sd.RxPipe(ctx, 1, nb_fec=nb_fec[s], ...), fed stream s's input with its stamps (and, first, the compiled
reference decimators with the oracle framer and frame_encode); every comparison is byte equality.  The departure order of the
twins' frames is the literal simulation of the rounds of tests/test_gpu_rx_egress.py."""
import struct
import zlib

import numpy as np
import pytest

import test_gpu_rx_follow_meta as tf
from test_gpu_rx_egress import PLAN, ctx, dgram_calls, merge, mismatches, ragged_blocks, rounds, stamps, torch_first  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F = 16129
EBUSY, EINVAL = -6, -1
HUB = [0, 1, 32, 127, 4]  # the egress cases' counts: B = 128, 129, 160, 255, 132


class Twins:
    """S one-stream pipes, stream s with its own nb_fec: the expected result of the bank"""

    def __init__(self, ctx, fec, **cfg):
        import sdrdaemon_amd as sd

        self.p = [sd.RxPipe(ctx, 1, nb_fec=r, **cfg) for r in fec]

    def ragged(self, x, counts, secs, usecs):
        return [p.process(np.ascontiguousarray(x[s][:counts[s]]), int(secs[s]), int(usecs[s])) for s, p in enumerate(self.p)]

    def datagrams(self, chunk, secs, usecs):
        return [p.process_datagrams([chunk[s]], int(secs[s]), int(usecs[s]))[0] for s, p in enumerate(self.p)]

    def reconfigure(self, fec):
        for p, r in zip(self.p, fec):
            p.reconfigure(nb_fec=r)


def same(got, exp, fec, where):
    """a bank's per-stream frames against the twins': shapes (n, 128 + nb_fec[s], 512) and bytes"""
    assert len(got) == len(exp) == len(fec), where
    for s, (g, e) in enumerate(zip(got, exp)):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape == (e.shape[0], 128 + fec[s], 512), (where, s, g.shape, e.shape)
        assert g.tobytes() == e.tobytes(), (where, s)


def rows_of(xs, counts):
    rows = np.zeros((len(xs), max(max(counts), 1), 2), np.int16)
    for s, x in enumerate(xs):
        rows[s, :counts[s]] = x
    return rows


def code(fn, *args, **kw):
    import sdrdaemon_amd as sd

    with pytest.raises(sd.SdrHipError) as e:
        fn(*args, **kw)
    return e.value.code


# ------------------------------------------------------------------------------------------------ 1. reference chain
@pytest.mark.parametrize("L", [0, 1])
@pytest.mark.parametrize("fec", [[0, 1, 12, 32, 127], [13, 33, 128, 8, 8]], ids=["forms", "form_edges"])
def test_reference_chain_ragged_entry(ctx, oracle, fec, L):
    """per stream: the compiled reference decimators, the oracle framer with nb_fec_blocks = nb_fec[s], frame_encode.  [0, 1, 12, 32,
    127]: group maximum 12 = the generic kernel, 32 = the FFT form, 127 = the walk; [13, 33, 128, 8, 8]: the form edges and a slot of
    256 blocks.  The nbFECBlocks byte and the CRC explicitly; every stream completes at least 2 frames per call over 3 calls"""
    import sdrdaemon_amd as sd
    from oracle_lib import Reference

    S = len(fec)
    bank = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, sample_bits=16, nb_fec=8, center_frequency_khz=435000, sample_rate=625000)
    bank.set_stream_fec(fec)
    for s in range(S):
        assert bank.stream_fec(s) == (fec[s], 128 + max(fec))
    decs = [Reference("eo1").decimators() if Reference.available("eo1") else oracle.decimators() for _ in range(S)]
    framers = [None] * S
    rs = np.random.RandomState(10 * L + fec[0])
    for k in range(3):
        counts = [((2 * F + 11 * s + 5 * k + 1) << L) + (s % 2) * L for s in range(S)]
        x = rs.randint(-32768, 32768, size=(S, max(counts), 2)).astype(np.int16)
        secs, usecs = [1000 + 10 * k + s for s in range(S)], [37 * k + s for s in range(S)]
        got, nf = bank.process_ragged(x, counts, secs, usecs)
        assert len(got) == S and min(nf) >= 2, (k, list(nf))
        for s in range(S):
            y, ss = decs[s].decimate(L, sd.FC_CEN, 16, np.ascontiguousarray(x[s, :counts[s]]))
            if framers[s] is None:
                framers[s] = oracle.framer(nb_fec_blocks=fec[s], sample_bytes=(ss - 1) // 8 + 1, sample_bits=ss)
            framers[s].s.tv_sec, framers[s].s.tv_usec = secs[s], usecs[s]
            exp = framers[s].write(y)
            assert got[s].shape == (exp.shape[0], 128 + fec[s], 512) and nf[s] == exp.shape[0], (k, s, got[s].shape)
            for f in range(exp.shape[0]):
                fr = np.asarray(got[s][f])
                meta = fr[0, 4:28].tobytes()
                assert meta[11] == fec[s] and meta[10] == 128, (k, s, f)
                assert struct.unpack("<I", meta[20:24])[0] == zlib.crc32(meta[:20]) == oracle.crc32(meta[:20]), (k, s, f)
                assert np.array_equal(fr[:128], exp[f]), (k, s, f)
                if fec[s]:
                    assert np.array_equal(fr[128:], oracle.frame_encode(exp[f], fec[s])), (k, s, f)


# ------------------------------------------------------------------------------------------------ 2. twins, synchronous entries
def test_twins_process_ragged_wrap_reset_and_an_idle_stream(ctx):
    """unequal counts; rx_window = 1, so the windows pass the area's end every few calls; stream 1 is fed nothing in call 2; stream
    3 is reset between calls 3 and 4 (the array stays); the zero-copy view shows each stream's own blocks at the slot pitch"""
    import sdrdaemon_amd as sd

    fec, L = [0, 1, 32, 127, 4], 1
    S = len(fec)
    plan = [[2, 1, 3, 1, 2], [1, 2, 0, 2, 1], [3, 0, 1, 1, 2], [1, 1, 2, 3, 0], [2, 2, 1, 0, 3], [1, 3, 2, 2, 1], [2, 1, 1, 2, 2]]
    ctx.set_option("rx_window", 1)
    try:
        cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
        bank, twins = sd.RxPipe(ctx, S, nb_fec=16, **cfg), Twins(ctx, fec, **cfg)
        bank.set_stream_fec(fec)
        rs = np.random.RandomState(2)
        for k, frames in enumerate(plan):
            xs, counts = ragged_blocks(rs, S, L, frames, k == 0)
            if k == 2:
                counts[1], xs[1] = 0, xs[1][:0]
            if k == 4:
                bank.reset_streams([3])
                twins.p[3].reset_streams()
                assert bank.stream_fec(3) == (127, 255)
            secs, usecs = stamps(k, S)
            got, nf = bank.process_ragged(rows_of(xs, counts), counts, secs, usecs)
            exp = twins.ragged(xs, counts, secs, usecs)
            same(got, exp, fec, ("ragged", k))
            assert list(nf) == [e.shape[0] for e in exp]
            if k == 1:
                view = bank.frames_view_ragged()
                same([v.cpu().numpy() for v in view], exp, fec, "view")
        assert min(sum(p[s] for p in plan) for s in range(S)) > 4  # (every stream delivered more frames than a window of 3 + 1 slots)
    finally:
        ctx.set_option("rx_window", 0)


def test_twins_on_the_matrix_cores_direct_stores(ctx):
    """decimate4_cen forced onto the matrix-core launch, which stores straight into the windows with the shared record: the meta
    blocks are written again with each stream's own nbFECBlocks byte and CRC"""
    import sdrdaemon_amd as sd

    fec, L = [4, 32, 0, 33], 2
    S = len(fec)
    ctx.set_option("decim_path", "mfma")
    try:
        cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
        bank, twins = sd.RxPipe(ctx, S, nb_fec=16, **cfg), Twins(ctx, fec, **cfg)
        bank.set_stream_fec(fec)
        rs = np.random.RandomState(12)
        for k, frames in enumerate([[2, 1, 2, 1], [1, 2, 1, 2]]):
            xs, counts = ragged_blocks(rs, S, L, frames, k == 0)
            secs, usecs = stamps(k, S)
            got, _ = bank.process_ragged(rows_of(xs, counts), counts, secs, usecs)
            same(got, twins.ragged(xs, counts, secs, usecs), fec, ("mfma", k))
        assert bank.last_plan()["path"] == "mfma"
    finally:
        ctx.set_option("decim_path", "auto")


def test_twins_process_datagrams(oracle, ctx):
    """the datagram entry, follow meta off: PLAN's batches (a stream fed nothing in some calls, 0 .. 3 frames released); frames,
    records, carry and collector statistics equal the twins' after every call"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S = len(calls[0])
    for L in (0, 1):
        cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
        bank, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, HUB, **cfg)
        bank.set_stream_fec(HUB)
        for i, chunk in enumerate(calls):
            secs, usecs = stamps(i, S)
            got = bank.process_datagrams(chunk, secs, usecs)
            exp = twins.datagrams(chunk, secs, usecs)
            same([g for g, _ in got], [e for e, _ in exp], HUB, ("dg", L, i))
            assert [r for _, r in got] == [r for _, r in exp], i
            assert list(bank.carry()) == [int(p.carry()[0]) for p in twins.p], i
            for s in range(S):
                assert bank.collector_stats(s) == twins.p[s].collector_stats(0), (i, s)
    assert mismatches(ctx) == 0


def test_twins_process_datagrams_follow_meta(oracle, ctx):
    """follow meta on, incoming frames with real meta blocks (the eight sender kinds of tests/test_gpu_rx_follow_meta.py): KF's CRC
    is formed over each stream's own third word"""
    import sdrdaemon_amd as sd

    fec, L = [0, 1, 12, 32, 127, 4, 13, 33], 0
    S = len(fec)
    calls = tf.follow_calls(oracle, 31, L, 3, 3)
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    bank, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, fec, **cfg)
    bank.set_stream_fec(fec)
    bank.set_follow_meta(True)
    for p in twins.p:
        p.set_follow_meta(True)
    followed = 0
    for i, chunk in enumerate(calls):
        secs, usecs = stamps(i, S)
        got = bank.process_datagrams(chunk, secs, usecs)
        exp = twins.datagrams(chunk, secs, usecs)
        same([g for g, _ in got], [e for e, _ in exp], fec, ("follow", i))
        for s, (g, _) in enumerate(got):
            for fr in np.asarray(g):
                assert tf.crc_ok(fr) and fr[0, 15] == fec[s], (i, s)
                followed += tf.meta_of(fr)[:2] != (435000, 625000)
    assert followed >= 8  # (frames that announce their sender's values, not the configuration's)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 3. a change in flight
def test_a_change_between_calls_with_frames_open(ctx):
    """set_stream_fec between calls while frames are open: stream 1 raised so that the pitch grows, stream 3 lowered, then NULL;
    the twins get reconfigure(nb_fec=...) at the same points.  The open frame keeps its old nbFECBlocks byte and is encoded with
    the new count"""
    import sdrdaemon_amd as sd

    L, cfg_fec = 1, 8
    steps = [[4, 8, 0, 32, 4], [4, 64, 0, 32, 4], [4, 64, 0, 2, 4], None, [1, 1, 1, 1, 1]]
    S = 5
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    bank, twins = sd.RxPipe(ctx, S, nb_fec=cfg_fec, **cfg), Twins(ctx, [cfg_fec] * S, **cfg)
    rs = np.random.RandomState(4)
    prev = [cfg_fec] * S
    for k, fec in enumerate(steps):
        bank.set_stream_fec(fec)
        now = fec if fec is not None else [cfg_fec] * S
        twins.reconfigure(now)
        assert [bank.stream_fec(s) for s in range(S)] == [(now[s], 128 + max(now)) for s in range(S)]
        xs, counts = ragged_blocks(rs, S, L, [2] * S, k == 0)  # (k = 0 leaves every stream's frame open from then on)
        secs, usecs = stamps(k, S)
        got, nf = bank.process_ragged(rows_of(xs, counts), counts, secs, usecs)
        if fec is None:  # (bank-wide again: one array of equal frames)
            got = [got[s, :nf[s]] for s in range(S)]
        same(got, twins.ragged(xs, counts, secs, usecs), now, ("change", k))
        if k:
            for s in range(S):  # the frame that was open across the change: the old byte in its meta block, the new count of blocks
                first = np.asarray(got[s][0])
                assert first[0, 15] == prev[s] and first.shape[0] == 128 + now[s], (k, s)
                assert np.asarray(got[s][1])[0, 15] == now[s], (k, s)
        prev = now


# ------------------------------------------------------------------------------------------------ 4. egress
def twin_rounds(exp):
    """the twins' frames of one batch in departure order"""
    return rounds([np.asarray(e) for e in exp])


def same_egress(rx, got, exp, recs, fec, where):
    dg, tags, nf, records = got
    e_dg, e_tags = twin_rounds(exp)
    print(where, "n_frames", list(nf), "blocks", rx.last_stream_blocks, "n_dgrams", dg.shape[0])
    assert list(nf) == [np.asarray(e).shape[0] for e in exp], where
    assert dg.shape == e_dg.shape == (sum(int(nf[s]) * (128 + fec[s]) for s in range(len(fec))), 512), where
    assert np.array_equal(tags, e_tags), where
    assert dg.tobytes() == e_dg.tobytes(), where
    assert records == recs, where
    if dg.shape[0]:
        assert rx.last_blocks_per_frame == 0 and rx.last_stream_blocks == [128 + r for r in fec], where


@pytest.mark.parametrize("L,tagged,depth", [(0, False, 1), (1, True, 4), (0, True, 1), (1, False, 4)])
def test_egress_datagram_batches(oracle, ctx, L, tagged, depth):
    """nb_fec = [0, 1, 32, 127, 4] over PLAN's batches (zeros at the first, a middle and the last stream, 0 .. 3 frames), untagged
    and tagged, depths 1 and 4: array, tags, n_frames, last_stream_blocks and records equal rounds() over the twins' frames;
    d2h_bytes per batch exact; carry and collector statistics equal the twins' after every batch"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S = len(calls[0])
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, HUB, **cfg)
    a.set_stream_fec(HUB)
    a.set_async(depth=depth)
    a.set_egress("round_robin")
    got, exp, down = [], [], []
    for i, chunk in enumerate(calls):
        secs, usecs = stamps(i, S)
        while True:
            d0 = ctx.counter("d2h_bytes")
            try:
                if tagged:
                    arr, tags = merge(chunk, 60 + i, skip=3)
                    a.submit_datagrams_tagged(arr, tags, secs, usecs)
                else:
                    a.submit_datagrams(chunk, secs, usecs)
                break
            except sd.SdrHipError as e:
                assert e.code == EBUSY
                got.append(a.collect_egress())
        down.append(ctx.counter("d2h_bytes") - d0)
        exp.append(twins.datagrams(chunk, secs, usecs))
        assert list(a.carry()) == [int(p.carry()[0]) for p in twins.p], i
        for s in range(S):
            assert a.collector_stats(s) == twins.p[s].collector_stats(0), (i, s)
    while len(got) < len(calls):
        got.append(a.collect_egress())
    assert a.collect_egress(wait=False) is None
    zero_at, seen = set(), set()
    for i, e in enumerate(exp):
        same_egress(a, got[i], [fr for fr, _ in e], [r for _, r in e], HUB, (L, tagged, i))
        nf = [np.asarray(fr).shape[0] for fr, _ in e]
        assert down[i] == sum(nf[s] * (128 + HUB[s]) * 512 for s in range(S)) + sum(len(r) for _, r in e) * 16, i
        zero_at |= {s for s in range(S) if nf[s] == 0}
        seen |= {len(r) for _, r in e}  # (frames released per stream and batch; with L = 1 two of them make one outgoing frame)
    assert {0, 2, S - 1} <= zero_at and seen == {0, 1, 2, 3}, (zero_at, seen)
    assert mismatches(ctx) == 0


def test_egress_ragged_batches(ctx):
    """sample-fed batches, two blocks per batch: the same against the twins fed the batch's summed counts"""
    import sdrdaemon_amd as sd

    L, S = 1, 5
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, HUB, **cfg)
    a.set_stream_fec(HUB)
    a.set_async(depth=2, blocks=2)
    a.set_egress("round_robin")
    rs = np.random.RandomState(9)
    for i in range(0, len(PLAN), 2):
        blocks = [ragged_blocks(rs, S, L, PLAN[i + j], i + j == 0) for j in (0, 1)]
        d0 = ctx.counter("d2h_bytes")
        for xs, counts in blocks:
            a.submit_ragged(np.concatenate(xs).reshape(-1), counts, 100 + i, i)
        down = ctx.counter("d2h_bytes") - d0
        both = [np.concatenate([blocks[0][0][s], blocks[1][0][s]]) for s in range(S)]
        tot = [blocks[0][1][s] + blocks[1][1][s] for s in range(S)]
        exp = twins.ragged(both, tot, [100 + i] * S, [i] * S)
        got = a.collect_egress()
        same_egress(a, got, exp, None, HUB, ("ragged", i))
        assert down == got[0].shape[0] * 512, i
    assert a.collect_egress(wait=False) is None


def test_egress_batch_without_a_frame_in_a_used_slot(ctx):
    """depth 1, so every batch takes the same ring slot: a departure-order batch that completes no frame in any stream, behind one
    that did, is empty -- no datagrams, no tags, nothing of the slot's earlier batch -- with differing counts, and again after
    set_stream_fec(None); the batch after it still equals the twins"""
    import sdrdaemon_amd as sd

    L, S = 1, 5
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, HUB, **cfg)
    a.set_stream_fec(HUB)
    a.set_async(depth=1)
    a.set_egress("round_robin")
    rs = np.random.RandomState(23)
    fec = HUB
    for i, frames in enumerate([[2, 1, 0, 1, 2], None, [1, 0, 2, 1, 1], "bank-wide", None, [1, 1, 1, 0, 2]]):
        if frames == "bank-wide":
            a.set_stream_fec(None)
            fec = [8] * S
            twins.reconfigure(fec)
            continue
        if frames is None:  # (fewer samples than a frame has left, one stream nothing)
            counts = [40 << L, 0, 8 << L, 2 << L, 100 << L]
            xs = [rs.randint(-32768, 32768, size=(c, 2)).astype(np.int16) for c in counts]
        else:
            xs, counts = ragged_blocks(rs, S, L, frames, i == 0)
        d0 = ctx.counter("d2h_bytes")
        a.submit_ragged(np.concatenate(xs).reshape(-1), counts, 100 + i, i)
        down = ctx.counter("d2h_bytes") - d0
        exp = twins.ragged(xs, counts, [100 + i] * S, [i] * S)
        dg, tags, nf, recs = a.collect_egress(copy=False)
        if frames is None:
            assert dg.shape == (0, 512) and tags.shape == (0,) and list(nf) == [0] * S and recs is None and down == 0, (i, dg.shape, tags.shape)
            assert all(np.asarray(e).shape[0] == 0 for e in exp)
        elif fec is HUB:
            same_egress(a, (dg, tags, nf, recs), exp, None, HUB, ("slot", i))
        else:
            e_dg, e_tags = twin_rounds(exp)
            assert a.last_blocks_per_frame == 136 and a.last_stream_blocks is None
            assert dg.tobytes() == e_dg.tobytes() and np.array_equal(tags, e_tags) and list(nf) == frames, i
        a.release_egress()


# ------------------------------------------------------------------------------------------------ 5. equal counts
def test_equal_counts_through_the_array(oracle, ctx):
    """an array of equal entries: the bytes of the handle whose config carries that count, blocks_per_frame = 128 + R"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S, R, L = len(calls[0]), 32, 0
    a, b = sd.RxPipe(ctx, S, log2decim=L, nb_fec=8), sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    a.set_stream_fec([R] * S)
    for p in (a, b):
        p.set_egress("round_robin")
    for i in (0, 1, 2):
        secs, usecs = stamps(i, S)
        a.submit_datagrams(calls[i], secs, usecs)
        b.submit_datagrams(calls[i], secs, usecs)
        ga, gb = a.collect_egress(), b.collect_egress()
        assert a.last_blocks_per_frame == b.last_blocks_per_frame == 128 + R and a.last_stream_blocks is None
        assert ga[0].tobytes() == gb[0].tobytes() and np.array_equal(ga[1], gb[1]) and list(ga[2]) == list(gb[2]) and ga[3] == gb[3]
    a.set_egress(None)  # (stream order is open to equal counts)
    b.set_egress(None)
    a.submit_datagrams(calls[3], 1, 2)
    b.submit_datagrams(calls[3], 1, 2)
    ea, eb = a.collect_datagrams(), b.collect_datagrams()
    assert sum(f.shape[0] for f, _ in eb) > 0
    same([f for f, _ in ea], [f for f, _ in eb], [R] * S, "stream order")
    xs, counts = ragged_blocks(np.random.RandomState(1), S, L, [1, 2, 0, 1, 1], False)
    ga, na = a.process_ragged(rows_of(xs, counts), counts, 3, 4)
    gb, nb = b.process_ragged(rows_of(xs, counts), counts, 3, 4)
    assert list(na) == list(nb)
    same(ga, [gb[s, :nb[s]] for s in range(S)], [R] * S, "sync")
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_consume_nothing(oracle, ctx):
    """each refused call leaves the pipe where it was: the next accepted call still matches the twins"""
    import ctypes as C

    import sdrdaemon_amd as sd

    L, S = 0, 5
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, HUB, **cfg)
    rs = np.random.RandomState(14)
    calls = dgram_calls(oracle)
    step = [0]

    def accepted():
        xs, counts = ragged_blocks(rs, S, L, [1, 2, 1, 0, 1], step[0] == 0)
        secs, usecs = stamps(step[0], S)
        step[0] += 1
        got, _ = a.process_ragged(rows_of(xs, counts), counts, secs, usecs)
        same(got, twins.ragged(xs, counts, secs, usecs), HUB, ("accepted", step[0]))
        return xs, counts

    assert code(a.set_stream_fec, [0, 1, 129, 4, 4]) == EINVAL and code(a.set_stream_fec, [0, -1, 32, 4, 4]) == EINVAL
    assert a.stream_fec(2) == (8, 136)  # (nothing changed)
    a.set_stream_fec(HUB)
    xs, counts = accepted()
    # ---- the uniform entries and pipelined mode
    x = rows_of(xs, counts)[:, :64]
    assert code(a.process, x) == EINVAL and code(a.submit, x) == EINVAL
    assert ctx.lib.sdrhip_rx_set_pipelined(a.h, 1) == EINVAL
    accepted()
    # ---- a frame stride one byte short (the largest n_frames[s] * (128 + nb_fec[s]) * 512: stream 1's two frames of 129, not 3's none)
    xs, counts = ragged_blocks(rs, S, L, [1, 2, 1, 0, 1], False)
    need = 2 * 129 * 512
    assert max(n * (128 + r) for n, r in zip([1, 2, 1, 0, 1], HUB)) * 512 == need
    out = np.zeros(S * need, np.uint8)
    nf = (C.c_size_t * S)()
    rows = rows_of(xs, counts)
    args = lambda stride: (a.h, rows.ctypes.data_as(C.c_void_p), (C.c_size_t * S)(*counts), max(counts),  # noqa: E731
                           (C.c_uint32 * S)(*[7] * S), (C.c_uint32 * S)(*[8] * S), out.ctypes.data_as(C.c_void_p), stride, nf, sd.engine.MEM_HOST)
    assert ctx.lib.sdrhip_rx_process_ragged(*args(need - 1)) == EINVAL and list(nf) == [0] * S
    assert ctx.lib.sdrhip_rx_process_ragged(*args(need)) == 0 and list(nf) == [1, 2, 1, 0, 1]
    exp = twins.ragged(xs, counts, [7] * S, [8] * S)
    for s in range(S):
        assert out[s * need:s * need + exp[s].size].tobytes() == np.asarray(exp[s]).tobytes(), s
    # ---- stream-order asynchronous submits with differing counts: departure order only
    packed, pc = np.concatenate(xs).reshape(-1), counts
    with pytest.raises(sd.SdrHipError) as e:
        a.submit_ragged(packed, pc, 1, 2)
    assert e.value.code == EINVAL and "sdrhip_rx_set_egress" in str(e.value)
    arr, tags = merge(calls[0], 5, skip=3)
    for fn, args2 in ((a.submit_datagrams, (calls[0], 1, 2)), (a.submit_datagrams_tagged, (arr, tags, 1, 2))):
        with pytest.raises(sd.SdrHipError) as e:
            fn(*args2)
        assert e.value.code == EINVAL and "sdrhip_rx_set_egress" in str(e.value)
    assert all(v == 0 for v in a.carry())  # (no datagram was consumed)
    accepted()
    # ---- the setter while a batch is in flight, and while one is lent
    a.set_egress("round_robin")
    xs, counts = ragged_blocks(rs, S, L, [1, 0, 2, 1, 1], False)
    a.submit_ragged(np.concatenate(xs).reshape(-1), counts, 11, 12)
    assert code(a.set_stream_fec, [4] * S) == EINVAL and code(a.set_stream_fec, None) == EINVAL
    lent = a.collect_egress(copy=False)
    assert code(a.set_stream_fec, [4] * S) == EINVAL
    same_egress(a, lent, twins.ragged(xs, counts, [11] * S, [12] * S), None, HUB, "lent")
    blocks = (C.c_size_t * S)()
    assert ctx.lib.sdrhip_rx_egress_stream_blocks(a.h, blocks) == 0 and list(blocks) == [128 + r for r in HUB]
    a.release_egress()
    assert ctx.lib.sdrhip_rx_egress_stream_blocks(a.h, blocks) == EINVAL  # (nothing is lent)
    a.set_stream_fec(HUB)  # (accepted again)
    accepted()
    assert mismatches(ctx) == 0
