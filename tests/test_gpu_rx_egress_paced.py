"""The paced departure order (sdrhip_rx_set_egress with SDRHIP_EGRESS_PACED, delivered by KP).  The yardstick is always the existing
stream-order collect on a twin handle of the same context fed the same input: its frames are put in paced order on the host by a
literal statement of the definition -- sort all datagrams by Fraction(2j + 1, 2 D_s), then by stream -- and every comparison is byte
equality.  Every delivered array is also checked, from its tags alone, for the gap guarantee: between two consecutive datagrams of
stream s lie floor(D_t / D_s) or ceil(D_t / D_s) datagrams of every other stream t."""
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_rx_egress as te
from test_gpu_rx_egress import ctx, dgram_calls, merge, mismatches, ragged_blocks, rounds, stamps, submit_both, torch_first  # noqa: F401  (fixtures)
from test_gpu_rx_stream_fec import Twins

pytestmark = pytest.mark.gpu

EBUSY, EINVAL = -6, -1


def paced(per_stream):
    """the definition, literally: per stream an (n_s, B_s, 512) array in wire order -> (datagrams (N, 512), tags (N,))"""
    rows = [np.asarray(f).reshape(-1, 512) for f in per_stream]
    order = sorted((Fraction(2 * j + 1, 2 * r.shape[0]), s, j) for s, r in enumerate(rows) for j in range(r.shape[0]))
    out = [rows[s][j] for _, s, j in order]
    return (np.stack(out) if out else np.zeros((0, 512), np.uint8)), np.asarray([s for _, s, _ in order], np.uint16)


def longest_run(tags):
    best = run = 0
    for i, t in enumerate(tags):
        run = run + 1 if i and t == tags[i - 1] else 1
        best = max(best, run)
    return best


def gaps_hold(tags, S, where):
    """the no-burst guarantee, from the delivered tags alone"""
    tags = np.asarray(tags).astype(np.int64)
    D = np.bincount(tags, minlength=S)
    # before[t][i] = datagrams of stream t among the first i entries
    before = np.zeros((S, tags.shape[0] + 1), np.int64)
    for t in range(S):
        before[t, 1:] = np.cumsum(tags == t)
    for s in range(S):
        at = np.nonzero(tags == s)[0]
        for t in range(S):
            if t == s or at.shape[0] < 2:
                continue
            between = before[t, at[1:]] - before[t, at[:-1] + 1]
            lo, hi = D[t] // D[s], -(-D[t] // D[s])
            assert between.min() >= lo and between.max() <= hi, (where, s, t, int(between.min()), int(between.max()), int(lo), int(hi))


def same_as_twin(rx, got, frames, records, B, where):
    """one collect_egress result of a paced batch against the twin's stream-order frames (and records) of the same batch; B = the
    batch's blocks per frame, or every stream's (a list: per-stream fecblk with differing counts)"""
    assert got is not None, where
    dg, tags, nf, recs = got
    exp_dg, exp_tags = paced(frames)
    S = len(frames)
    each = B if isinstance(B, list) else [B] * S
    print(where, "n_frames", list(nf), "B", rx.last_blocks_per_frame, rx.last_stream_blocks, "n_dgrams", dg.shape[0],
          "longest run", longest_run(tags), "round robin's", longest_run(rounds(frames)[1]))
    assert list(nf) == [np.asarray(f).shape[0] for f in frames], where
    assert dg.dtype == np.uint8 and tags.dtype == np.uint16, where
    assert dg.shape == exp_dg.shape == (sum(int(nf[s]) * each[s] for s in range(S)), 512), where
    assert np.array_equal(tags, exp_tags), where
    assert dg.tobytes() == exp_dg.tobytes(), where
    assert recs == records, where
    if isinstance(B, list):
        if dg.shape[0]:
            assert rx.last_blocks_per_frame == 0 and rx.last_stream_blocks == B, where
    else:
        assert rx.last_blocks_per_frame == B and rx.last_stream_blocks is None, where
    gaps_hold(tags, S, where)


def code(fn, *args, **kw):
    import sdrdaemon_amd as sd

    with pytest.raises(sd.SdrHipError) as e:
        fn(*args, **kw)
    return e.value.code


# ------------------------------------------------------------------------------------------------ 1. datagram batches
@pytest.mark.parametrize("R,tagged,depth", [(0, False, 1), (1, True, 4), (32, True, 1), (1, False, 4)])
def test_datagram_batches(oracle, ctx, R, tagged, depth):
    """decimate1, released counts 0 .. 3 with zeros at the first, a middle and the last stream; outgoing nb_fec 0 / 1 / 32 (B = 128
    and 160: n a multiple of 32; B = 129: a part-filled last workgroup), untagged and tagged submits, depths 1 and 4: array, tags,
    n_frames, blocks_per_frame and records equal the model; carry and collector statistics equal the twin's after every batch; the
    bytes that come down are the twin's"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S, B = len(calls[0]), 128 + R
    a = sd.RxPipe(ctx, S, log2decim=0, nb_fec=R)
    b = sd.RxPipe(ctx, S, log2decim=0, nb_fec=R)
    a.set_async(depth=depth)
    b.set_async(depth=depth)
    a.set_egress("paced")
    got, exp = [], []

    def collect_a():
        d0 = ctx.counter("d2h_bytes")
        g = a.collect_egress()
        assert ctx.counter("d2h_bytes") == d0  # (the one download was counted when the batch was submitted)
        got.append(g)

    for i, chunk in enumerate(calls):
        sec, usec = stamps(i, S)
        for pipe, collect in ((a, collect_a), (b, lambda: exp.append(b.collect_datagrams()))):
            d0 = ctx.counter("d2h_bytes")
            while True:
                try:
                    if tagged and pipe is a:
                        arr, tags = merge(chunk, 60 + i, skip=3)
                        pipe.submit_datagrams_tagged(arr, tags, sec, usec)
                    else:
                        pipe.submit_datagrams(chunk, sec, usec)
                    break
                except sd.SdrHipError as e:
                    assert e.code == EBUSY
                    collect()
                    d0 = ctx.counter("d2h_bytes")
            if pipe is a:
                down_a = ctx.counter("d2h_bytes") - d0
            else:
                assert ctx.counter("d2h_bytes") - d0 == down_a, i  # (link traffic of such a batch is unchanged)
        assert list(a.carry()) == list(b.carry()), i
        for s in range(S):
            assert a.collector_stats(s) == b.collector_stats(s), (i, s)
    while len(got) < len(calls):
        collect_a()
    while len(exp) < len(calls):
        exp.append(b.collect_datagrams())
    assert a.collect_egress(wait=False) is None
    seen, zero_at, unequal = set(), set(), 0
    for i, e in enumerate(exp):
        same_as_twin(a, got[i], [fr for fr, _ in e], [recs for _, recs in e], B, (R, i))
        seen |= {len(recs) for _, recs in e}
        zero_at |= {s for s in range(S) if e[s][0].shape[0] == 0}
        unequal += len({fr.shape[0] for fr, _ in e if fr.shape[0]}) > 1
    assert seen == {0, 1, 2, 3} and {0, 2, S - 1} <= zero_at and unequal >= 4, (seen, zero_at, unequal)
    assert mismatches(ctx) == 0


def test_records_only_batch(oracle, ctx):
    """decimate64: every stream's collector releases frames (in the second batch exactly one) whose samples complete no outgoing
    frame -- n_dgrams = 0, and the records are delivered where the array would end"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S = len(calls[0])
    whole = [np.concatenate([c[s] for c in calls]) for s in range(S)]
    a, b = sd.RxPipe(ctx, S, log2decim=6, fcpos=sd.FC_CEN, nb_fec=1), sd.RxPipe(ctx, S, log2decim=6, fcpos=sd.FC_CEN, nb_fec=1)
    a.set_egress("paced")
    # (the first batch starts the collectors, which release more than the one frame then; the second holds the 130 datagrams
    # that end with the first one of the frame after: one released frame per stream)
    for k, (lo, hi) in enumerate(((0, 131), (131, 261))):
        chunk = [w[lo:hi] for w in whole]
        d0 = ctx.counter("d2h_bytes")
        a.submit_datagrams(chunk, 5, 6 + k)
        down_a = ctx.counter("d2h_bytes") - d0
        b.submit_datagrams(chunk, 5, 6 + k)
        assert ctx.counter("d2h_bytes") - d0 == 2 * down_a  # (the twin's batch brings down the same bytes)
        e = b.collect_datagrams()
        dg, tags, nf, recs = a.collect_egress()
        print("records", [len(r) for r in recs], "down", down_a)
        assert dg.shape == (0, 512) and tags.shape == (0,) and list(nf) == [0] * S
        assert all(fr.shape[0] == 0 for fr, _ in e)
        assert recs == [r for _, r in e] and min(len(r) for r in recs) >= 1
        assert down_a == 16 * sum(len(r) for r in recs)
        assert list(a.carry()) == list(b.carry())
    assert [len(r) for r in recs] == [1] * S
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 2. ragged sample-fed batches
@pytest.mark.parametrize("case", ["five_streams", "one_stream", "u8_input"])
def test_ragged_batches(ctx, case):
    """decimate2_cen with unequal frame counts (zeros among them); S = 1 (the identity order); 8-bit input with B = 255"""
    import sdrdaemon_amd as sd

    c = te.RAGGED[case]
    S, L, R, plan, fmt = c["S"], c["L"], c["R"], c["plan"], c.get("fmt", "s16")
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R, input_format=fmt, sample_bits=8 if fmt != "s16" else 16)
    a, b = sd.RxPipe(ctx, S, **cfg), sd.RxPipe(ctx, S, **cfg)
    a.set_async(depth=4)
    b.set_async(depth=4)
    a.set_egress("paced")
    rs = np.random.RandomState(len(case))
    for i, frames in enumerate(plan):
        xs, counts = ragged_blocks(rs, S, L, frames, i == 0, fmt)
        d0 = ctx.counter("d2h_bytes")
        submit_both(a, b, xs, counts, 100 + i, i)
        assert ctx.counter("d2h_bytes") - d0 == 2 * sum(frames) * (128 + R) * 512, i
    for k in range(len(plan)):
        exp = b.collect_ragged()
        assert [e.shape[0] for e in exp] == plan[k], (case, k)
        same_as_twin(a, a.collect_egress(), exp, None, 128 + R, (case, k))
    assert a.collect_egress(wait=False) is None and b.collect_ragged(wait=False) is None
    assert mismatches(ctx) == 0


def test_equal_counts_are_the_round_robin_array(ctx):
    """equal counts: the paced array is byte for byte that of a third handle in round robin (and the twin's frames in rounds)"""
    import sdrdaemon_amd as sd

    c = te.RAGGED["equal_counts"]
    S, L, R, plan = c["S"], c["L"], c["R"], c["plan"]
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    a, r, b = sd.RxPipe(ctx, S, **cfg), sd.RxPipe(ctx, S, **cfg), sd.RxPipe(ctx, S, **cfg)
    for p in (a, r, b):
        p.set_async(depth=4)
    a.set_egress("paced")
    r.set_egress("round_robin")
    rs = np.random.RandomState(12)
    for i, frames in enumerate(plan):
        xs, counts = ragged_blocks(rs, S, L, frames, i == 0)
        submit_both(a, b, xs, counts, 100 + i, i)
        r.submit_ragged(np.concatenate(xs).reshape(-1), counts, 100 + i, i)
    for k in range(len(plan)):
        exp = b.collect_ragged()
        ga, gr = a.collect_egress(), r.collect_egress()
        assert ga[0].shape == gr[0].shape == (sum(plan[k]) * (128 + R), 512)
        assert ga[0].tobytes() == gr[0].tobytes() == rounds(exp)[0].tobytes(), k
        assert np.array_equal(ga[1], gr[1]) and list(ga[2]) == list(gr[2]) == plan[k], k
        same_as_twin(a, ga, exp, None, 128 + R, ("equal", k))


def test_tie_rule(ctx):
    """two streams with 3 and 1 frames of equal length: datagram i of stream 1 has the key of datagram 3 i + 1 of stream 0, and
    stream 0's comes first at every one of them"""
    import sdrdaemon_amd as sd

    S, L, R = 2, 0, 1
    B = 128 + R
    a, b = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R), sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    a.set_egress("paced")
    xs, counts = ragged_blocks(np.random.RandomState(31), S, L, [3, 1], True)
    submit_both(a, b, xs, counts, 1, 2)
    exp = b.collect_ragged()
    got = a.collect_egress()
    same_as_twin(a, got, exp, None, B, "tie")
    tags = got[1]
    at1 = np.nonzero(tags == 1)[0]
    assert at1.shape[0] == B
    for i, p in enumerate(at1):
        assert tags[p - 1] == 0 and int(np.sum(tags[:p] == 0)) == 3 * i + 2, i  # (stream 0's datagrams 0 .. 3 i + 1 lie before it)
        assert got[0][p - 1].tobytes() == np.asarray(exp[0]).reshape(-1, 512)[3 * i + 1].tobytes(), i


def test_per_stream_fecblk(ctx):
    """nb_fec (0, 1, 32) with frames (2, 1, 3), then (1, 2, 0): blocks_per_frame == 0, sdrhip_rx_egress_stream_blocks lists
    128, 129, 160, and the array is the paced order of the one-stream twins' frames; exactly its datagrams come down"""
    import sdrdaemon_amd as sd

    L, S, fec = 1, 3, [0, 1, 32]
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, fec, **cfg)
    a.set_stream_fec(fec)
    a.set_async(depth=2)
    a.set_egress("paced")
    rs = np.random.RandomState(17)
    for i, frames in enumerate([[2, 1, 3], [1, 2, 0]]):
        xs, counts = ragged_blocks(rs, S, L, frames, i == 0)
        d0 = ctx.counter("d2h_bytes")
        a.submit_ragged(np.concatenate(xs).reshape(-1), counts, 100 + i, i)
        down = ctx.counter("d2h_bytes") - d0
        exp = twins.ragged(xs, counts, [100 + i] * S, [i] * S)
        got = a.collect_egress()
        same_as_twin(a, got, exp, None, [128 + r for r in fec], ("fecblk", i))
        assert list(got[2]) == frames and down == got[0].shape[0] * 512, i
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 3. window wrap, reconfigure
def test_window_wrap_and_reconfigure(ctx):
    """rx_window = 1: the frame area holds one call's window (at most 3 + 1 slots), so a stream that delivers more than 4 frames
    has wrapped; sdrhip_rx_reconfigure to another nb_fec with a batch uncollected: each batch reports its own blocks_per_frame"""
    import sdrdaemon_amd as sd

    S, L = 5, 1
    plan = [[2, 0, 3, 1, 1], [1, 3, 0, 2, 1], [3, 1, 1, 0, 2], [0, 2, 2, 3, 1], [1, 1, 3, 1, 0], [2, 0, 1, 2, 3]]
    fec = [8, 8, 8, 8, 1, 32]  # nb_fec each batch is submitted with (a fecblk change gives the windows a new area)
    ctx.set_option("rx_window", 1)
    try:
        a = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=fec[0])
        b = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=fec[0])
        a.set_async(depth=4)
        a.set_egress("paced")
        rs = np.random.RandomState(21)
        exp, got = [], []

        def collect_a():
            g = a.collect_egress()
            got.append((g, a.last_blocks_per_frame))

        for i, frames in enumerate(plan):
            if i and fec[i] != fec[i - 1]:
                a.reconfigure(nb_fec=fec[i])  # (batch i - 1 of `a` has not been collected)
                b.reconfigure(nb_fec=fec[i])
            xs, counts = ragged_blocks(rs, S, L, frames, i == 0)
            submit_both(a, b, xs, counts, 50 + i, 2 * i)
            exp.append(b.collect_ragged())  # (the twin collects at once: its shapes follow the configuration in force)
            if i:
                collect_a()  # (batch i - 1)
        collect_a()
        for i, (g, bpf) in enumerate(got):
            a.last_blocks_per_frame = bpf
            same_as_twin(a, g, exp[i], None, 128 + fec[i], ("wrap", i))
        # the four batches of the first area: every stream delivers more frames than the area has slots per stream
        assert max(max(p) for p in plan) == 3 and min(sum(p[s] for p in plan[:4]) for s in range(S)) > 1 * (3 + 1)
    finally:
        ctx.set_option("rx_window", 0)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 4. both orders in one ring, lending
def test_both_orders_in_the_ring_and_lending(ctx):
    """depth 4: a round-robin batch, a paced batch and another round-robin batch in flight together, each collected in the order
    it was launched with.  depth 2: the views collect_egress(copy=False) lends stay valid and unchanged while a later batch
    completes, a submit that finds one slot in flight and one lent is SDRHIP_EBUSY until the release; every value but 0, 1, 2 is
    refused"""
    import sdrdaemon_amd as sd

    S, L, R = 3, 0, 1
    B = 128 + R
    a, b = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R), sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    rs = np.random.RandomState(8)
    first = [True]

    def block(frames):
        xs, counts = ragged_blocks(rs, S, L, frames, first[0])
        first[0] = False
        return xs, counts

    a.set_async(depth=4)
    b.set_async(depth=4)
    for bad in (3, 7, -1):
        assert code(a.set_egress, bad) == EINVAL
    exp = []
    for order, frames in (("round_robin", [3, 0, 1]), ("paced", [1, 0, 3]), ("round_robin", [2, 1, 0])):
        a.set_egress(order)  # (batches are in flight, none is being filled: accepted)
        xs, counts = block(frames)
        submit_both(a, b, xs, counts, 9, len(exp))
        exp.append((order, b.collect_ragged()))
    for k, (order, e) in enumerate(exp):
        if order == "paced":
            g = a.collect_egress()
            same_as_twin(a, g, e, None, B, ("ring", k))
            assert longest_run(g[1]) <= 3 < longest_run(rounds(e)[1])
        else:
            te.same_as_twin(a, a.collect_egress(), e, None, B, ("ring", k))
    assert a.collect_egress(wait=False) is None

    # ---- lending
    a.set_async(depth=2)
    b.set_async(depth=2)
    a.set_egress("paced")
    assert code(a.submit, np.zeros((S, 64, 2), np.int16)) == EINVAL  # (uniform batches have no order: nothing consumed)
    x1, c1 = block([2, 1, 0])
    submit_both(a, b, x1, c1, 9, 10)
    e1 = b.collect_ragged()
    x2, c2 = block([0, 1, 3])
    submit_both(a, b, x2, c2, 9, 11)
    e2 = b.collect_ragged()
    assert code(a.collect_ragged) == EINVAL  # (a mismatched collect: the batch stays ...)
    lent = a.collect_egress(copy=False)      # (... and is collected afterwards)
    same_as_twin(a, lent, e1, None, B, "lent")
    at = (lent[0].ctypes.data, lent[1].ctypes.data)
    snapshot = (lent[0].copy(), lent[1].copy())
    x3, c3 = block([1, 1, 1])
    assert code(a.submit_ragged, np.concatenate(x3).reshape(-1), c3, 9, 12) == EBUSY  # (one slot in flight, one lent)
    assert code(a.set_async, 2, 1) == EINVAL                                           # (the ring is busy)
    ctx.synchronize()  # (the later batch has completed)
    assert (lent[0].ctypes.data, lent[1].ctypes.data) == at
    assert np.array_equal(lent[0], snapshot[0]) and np.array_equal(lent[1], snapshot[1])
    a.release_egress()
    a.release_egress()  # (nothing lent: SDRHIP_OK)
    submit_both(a, b, x3, c3, 9, 12)
    e3 = b.collect_ragged()
    same_as_twin(a, a.collect_egress(), e2, None, B, "second")
    same_as_twin(a, a.collect_egress(), e3, None, B, "third")
    assert a.collect_egress(wait=False) is None
    assert mismatches(ctx) == 0
