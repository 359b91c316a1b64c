"""Departure-order egress (sdrhip_rx_set_egress / sdrhip_rx_collect_egress / sdrhip_rx_release_egress).  The yardstick is always
the existing stream-order collect on a twin handle of the same context fed the same input: its frames are put in departure order on
the host by a literal simulation of the rounds (round j = datagram j of every stream that still has one, streams ascending), and
every comparison is byte equality.  Every test also checks that the host's shadow of the classification never disagreed with the
device ("fecbuf_shadow_mismatch" stays 0)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_tx_datagrams as tt
from test_gpu_dgram_tagged import merge
from test_gpu_rx_datagrams import torch_first  # noqa: F401  (fixture)
from test_gpu_rx_datagrams_async import stamps
from test_gpu_rx_ragged_async import rand_block

pytestmark = pytest.mark.gpu

F = 16129
EBUSY, EINVAL = -6, -1
ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)


def mismatches(ctx):
    return ctx.counter("fecbuf_shadow_mismatch")


def rounds(per_stream):
    """the definition, literally: per stream an (n_s, B, 512) array in wire order -> (datagrams (N, 512), tags (N,))"""
    rows = [np.asarray(f).reshape(-1, 512) for f in per_stream]
    out, tags, j = [], [], 0
    while True:
        live = [s for s, r in enumerate(rows) if r.shape[0] > j]
        if not live:
            break
        for s in live:
            out.append(rows[s][j])
            tags.append(s)
        j += 1
    return (np.stack(out) if out else np.zeros((0, 512), np.uint8)), np.asarray(tags, np.uint16)


def same_as_twin(rx, got, frames, records, B, where):
    """one collect_egress result against the twin's stream-order frames (and records) of the same batch"""
    assert got is not None, where
    dg, tags, nf, recs = got
    exp_dg, exp_tags = rounds(frames)
    print(where, "n_frames", list(nf), "B", rx.last_blocks_per_frame, "n_dgrams", dg.shape[0])
    assert list(nf) == [np.asarray(f).shape[0] for f in frames], where
    assert rx.last_blocks_per_frame == B, where
    assert dg.dtype == np.uint8 and tags.dtype == np.uint16 and dg.shape == exp_dg.shape == (B * int(sum(nf)), 512), where
    assert np.array_equal(tags, exp_tags), where
    assert dg.tobytes() == exp_dg.tobytes(), where
    assert recs == records, where


# ------------------------------------------------------------------------------------------------ 1. datagram batches
# frames each stream's datagrams of a batch make its collector release (a frame is released by the first datagram of the next one):
# a zero at the first, a middle and the last stream, every count of 0 .. 3
PLAN = [[0, 2, 1, 2, 1], [1, 0, 3, 2, 0], [2, 1, 0, 1, 3], [3, 3, 2, 0, 2], [1, 2, 0, 3, 0], [0, 1, 1, 2, 1]]
_DG = {}


def dgram_calls(oracle):
    """5 streams, incoming fecblk 4 with two originals lost per frame (130 datagrams a frame); batch i holds PLAN[i][s] frames'
    worth of stream s, cut one datagram into the next frame.  Kept: every case shares it"""
    if "calls" not in _DG:
        rs = np.random.RandomState(77)
        S = len(PLAN[0])
        per = []
        for s in range(S):
            dg = []
            for fr in tg.make_frames(oracle, rs, sum(p[s] for p in PLAN) + 1, 4, 100 * s):
                lost = set(rs.choice(np.arange(1, 128), 2, replace=False).tolist())
                dg += [fr[i] for i in range(132) if i not in lost]
            per.append(np.asarray(dg, np.uint8).reshape(-1, 512))
        calls, at = [], [0] * S
        for p in PLAN:
            chunk = []
            for s in range(S):
                n = 130 * p[s] + (1 if at[s] == 0 and p[s] else 0)
                chunk.append(per[s][at[s]:at[s] + n])
                at[s] += n
            calls.append(chunk)
        _DG["calls"] = calls
    return _DG["calls"]


DG_CASES = [(L, R, k % 2 == 1, 1 if k % 4 < 2 else 4) for k, (L, R) in enumerate((L, R) for L in (0, 1) for R in (0, 1, 32, 127))]


@pytest.mark.parametrize("L,R,tagged,depth", DG_CASES)
def test_datagram_batches(oracle, ctx, L, R, tagged, depth):
    """decimate1 and decimate2_cen, outgoing nb_fec 0 / 1 / 32 / 127 (B = 129: the odd count, a partial last workgroup and a
    half-filled wave; B = 255: the largest), untagged and tagged submits, depths 1 and 4: array, tags, n_frames, blocks_per_frame
    and records equal the model; carry and collector statistics equal the twin's after every batch; d2h bytes exact"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S, B = len(calls[0]), 128 + R
    a = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    b = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    a.set_async(depth=depth)
    b.set_async(depth=depth)
    a.set_egress("round_robin")
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
    seen, zero_at = set(), set()
    for i, e in enumerate(exp):
        same_as_twin(a, got[i], [fr for fr, _ in e], [recs for _, recs in e], B, (L, R, i))
        rel = [len(recs) for _, recs in e]
        print("released", rel)
        assert max(rel) <= 3
        seen |= set(rel)
        zero_at |= {s for s in range(S) if e[s][0].shape[0] == 0}
    assert seen == {0, 1, 2, 3} and {0, 2, S - 1} <= zero_at, (seen, zero_at)
    assert sum(g[0].shape[0] for g in got) >= 10 * B
    assert mismatches(ctx) == 0


def test_datagram_batch_d2h_bytes_and_max_released(oracle, ctx):
    """down exactly sum n_frames x B x 512 + sum n_released x 16 in one copy; a stream with more records than max_released leaves
    the batch where it is with both count arrays filled"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S, R = len(calls[0]), 1
    a = sd.RxPipe(ctx, S, log2decim=0, nb_fec=R)
    a.set_egress()
    for i in (0, 1, 2):
        d0 = ctx.counter("d2h_bytes")
        a.submit_datagrams(calls[i], 5, 6)
        down = ctx.counter("d2h_bytes") - d0
        if i == 2:
            with pytest.raises(sd.SdrHipError) as e:
                a.collect_egress(max_released=1)
            assert e.value.code == EINVAL and max(a.last_n_released) > 1 and sum(a.last_n_frames) > 0
        dg, tags, nf, recs = a.collect_egress()
        assert down == int(nf.sum()) * (128 + R) * 512 + sum(len(r) for r in recs) * 16, i
        assert dg.shape[0] == int(nf.sum()) * (128 + R)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 2. ragged sample-fed batches
def ragged_blocks(rs, S, L, frames, first, fmt="s16"):
    """one block that completes frames[s] frames of stream s (`first`: a few samples more, so that frames stay open between batches)"""
    counts = [(f * F << L) + ((3 + 5 * s) << L if first else 0) for s, f in enumerate(frames)]
    return rand_block(rs, counts, fmt), counts


def submit_both(a, b, xs, counts, sec, usec):
    packed = np.concatenate(xs).reshape(-1)
    a.submit_ragged(packed, counts, sec, usec)
    b.submit_ragged(packed, counts, sec, usec)


RAGGED = {
    "five_streams": dict(S=5, L=1, R=8, plan=[[2, 0, 3, 1, 1], [0, 1, 1, 3, 0], [1, 2, 0, 0, 2]]),
    "one_stream": dict(S=1, L=1, R=1, plan=[[2], [0], [3]]),
    "equal_counts": dict(S=5, L=1, R=32, plan=[[2] * 5, [1] * 5]),
    "two_blocks": dict(S=5, L=1, R=8, plan=[[1, 0, 2, 1, 0], [1, 0, 1, 0, 1], [0, 2, 0, 1, 1], [2, 1, 1, 0, 0]], blocks=2),
    "u8_input": dict(S=5, L=1, R=127, plan=[[2, 0, 3, 1, 1], [1, 1, 0, 0, 2]], fmt="u8"),
    "longest_run": dict(S=3, L=1, R=128, plan=[[2, 0, 1], [1, 1, 0]]),  # (B = 256: 8 workgroups per run)
}


@pytest.mark.parametrize("case", sorted(RAGGED))
def test_ragged_batches(ctx, case):
    """decimate2_cen with frame counts [2, 0, 3, 1, 1]; S = 1 (the identity order); equal counts; two blocks per batch; 8-bit input; nb_fec = 128
    (frames of 256 datagrams, the run kernel's longest run)"""
    import sdrdaemon_amd as sd

    c = RAGGED[case]
    S, L, R, plan, blocks, fmt = c["S"], c["L"], c["R"], c["plan"], c.get("blocks", 1), c.get("fmt", "s16")
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R, input_format=fmt, sample_bits=8 if fmt != "s16" else 16)
    a, b = sd.RxPipe(ctx, S, **cfg), sd.RxPipe(ctx, S, **cfg)
    a.set_async(depth=4, blocks=blocks)
    b.set_async(depth=4, blocks=blocks)
    a.set_egress("round_robin")
    rs = np.random.RandomState(len(case))
    for i, frames in enumerate(plan):
        xs, counts = ragged_blocks(rs, S, L, frames, i == 0, fmt)
        submit_both(a, b, xs, counts, 100 + i, i)
    nb = len(plan) // blocks
    total = 0
    for k in range(nb):
        exp = b.collect_ragged()
        if blocks == 1:
            assert [e.shape[0] for e in exp] == plan[k], (case, k)
        same_as_twin(a, a.collect_egress(), exp, None, 128 + R, (case, k))
        total += sum(e.shape[0] for e in exp)
    assert a.collect_egress(wait=False) is None and b.collect_ragged(wait=False) is None
    assert total == sum(sum(p) for p in plan)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 3. header walk
def test_header_walk(ctx):
    """independent of the twin: over 6 consecutive batches every stream's subsequence carries blockIndex 0 .. B - 1 per frame, and
    frameIndex increases by one per frame and continues across batches"""
    import sdrdaemon_amd as sd

    S, L, R = 5, 0, 1
    B = 128 + R
    plan = [[2, 0, 3, 1, 1], [0, 1, 1, 3, 0], [1, 2, 0, 0, 2], [3, 1, 1, 2, 0], [0, 0, 2, 1, 3], [1, 3, 0, 0, 1]]
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    rx.set_async(depth=2)
    rx.set_egress("round_robin")
    rs = np.random.RandomState(3)
    nxt = [None] * S
    for i, frames in enumerate(plan):
        xs, counts = ragged_blocks(rs, S, L, frames, i == 0)
        rx.submit_ragged(np.concatenate(xs).reshape(-1), counts, 7, i)
        dg, tags, nf, recs = rx.collect_egress()
        assert list(nf) == frames and recs is None and dg.shape[0] == B * sum(frames)
        for s in range(S):
            mine = dg[tags == s].reshape(-1, B, 512)
            assert mine.shape[0] == frames[s]
            for fr in mine:
                assert np.array_equal(fr[:, 2], np.arange(B, dtype=np.uint8)), (i, s)
                fi = int(fr[0, 0]) | int(fr[0, 1]) << 8
                assert np.all(fr[:, 0] == fr[0, 0]) and np.all(fr[:, 1] == fr[0, 1]), (i, s)
                assert nxt[s] is None or fi == nxt[s], (i, s, fi, nxt[s])
                nxt[s] = (fi + 1) & 0xFFFF
    assert all(n is not None for n in nxt)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 4. window wrap, reconfigure
def test_window_wrap_and_reconfigure(ctx):
    """rx_window = 1: the frame area holds one call's window (at most 3 + 1 slots), so a stream that delivers more than 4 frames
    has wrapped; sdrhip_rx_reconfigure to another nb_fec with a batch in flight: each batch reports its own blocks_per_frame"""
    import sdrdaemon_amd as sd

    S, L = 5, 1
    plan = [[2, 0, 3, 1, 1], [1, 3, 0, 2, 1], [3, 1, 1, 0, 2], [0, 2, 2, 3, 1], [1, 1, 3, 1, 0], [2, 0, 1, 2, 3]]
    fec = [8, 8, 8, 8, 1, 127]  # nb_fec each batch is submitted with (a fecblk change gives the windows a new area)
    ctx.set_option("rx_window", 1)
    try:
        a = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=fec[0])
        b = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=fec[0])
        a.set_async(depth=4)
        a.set_egress("round_robin")
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


# ------------------------------------------------------------------------------------------------ 5. contract
def test_contract(ctx):
    import sdrdaemon_amd as sd

    S, L, R = 3, 0, 1
    B = 128 + R
    a, b = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R), sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    lib = ctx.lib
    rs = np.random.RandomState(8)
    plans = iter([[1, 0, 2], [2, 1, 0], [0, 1, 1], [1, 1, 1], [1, 2, 1], [0, 0, 0], [2, 0, 1], [1, 0, 1], [0, 1, 0], [1, 1, 2]])
    n_sub = [0]

    def block():
        xs, counts = ragged_blocks(rs, S, L, next(plans), n_sub[0] == 0)
        if not sum(counts):  # (the batch with no frames still feeds a few samples)
            counts = [7, 0, 3]
            xs = rand_block(rs, counts)
        n_sub[0] += 1
        return np.concatenate(xs).reshape(-1), counts

    def both(x, counts):
        a.submit_ragged(x, counts, 9, n_sub[0])
        b.submit_ragged(x, counts, 9, n_sub[0])

    def code(fn, *args, **kw):
        with pytest.raises(sd.SdrHipError) as e:
            fn(*args, **kw)
        return e.value.code

    # ---- depth 2: two submits, collect the first, a third submit is SDRHIP_EBUSY until the loan is released
    a.set_async(depth=2)
    b.set_async(depth=2)
    assert code(a.set_egress, 7) == EINVAL  # (an unknown order: nothing changed, the next batches are in stream order ...)
    x, counts = block()
    both(x, counts)
    assert code(a.collect_egress) == EINVAL  # (... and a stream-order batch is not for collect_egress: it stays)
    e0 = b.collect_ragged()
    g0 = a.collect_ragged()
    assert all(np.array_equal(g, e) for g, e in zip(g0, e0))
    a.set_egress("round_robin")
    assert code(a.submit, np.zeros((S, 64, 2), np.int16)) == EINVAL  # (uniform batches have no order: nothing consumed)
    d0 = ctx.counter("d2h_bytes")
    x1, c1 = block()
    both(x1, c1)
    e1 = b.collect_ragged()
    assert ctx.counter("d2h_bytes") - d0 == 2 * sum(f.shape[0] for f in e1) * B * 512  # (one copy on each handle: exactly the frames)
    x2, c2 = block()
    both(x2, c2)
    e2 = b.collect_ragged()
    assert code(a.collect_ragged) == EINVAL  # (a mismatched collect: the batch stays ...)
    lent = a.collect_egress(copy=False)      # (... and is collected afterwards)
    same_as_twin(a, lent, e1, None, B, "lent")
    at = lent[0].ctypes.data
    snapshot = (lent[0].copy(), lent[1].copy())
    x3, c3 = block()
    assert code(a.submit_ragged, x3, c3, 9, 9) == EBUSY  # (one slot in flight, one lent)
    assert code(a.set_async, 2, 1) == EINVAL             # (the ring is busy)
    a.release_egress()
    a.release_egress()  # (nothing lent: SDRHIP_OK)
    a.submit_ragged(x3, c3, 9, n_sub[0])
    b.submit_ragged(x3, c3, 9, n_sub[0])
    e3 = b.collect_ragged()
    same_as_twin(a, a.collect_egress(), e2, None, B, "second")
    same_as_twin(a, a.collect_egress(), e3, None, B, "third")
    assert a.collect_egress(wait=False) is None

    # ---- depth 4: the lent bytes equal the copy taken at collect after two later batches have completed
    a.set_async(depth=4)
    b.set_async(depth=4)
    exp = []
    for _ in range(3):
        x, counts = block()  # [1, 2, 1], [0, 0, 0], [2, 0, 1]
        both(x, counts)
        exp.append(b.collect_ragged())
    lent = a.collect_egress(copy=False)
    snapshot = (lent[0].copy(), lent[1].copy())
    at = (lent[0].ctypes.data, lent[1].ctypes.data)
    ctx.synchronize()  # (the two later batches have completed)
    assert (lent[0].ctypes.data, lent[1].ctypes.data) == at
    assert np.array_equal(lent[0], snapshot[0]) and np.array_equal(lent[1], snapshot[1])
    same_as_twin(a, lent, exp[0], None, B, "lent 4")
    # a lent batch is not in flight for the synchronous entries ...
    none = a.collect_egress(copy=False)  # (a batch with no frames; it releases the first one implicitly)
    assert none[0].shape == (0, 512) and none[1].shape == (0,) and list(none[2]) == [0, 0, 0]
    last = a.collect_egress(copy=False)
    same_as_twin(a, last, exp[2], None, B, "last 4")
    xs, counts = ragged_blocks(rs, S, L, [1, 2, 0], False)  # (fed synchronously to both)
    rows = np.zeros((S, max(counts), 2), np.int16)
    for s in range(S):
        rows[s, :counts[s]] = xs[s]
    ga, na = a.process_ragged(rows, counts, 3, 4)
    gb, nb = b.process_ragged(rows, counts, 3, 4)
    assert list(na) == list(nb) == [1, 2, 0] and all(np.array_equal(ga[s, :na[s]], gb[s, :nb[s]]) for s in range(S))
    assert np.array_equal(last[0], rounds(exp[2])[0])  # (... and the loan outlives them)
    a.release_egress()

    # ---- a batch being filled refuses set_egress; with the order off again the stream-order collects give the twin's bytes
    a.set_async(depth=2, blocks=2)
    b.set_async(depth=2, blocks=2)
    x, counts = block()
    both(x, counts)
    assert code(a.set_egress, None) == EINVAL  # (the order stays on: this batch is delivered in departure order)
    x, counts = block()
    both(x, counts)
    same_as_twin(a, a.collect_egress(), b.collect_ragged(), None, B, "two blocks")
    a.set_egress(None)
    a.set_async(depth=2)
    b.set_async(depth=2)
    x, counts = block()
    both(x, counts)
    ea, eb = a.collect_ragged(), b.collect_ragged()
    assert [e.shape[0] for e in eb] == [1, 1, 2] and all(np.array_equal(g, e) for g, e in zip(ea, eb))
    nf = (C.c_size_t * S)()
    assert lib.sdrhip_rx_collect_egress(a.h, None, nf, 0, None, None, 1) == EINVAL  # (NULL out)
    assert mismatches(ctx) == 0
