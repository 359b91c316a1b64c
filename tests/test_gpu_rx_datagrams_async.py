"""Asynchronous datagram-fed Rx batches (sdrhip_rx_submit_datagrams / sdrhip_rx_collect_datagrams) against the yardsticks of the
synchronous entry: the hub chain of test_gpu_rx_datagrams (the reference's own SDRdaemonFECBuffer fed datagram by datagram, a
Python remainder buffer, the reference decimators, the oracle framer and frame_encode), the FEC buffer bank's records, and
sdrhip_rx_process_datagrams itself on a twin handle.  Bit-exact everywhere.  Every test also checks that the host's shadow of the
classification never disagreed with the device ("fecbuf_shadow_mismatch" stays 0)."""
import ctypes as C
import threading

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_rx_datagrams as tr
import test_gpu_tx_datagrams as tt
import test_gpu_tx_datagrams_async as ta
from test_gpu_rx_datagrams import HubChain, bank_calls, check_frames, prime, torch_first  # noqa: F401  (torch_first: fixture)

pytestmark = pytest.mark.gpu

F = 16129
EBUSY, EINVAL = -6, -1
ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)
reflib = tt.reflib


def mismatches(ctx):
    return ctx.counter("fecbuf_shadow_mismatch")


def stamps(i, S):
    return [1000 + 10 * i + s for s in range(S)], [37 * i + s for s in range(S)]


def as_np(batch):
    return [(np.asarray(fr), recs) for fr, recs in batch]


def run_async(rx, calls, depth=4, stamp=stamps, after_submit=None):
    """submits every batch with its stamps, collecting the oldest whenever the ring is full; -> per batch, per stream (frames, records)"""
    import sdrdaemon_amd as sd

    S = len(calls[0])
    rx.set_async(depth=depth)
    out = []
    for i, chunk in enumerate(calls):
        sec, usec = stamp(i, S)
        while True:
            try:
                rx.submit_datagrams(chunk, sec, usec)
                break
            except sd.SdrHipError as e:
                if e.code != EBUSY:
                    raise
                out.append(as_np(rx.collect_datagrams()))
        if after_submit:
            after_submit(i)
    while len(out) < len(calls):
        out.append(as_np(rx.collect_datagrams()))
    assert rx.collect_datagrams(wait=False) is None  # (nothing left: SDRHIP_EBUSY)
    return out


def with_an_empty_stream(calls, i, s):
    calls = [list(c) for c in calls]
    calls[i][s] = np.zeros((0, 512), np.uint8)
    return calls


_EXPECT = {}


def expected(oracle, reflib, L, fcpos, hb, R, calls):
    """the hub chain's frames per batch and stream, and the remainders after every batch; kept per case (both depths share it)"""
    key = (L, fcpos, hb, R)
    if key not in _EXPECT:
        S = len(calls[0])
        chains = [HubChain(reflib, oracle, hb) for _ in range(S)]
        x = None
        if L >= 3:  # (what prime feeds, here to the chains alone)
            n = (F - 300) << L
            x = np.random.RandomState(5).randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)
            for s, c in enumerate(chains):
                assert c.samples(x[s], L, fcpos, R, 999, 1) == []
        frames, rems = [], []
        for i, chunk in enumerate(calls):
            sec, usec = stamps(i, S)
            frames.append([chains[s].dgrams(chunk[s], L, fcpos, R, sec[s], usec[s]) for s in range(S)])
            rems.append([len(c.rem) for c in chains])
        _EXPECT[key] = (frames, rems)
    return _EXPECT[key]


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("hb", [0, 1])
@pytest.mark.parametrize("L,fcpos", tr.CASES)
def test_parity_with_the_reference_chain(oracle, ctx, reflib, L, fcpos, hb, depth):
    """8 streams, incoming fecblk 1 / 32 / 64 / 127 with random losses, 3-4 batches cut at random points, one stream of one batch
    empty; every decimation and position with both half-band variants, outgoing nb_fec 8 and 32 alternating over the cases; the
    records equal a FECBufferBank's, the carry after every submit is the chain's remainder after that batch"""
    import sdrdaemon_amd as sd

    S = 8
    R = 8 if (L + fcpos + hb) % 2 else 32
    calls = with_an_empty_stream(bank_calls(oracle, 300 + L % 2, ncalls=3 + L % 2), 1, 3)
    exp, rems = expected(oracle, reflib, L, fcpos, hb, R, calls)
    rx = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, hb_variant=hb, nb_fec=R)
    if L >= 3:
        n = (F - 300) << L
        x = np.random.RandomState(5).randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)
        assert not rx.process_ragged(x, [n] * S, 999, 1)[1].any()

    def carry_is_the_chains(i):
        assert list(rx.carry()) == rems[i], i

    got = run_async(rx, calls, depth, after_submit=carry_is_the_chains)
    bank = sd.FECBufferBank(ctx, S)
    total, held = 0, 0
    for i, chunk in enumerate(calls):
        ref = bank.write_and_read(chunk)
        for s in range(S):
            assert got[i][s][1] == ref[s][2], (i, s)
            check_frames(got[i][s][0], exp[i][s], (L, fcpos, hb, i, s))
            total += got[i][s][0].shape[0]
        held += sum(rems[i])
    assert total >= S and (held > 0 or L == 0)
    assert mismatches(ctx) == 0


def submit_raw(ctx, rx, chunk, sec, usec, strided, pinned, keep):
    """the C entry itself: packed or strided rows, pageable or sdrhip_host_alloc memory (kept in `keep` until collected)"""
    from sdrdaemon_amd._lib import check

    S = len(chunk)
    counts = [c.shape[0] for c in chunk]
    rows = max(counts + [1]) + 2 if strided else max(sum(counts), 1)  # (strided: two datagrams of padding per row)
    shape = (S, rows, 512) if strided else (rows, 512)
    buf = ctx.host_alloc(shape, np.uint8) if pinned else np.empty(shape, np.uint8)
    buf[...] = 0xA5
    if strided:
        for s, c in enumerate(chunk):
            buf[s, :counts[s]] = c
    elif sum(counts):
        buf[:sum(counts)] = np.concatenate([c for c in chunk if c.shape[0]])
    keep.append((buf, pinned))
    nd = (C.c_size_t * S)(*counts)
    sec = (C.c_uint32 * S)(*[int(v) for v in np.broadcast_to(sec, (S,))])
    usec = (C.c_uint32 * S)(*[int(v) for v in np.broadcast_to(usec, (S,))])
    check(ctx.lib.sdrhip_rx_submit_datagrams(rx.h, buf.ctypes.data, nd, rows * 512 if strided else 0, sec, usec))
    rx._dg_submitted()


@pytest.mark.parametrize("strided,pinned", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("L,fcpos,R", [(0, 2, 8), (1, 0, 32), (4, 2, 32)])
def test_equal_to_the_synchronous_call(oracle, ctx, L, fcpos, R, strided, pinned):
    """the same batches through sdrhip_rx_process_datagrams (host memory) on a twin handle: frames, records, carry() and the
    collector's statistics after every batch, byte for byte; packed and strided input, pageable and pinned in place.  At x16 the
    streams release frames in batches that complete none."""
    import sdrdaemon_amd as sd

    S = 8
    calls = with_an_empty_stream(bank_calls(oracle, 410 + L, ncalls=5), 2, 5)
    a = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, nb_fec=R)
    b = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, nb_fec=R)
    a.set_async(depth=2)
    if L >= 3:  # (as prime: every open frame 300 decimated samples from full, so that the few payloads complete frames)
        n = (F - 300) << L
        x = np.random.RandomState(5).randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)
        for p in (a, b):
            assert not p.process_ragged(x, [n] * S, 999, 1)[1].any()
    keep, nothing_completed, total = [], 0, 0
    for i, chunk in enumerate(calls):
        sec, usec = stamps(i, S)
        submit_raw(ctx, a, chunk, sec, usec, strided, pinned, keep)
        exp = b.process_datagrams(chunk, sec, usec)
        assert list(a.carry()) == list(b.carry()), i
        for s in range(S):
            assert a.collector_stats(s) == b.collector_stats(s), (i, s)
        got = a.collect_datagrams()
        for s in range(S):
            assert got[s][1] == exp[s][1], (i, s)
            assert got[s][0].shape == exp[s][0].shape and got[s][0].tobytes() == np.asarray(exp[s][0]).tobytes(), (i, s)
            nothing_completed += 1 if got[s][1] and not got[s][0].shape[0] else 0
            total += got[s][0].shape[0]
    for buf, pin in keep:
        if pin:
            ctx.host_free(buf)
    assert total >= 1 and (nothing_completed > 0 or L < 4)
    assert mismatches(ctx) == 0


@pytest.mark.parametrize("L,fcpos", [(1, 0), (3, 2), (6, 2)])
def test_cut_invariance(oracle, ctx, reflib, L, fcpos):
    """one datagram sequence per stream cut into 1, 3 and 7 batches: the same frames, the same carry at the end"""
    import sdrdaemon_amd as sd

    S = 4
    rs = np.random.RandomState(41 + L)
    per = [tt.stream_dgrams(oracle, rs, 4 + s % 2, [32, 64][s % 2], lose_rows=40 if s == 3 else 0) for s in range(S)]
    runs, carries = [], []
    for n in (1, 3, 7):
        rs = np.random.RandomState(7 * n)
        cut = [tt.split(rs, per[s], n) for s in range(S)]
        rx = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, nb_fec=8, sample_rate=0)
        if L >= 3:
            prime([rx], [HubChain(reflib, oracle, sample_rate=0) for _ in range(S)], L, fcpos, 8, 5, 6)
        got = run_async(rx, [[cut[s][i] for s in range(S)] for i in range(n)], 3, stamp=lambda i, S: (5, 6))
        runs.append([np.concatenate([g[s][0] for g in got]) for s in range(S)])
        carries.append(list(rx.carry()))
    for s in range(S):
        assert runs[0][s].shape[0] >= 1
        assert np.array_equal(runs[0][s], runs[1][s]) and np.array_equal(runs[0][s], runs[2][s]), s
    assert carries[0] == carries[1] == carries[2]
    assert mismatches(ctx) == 0


def test_mixed_with_synchronous_calls_reconfigure_and_reset(oracle, ctx, reflib):
    """synchronous datagram calls and sample-fed ragged calls before and after asynchronous runs, sdrhip_rx_reconfigure and a
    collector reset between collected batches: the streams continue exactly as the hub chain does"""
    import sdrdaemon_amd as sd

    S = 4
    calls = bank_calls(oracle, 302, S=S, ncalls=10, nframes=(16, 20))
    rs = np.random.RandomState(9)
    cfg = dict(L=3, fcpos=2, R=16)
    rx = sd.RxPipe(ctx, S, log2decim=3, fcpos=2, nb_fec=16)
    rx.set_async(depth=3)
    chains = [HubChain(reflib, oracle) for _ in range(S)]
    total = [0]

    def check(got, i, what):
        for s in range(S):
            check_frames(np.asarray(got[s][0]), chains[s].dgrams(calls[i][s], cfg["L"], cfg["fcpos"], cfg["R"], 20 + i, i), (what, i, s))
            total[0] += got[s][0].shape[0]

    def sync(i):
        check(tr.run_call(rx, calls[i], 20 + i, i, device=i % 2 == 0), i, "sync")
        assert list(rx.carry()) == [len(c.rem) for c in chains]

    def batches(ids):
        for i in ids:
            rx.submit_datagrams(calls[i], 20 + i, i)
        for i in ids:
            check(rx.collect_datagrams(), i, "async")
        assert list(rx.carry()) == [len(c.rem) for c in chains]

    def ragged(counts, sec):
        x = rs.randint(-32768, 32768, size=(S, max(counts), 2)).astype(np.int16)
        held = list(rx.carry())
        g, nf = rx.process_ragged(x, counts, sec, 1)
        for s in range(S):
            check_frames(g[s, :nf[s]], chains[s].samples(x[s, :counts[s]], cfg["L"], cfg["fcpos"], cfg["R"], sec, 1), ("ragged", sec, s))
        assert list(rx.carry()) == held

    def reconf(**kw):
        rx.reconfigure(**{dict(L="log2decim", R="nb_fec", fcpos="fcpos")[k]: v for k, v in kw.items()})
        cfg.update(kw)

    sync(0)
    batches([1, 2])
    ragged([(F << 3) // 2 + 3, 0, (F << 3) + 9, 17], 40)
    batches([3])
    reconf(L=5)
    batches([4])
    sync(5)
    ragged([5, (F << 5), 64, 0], 41)
    reconf(R=40)
    batches([6, 7])
    reconf(L=1, fcpos=0)
    batches([8])
    rx.reset_collector()
    assert list(rx.carry()) == [0] * S
    for c in chains:
        c.reset_collector()
    batches([9])
    assert total[0] >= S
    assert mismatches(ctx) == 0


def test_shadow_hostile_headers(oracle, ctx, reflib):
    """the twin of the Tx test, ending in frames: hostile headers and batch boundaries that fall anywhere; records equal the bank's,
    frames the hub chain's"""
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(11)
    st = ta.hostile_streams(oracle, rs)
    S = len(st)
    ncalls = 7
    per = [tt.split(rs, d, ncalls) for d in st]
    b1 = np.concatenate(per[1])
    per[1] = [b1[:100], b1[100:200], b1[200:240]] + tt.split(rs, list(b1[240:]), ncalls - 3)
    calls = [[per[s][i] for s in range(S)] for i in range(ncalls)]
    total = 0
    for L, R in ((0, 8), (3, 32)):
        rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
        chains = [HubChain(reflib, oracle) for _ in range(S)]
        if L:
            prime([rx], chains, L, 2, R, 999, 1)
        got = run_async(rx, calls, 2)
        bank = sd.FECBufferBank(ctx, S)
        for i, chunk in enumerate(calls):
            ref = bank.write_and_read(chunk)
            assert [len(g[1]) for g in got[i]] == bank.last_n_frames, i
            sec, usec = stamps(i, S)
            for s in range(S):
                assert got[i][s][1] == ref[s][2], (i, s)
                check_frames(got[i][s][0], chains[s].dgrams(chunk[s], L, 2, R, sec[s], usec[s]), (L, i, s))
                total += got[i][s][0].shape[0]
        assert list(rx.carry()) == [len(c.rem) for c in chains]
    flags = [r["flags"] for call in got for g in call for r in g[1]]
    assert any(f & 8 for f in flags) and any(f & 4 for f in flags)  # (a decode error and a repair happened)
    assert any(r["frame_index"] == 0 for call in got for r in call[3][1])  # (the wrap)
    assert total >= S
    assert mismatches(ctx) == 0


def test_decoder_bound_is_the_highest_row(oracle, ctx, reflib):
    """fecblk 64: recovery rows >= 32 among the first 128 with at most 32 recovery blocks per frame -- a bound taken from the count
    (<= 32) would send these frames to the one-launch decoder, which cannot restore rows >= 32"""
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(21)
    S = 6
    st = [tt.stream_dgrams(oracle, rs, 3, 64, lose_rows=32) for _ in range(S)]
    calls = [[c[i] for c in [tt.split(rs, d, 3) for d in st]] for i in range(3)]
    rx = sd.RxPipe(ctx, S, log2decim=1, nb_fec=8)
    chains = [HubChain(reflib, oracle) for _ in range(S)]
    got = run_async(rx, calls)
    recs = [r for call in got for g in call for r in g[1] if r["flags"] & 4]
    assert recs and all(r["recovery_count"] <= 32 for r in recs)
    total = 0
    for i, chunk in enumerate(calls):
        sec, usec = stamps(i, S)
        for s in range(S):
            check_frames(got[i][s][0], chains[s].dgrams(chunk[s], 1, 2, 8, sec[s], usec[s]), (i, s))
            total += got[i][s][0].shape[0]
    assert total >= S
    assert mismatches(ctx) == 0


@pytest.mark.parametrize("L,R", [(0, 8), (2, 32), (4, 32)])
def test_link_bytes(oracle, ctx, L, R):
    """H2D: exactly the datagrams; D2H: exactly the delivered frames and records"""
    import sdrdaemon_amd as sd

    calls = bank_calls(oracle, 500 + L, ncalls=4)
    rx = sd.RxPipe(ctx, 8, log2decim=L, nb_fec=R)
    rx.carry()
    rx._collector()  # (created on first use: its initial state goes up once)
    ctx.synchronize()
    for depth in (1, 4):
        per_batch = []
        rx.set_async(depth=depth)
        for i, chunk in enumerate(calls if depth == 1 else []):  # (depth 1: the deltas of every single batch)
            h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
            rx.submit_datagrams(chunk, i, 0)
            got = rx.collect_datagrams()
            up, down = ctx.counter("h2d_bytes") - h0, ctx.counter("d2h_bytes") - d0
            frames, recs = sum(g[0].shape[0] for g in got), sum(len(g[1]) for g in got)
            print("batch %d: h2d %d d2h %d frames %d records %d" % (i, up, down, frames, recs))
            assert up == sum(c.shape[0] for c in chunk) * 512
            assert down == frames * (128 + R) * 512 + recs * 16
            per_batch.append((frames, recs))
        if depth == 1:
            assert sum(r for _, r in per_batch) > 8
            continue
        h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        got = run_async(rx, calls, depth)
        up, down = ctx.counter("h2d_bytes") - h0, ctx.counter("d2h_bytes") - d0
        frames = sum(g[0].shape[0] for call in got for g in call)
        recs = sum(len(g[1]) for call in got for g in call)
        assert up == sum(c.shape[0] for call in calls for c in call) * 512
        assert recs > 8 and down == frames * (128 + R) * 512 + recs * 16
    assert mismatches(ctx) == 0


def test_contract(oracle, ctx, reflib):
    """EBUSY (nothing submitted, ring full, in flight with wait = 0); a collect without room keeps the batch and fills both count
    arrays; every refusal while datagram batches are in flight consumes nothing, and the reverse refusals"""
    import sdrdaemon_amd as sd
    from sdrdaemon_amd._lib import check

    S, L, R = 32, 1, 32
    rs = np.random.RandomState(31)
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    chains = [HubChain(reflib, oracle) for _ in range(S)]
    assert rx.collect_datagrams(wait=False) is None  # nothing submitted
    rx.set_async(depth=2)
    big = [np.asarray(tt.stream_dgrams(oracle, rs, 8, 32), np.uint8) for _ in range(S)]
    small = [tt.bank_calls(oracle, 600 + k, S=S, ncalls=1)[0] for k in range(3)]
    rx.submit_datagrams(big, 7, 8)
    # wait = 0 on a batch that is (in all likelihood) still in flight: no room offered, so that the batch stays either way --
    # SDRHIP_EBUSY while it runs, SDRHIP_EINVAL with its counts once it has finished
    nr0, nf0 = (C.c_size_t * S)(), (C.c_size_t * S)()
    rc = ctx.lib.sdrhip_rx_collect_datagrams(rx.h, None, 0, 0, 0, None, nr0, nf0, 0)
    assert rc in (EBUSY, EINVAL) and (list(nr0) == [0] * S if rc == EBUSY else list(nr0) == [9] * S)
    rx.submit_datagrams(small[0], 9, 10)
    held = list(rx.carry())
    with pytest.raises(sd.SdrHipError) as e:
        rx.submit_datagrams(small[1], 11, 12)  # ring full
    assert e.value.code == EBUSY
    # refusals with batches in flight: SDRHIP_EINVAL, nothing consumed
    fb = rx._collector()
    x = rs.randint(-32768, 32768, size=(S, 64, 2)).astype(np.int16)
    nd, nf = (C.c_size_t * S)(*[1] * S), (C.c_size_t * S)()
    one = np.zeros((S, 1, 512), np.uint8)
    pay = np.zeros((S, 127 * 508), np.uint8)
    info = (sd.engine.FECBufferFrame * S)()
    for call in (lambda: rx.submit(x), lambda: rx.collect(), lambda: rx.submit_ragged(x, [64] * S), lambda: rx.collect_ragged(),
                 lambda: rx.process(x), lambda: rx.process_ragged(x, [64] * S), lambda: rx.process_datagrams(small[1], 11, 12),
                 lambda: rx.set_input_format("s8"), lambda: rx.set_async(depth=4),
                 lambda: check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 1)), lambda: check(ctx.lib.sdrhip_fecbuf_reset(fb)),
                 lambda: check(ctx.lib.sdrhip_fecbuf_write_and_read(fb, one.ctypes.data, nd, 512, pay.ctypes.data, 127 * 508, None, 1, info, nf,
                                                                    sd.MEM_HOST))):
        with pytest.raises(sd.SdrHipError) as e:
            call()
        assert e.value.code == EINVAL
    assert list(rx.carry()) == held
    # bad arguments of the submit itself: refused as well
    st = (C.c_uint32 * S)()
    buf = np.zeros((S, 2, 512), np.uint8)
    two = (C.c_size_t * S)(*[2] * S)
    assert ctx.lib.sdrhip_rx_submit_datagrams(rx.h, buf.ctypes.data, None, 0, st, st) == EINVAL
    assert ctx.lib.sdrhip_rx_submit_datagrams(rx.h, buf.ctypes.data, two, 0, None, st) == EINVAL
    assert ctx.lib.sdrhip_rx_submit_datagrams(rx.h, buf.ctypes.data, two, 0, st, None) == EINVAL
    # too little room: the batch stays, both count arrays hold the counts
    exp_big = [chains[s].dgrams(big[s], L, 2, R, 7, 8) for s in range(S)]
    most = max(len(x) for x in exp_big)
    assert most >= 2
    for kw in (dict(max_frames=most - 1, max_released=9), dict(max_frames=most, max_released=8)):
        with pytest.raises(sd.SdrHipError) as e:
            rx.collect_datagrams(**kw)
        assert e.value.code == EINVAL and rx.last_n_released == [9] * S and rx.last_n_frames == [len(x) for x in exp_big]
    out = np.zeros((S, most, 128 + R, 512), np.uint8)
    info = (sd.engine.FECBufferFrame * (S * 9))()
    nr, nf = (C.c_size_t * S)(), (C.c_size_t * S)()
    fbytes = (128 + R) * 512
    assert ctx.lib.sdrhip_rx_collect_datagrams(rx.h, out.ctypes.data, most * fbytes - 512, most, 9, info, nr, nf, 1) == EINVAL  # stride
    assert list(nr) == [9] * S and list(nf) == [len(x) for x in exp_big]
    got = rx.collect_datagrams(max_frames=most, max_released=9)  # with room: collected
    for s in range(S):
        check_frames(np.asarray(got[s][0]), exp_big[s], ("big", s))
    got = rx.collect_datagrams()
    for s in range(S):
        check_frames(np.asarray(got[s][0]), chains[s].dgrams(small[0][s], L, 2, R, 9, 10), ("small0", s))
    assert rx.collect_datagrams(wait=False) is None
    # the reverse: a ragged batch being filled, a uniform batch in flight, pipelined mode
    rx.set_async(depth=2, blocks=2)
    xr = rs.randint(-32768, 32768, size=(S, 64 << L, 2)).astype(np.int16)
    rx.submit_ragged(xr, [64 << L] * S, 1, 2)
    with pytest.raises(sd.SdrHipError) as e:
        rx.submit_datagrams(small[1], 11, 12)
    assert e.value.code == EINVAL
    with pytest.raises(sd.SdrHipError) as e:
        rx.collect_datagrams()
    assert e.value.code == EINVAL
    batch = rx.collect_ragged(wait=True)
    for s in range(S):
        check_frames(batch[s], chains[s].samples(xr[s], L, 2, R, 1, 2), ("ragged batch", s))
    # (ragged calls left the streams at different frame positions: the uniform submit and pipelined mode refuse by themselves)
    # stride that is neither SDRHIP_PACKED nor >= the largest count x 512
    assert ctx.lib.sdrhip_rx_submit_datagrams(rx.h, buf.ctypes.data, two, 512, st, st) == EINVAL
    # nothing was consumed by any refusal: the next batches continue the hub chain
    rx.set_async(depth=2)
    for k in (1, 2):
        rx.submit_datagrams(small[k], 11 + k, 12)
    for k in (1, 2):
        got = rx.collect_datagrams()
        for s in range(S):
            check_frames(np.asarray(got[s][0]), chains[s].dgrams(small[k][s], L, 2, R, 11 + k, 12), ("small", k, s))
    assert list(rx.carry()) == [len(c.rem) for c in chains]
    assert mismatches(ctx) == 0


def test_pipelined_mode_and_uniform_batches_refuse_the_submit(oracle, ctx):
    """(while the streams still stand together) pipelined mode and a uniform batch in flight: SDRHIP_EINVAL, nothing consumed"""
    import sdrdaemon_amd as sd
    from sdrdaemon_amd._lib import check

    S = 4
    calls = bank_calls(oracle, 303, S=S, ncalls=2)
    rx, twin = sd.RxPipe(ctx, S, log2decim=2, nb_fec=8), sd.RxPipe(ctx, S, log2decim=2, nb_fec=8)
    check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 1))
    with pytest.raises(sd.SdrHipError) as e:
        rx.submit_datagrams(calls[0], 1, 2)
    assert e.value.code == EINVAL
    check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 0))
    x = np.random.RandomState(3).randint(-32768, 32768, size=(S, 4096, 2)).astype(np.int16)
    rx.set_async(depth=2, blocks=1)
    rx.submit(x, 5, 6)
    with pytest.raises(sd.SdrHipError) as e:
        rx.submit_datagrams(calls[0], 1, 2)
    assert e.value.code == EINVAL
    a = rx.collect()
    b = twin.process(x, 5, 6)
    assert np.array_equal(np.asarray(a), np.asarray(b))
    for i, chunk in enumerate(calls):
        rx.submit_datagrams(chunk, 1, i)
        got, exp = rx.collect_datagrams(), twin.process_datagrams(chunk, 1, i)
        for s in range(S):
            assert got[s][1] == exp[s][1] and np.array_equal(got[s][0], np.asarray(exp[s][0])), (i, s)
    assert mismatches(ctx) == 0


def test_two_threads_and_pinned_in_place(oracle, ctx, reflib):
    """a reader thread submits (packed sdrhip_host_alloc memory, uploaded in place), the main thread collects"""
    import sdrdaemon_amd as sd

    S, n, L, R = 8, 10, 2, 8
    calls = bank_calls(oracle, 800, S=S, ncalls=n, nframes=(8, 12))
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    rx.set_async(depth=3)
    pinned, bufs = [], []
    for call in calls:
        rows = sum(c.shape[0] for c in call)
        a = ctx.host_alloc((max(rows, 1), 512), np.uint8)
        pinned.append(a)
        a = a[:rows]
        if rows:
            a[:] = np.concatenate([c for c in call if c.shape[0]])
        bufs.append((a, [c.shape[0] for c in call]))
    got, err = [], []

    def reader():
        try:
            for i, b in enumerate(bufs):
                while True:
                    try:
                        rx.submit_datagrams(b, 50 + i, i)
                        break
                    except sd.SdrHipError as e:
                        if e.code != EBUSY:
                            raise
                        threading.Event().wait(0.0005)
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = threading.Thread(target=reader)
    th.start()
    while len(got) < n and not err:
        r = rx.collect_datagrams(wait=bool(len(got) % 2))  # (blocking and polling collects alternate)
        if r is None:
            threading.Event().wait(0.0005)
            continue
        got.append(as_np(r))
    th.join()
    assert not err, err
    for a in pinned:
        ctx.host_free(a)
    chains = [HubChain(reflib, oracle) for _ in range(S)]
    total = 0
    for i, chunk in enumerate(calls):
        for s in range(S):
            check_frames(got[i][s][0], chains[s].dgrams(chunk[s], L, 2, R, 50 + i, i), (i, s))
            total += got[i][s][0].shape[0]
    assert total >= S
    assert mismatches(ctx) == 0
