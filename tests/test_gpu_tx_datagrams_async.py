"""Asynchronous datagram-fed Tx batches (sdrhip_tx_submit_datagrams / sdrhip_tx_collect_datagrams) against the same yardsticks as
the synchronous call: the reference's own SDRdaemonFECBuffer fed datagram by datagram plus the oracle's interpolators
(test_gpu_tx_datagrams.RefChain), the FEC buffer bank's records and meta blocks, and sdrhip_tx_process_datagrams itself on a twin
handle.  Every test also checks that the host's shadow of the classification never disagreed with the device
("fecbuf_shadow_mismatch" stays 0)."""
import threading

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_tx_datagrams as tgd
from test_gpu_tx_datagrams import ctx, reflib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SPF = 16129
EBUSY, EINVAL = -6, -1


def submit_all(tx, calls, collected=None):
    """submits every batch, collecting the oldest whenever the ring is full; -> per batch, per stream (iq, block0, records)"""
    import sdrdaemon_amd as sd

    out = [] if collected is None else collected
    for chunk in calls:
        while True:
            try:
                tx.submit_datagrams(chunk)
                break
            except sd.SdrHipError as e:
                if e.code != EBUSY:
                    raise
                out.append(tx.collect_datagrams())
    return out


def run_async(tx, calls, depth=4):
    tx.set_async(depth)
    out = submit_all(tx, calls)
    while len(out) < len(calls):
        out.append(tx.collect_datagrams())
    assert tx.collect_datagrams(wait=False) is None  # (nothing left: SDRHIP_EBUSY)
    return out


def mismatches(ctx):
    return ctx.counter("fecbuf_shadow_mismatch")


def check_bank(ctx, got, calls):
    """records and meta blocks equal the FEC buffer bank's on the same datagrams; frame counts equal its read-back"""
    import sdrdaemon_amd as sd

    bank = sd.FECBufferBank(ctx, len(calls[0]))
    for i, chunk in enumerate(calls):
        ref = bank.write_and_read(chunk)
        for s in range(len(chunk)):
            assert got[i][s][2] == ref[s][2], (i, s)
            assert np.array_equal(got[i][s][1], ref[s][1]), (i, s)


def check_chain(got, chains, calls, log2interp):
    tgd.check_chain([[(g[0], g[1], g[2]) for g in call] for call in got], chains, calls, log2interp)


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("log2interp", [0, 1, 2, 4, 6])
def test_parity_with_the_reference_chain(oracle, ctx, reflib, log2interp, depth):
    """8 streams, ragged counts (some 0), frames that begin in one batch and end batches later, random losses of originals and
    recovery blocks, rows >= 32 on some streams; x2 runs K5, the others K5w"""
    import sdrdaemon_amd as sd

    calls = tgd.bank_calls(oracle, 300 + log2interp, ncalls=6)
    calls[2][3] = np.zeros((0, 512), np.uint8)
    assert any(c.shape[0] == 0 for call in calls for c in call)
    tx = sd.TxPipe(ctx, 8, log2interp)
    got = run_async(tx, calls, depth)
    assert any(len(got[i][s][2]) > 1 for i in range(len(calls)) for s in range(8))
    check_bank(ctx, got, calls)
    check_chain(got, [tgd.RefChain(reflib, oracle) for _ in range(8)], calls, log2interp)
    assert mismatches(ctx) == 0


@pytest.mark.parametrize("log2interp,fmt", [(0, "s16"), (0, "s8"), (1, "s16"), (4, "s8"), (5, "s16")])
def test_equal_to_the_synchronous_call(oracle, ctx, log2interp, fmt):
    """the same batches through sdrhip_tx_process_datagrams on a twin handle: samples, records, meta blocks and the collector's
    statistics afterwards byte for byte"""
    import sdrdaemon_amd as sd

    calls = tgd.bank_calls(oracle, 400 + log2interp, ncalls=5)
    a = sd.TxPipe(ctx, 8, log2interp, output_format=fmt)
    b = sd.TxPipe(ctx, 8, log2interp, output_format=fmt)
    got = run_async(a, calls, 3)
    for i, chunk in enumerate(calls):
        exp = b.process_datagrams(chunk)
        for s in range(8):
            assert got[i][s][0].dtype == exp[s][0].dtype == (np.int8 if fmt == "s8" else np.int16)
            assert got[i][s][0].tobytes() == exp[s][0].tobytes(), (i, s)
            assert np.array_equal(got[i][s][1], exp[s][1]) and got[i][s][2] == exp[s][2], (i, s)
    for s in range(8):
        assert a.collector_stats(s) == b.collector_stats(s), s
    assert mismatches(ctx) == 0


def hdr(fi, bi, rs):
    d = rs.randint(0, 256, 512).astype(np.uint8)
    d[0], d[1], d[2], d[3] = fi & 0xFF, (fi >> 8) & 0xFF, bi, 0
    return d


def hostile_streams(oracle, rs):
    """per stream a datagram list that stresses the classify rule"""
    fr = lambda n, R, fi0: tg.make_frames(oracle, rs, n, R, fi0)  # noqa: E731
    st = []
    # repeated originals among the first 128 with recovery blocks (cm256_decode refuses: delivered as received, the last copy
    # wins), then the same without recovery blocks among the first 128
    f = fr(2, 32, 10)
    st.append([f[0][i] for i in range(90)] + [f[0][5], f[0][7]] + [f[0][i] for i in range(128, 160)] + [f[0][i] for i in range(90, 100)]
              + [f[1][i] for i in range(100)] + [f[1][5], f[1][7]] + [f[1][i] for i in range(100, 160)])
    # more than 128 arrivals, the recovery rows late (none among the first 128), then again with losses in front of them
    f = fr(3, 40, 200)
    st.append(list(f[0]) + list(f[0][128:]) + [f[1][i] for i in range(168) if i not in (3, 9, 77)] + list(f[2][:3]))
    # a frame index repeated but not adjacent (A, B, A), and one-datagram frames
    f = fr(3, 16, 300)
    st.append(list(f[0][:130]) + list(f[1][:144]) + list(f[0][:50]) + [f[2][0]] + [hdr(301, 4, rs)] + [hdr(302, 9, rs)] + list(f[2][:20]))
    # frame index wrap 65535 -> 0
    f = fr(4, 32, 65534)
    st.append([f[k][i] for k in range(4) for i in range(160) if (i * 7 + k) % 11])
    # single datagrams only
    st.append([hdr(1000 + k, k % 200, rs) for k in range(40)])
    # late recovery rows >= 32 among the first 128 of a frame that has 128 + 64 blocks
    f = fr(3, 64, 4000)
    st.append([b for k in range(3) for i, b in enumerate(f[k]) if not (i < 20 or 128 <= i < 128 + 44)])
    return st


def test_shadow_hostile_headers(oracle, ctx, reflib):
    """the host's shadow gives the frame counts the bank's read-back gives, through hostile headers and batch boundaries that fall
    anywhere (a frame index equal to the carried head at a boundary continues the frame); outputs equal the reference chain"""
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(11)
    st = hostile_streams(oracle, rs)
    S = len(st)
    ncalls = 7
    per = [tgd.split(rs, d, ncalls) for d in st]
    # stream 1: a boundary inside the late recovery rows, so that the next batch starts with the carried frame index
    b1 = np.concatenate(per[1])
    per[1] = [b1[:100], b1[100:200], b1[200:240]] + tgd.split(rs, list(b1[240:]), ncalls - 3)
    calls = [[per[s][i] for s in range(S)] for i in range(ncalls)]
    for L in (0, 3):
        tx = sd.TxPipe(ctx, S, L)
        got = run_async(tx, calls, 2)
        bank = sd.FECBufferBank(ctx, S)
        for i, chunk in enumerate(calls):
            ref = bank.write_and_read(chunk)
            assert [len(g[2]) for g in got[i]] == bank.last_n_frames, i
            for s in range(S):
                assert got[i][s][2] == ref[s][2], (i, s)
        check_chain(got, [tgd.RefChain(reflib, oracle) for _ in range(S)], calls, L)
    flags = [r["flags"] for call in got for g in call for r in g[2]]
    assert any(f & 8 for f in flags) and any(f & 4 for f in flags)  # (a decode error and a repair happened)
    assert any(r["frame_index"] == 0 for call in got for r in call[3][2])  # (the wrap)
    assert mismatches(ctx) == 0


def test_decoder_bound_is_the_highest_row(oracle, ctx, reflib):
    """fecblk 64: recovery rows >= 32 among the first 128 with at most 32 recovery blocks per frame -- a bound taken from the count
    (<= 32) would send these frames to the one-launch decoder, which cannot restore rows >= 32"""
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(21)
    S = 6
    st = [tgd.stream_dgrams(oracle, rs, 3, 64, lose_rows=32) for _ in range(S)]
    calls = [[c[i] for c in [tgd.split(rs, d, 3) for d in st]] for i in range(3)]
    tx = sd.TxPipe(ctx, S, 0)
    got = run_async(tx, calls)
    recs = [r for call in got for g in call for r in g[2] if r["flags"] & 4]
    assert recs and all(r["recovery_count"] <= 32 for r in recs)
    check_bank(ctx, got, calls)
    check_chain(got, [tgd.RefChain(reflib, oracle) for _ in range(S)], calls, 0)
    assert mismatches(ctx) == 0


@pytest.mark.parametrize("log2interp,fmt", [(0, "s16"), (2, "s16"), (4, "s8")])
def test_link_bytes(oracle, ctx, log2interp, fmt):
    """H2D: exactly the datagrams; D2H: exactly the delivered samples, records and meta blocks"""
    import sdrdaemon_amd as sd

    calls = tgd.bank_calls(oracle, 500 + log2interp, ncalls=4)
    tx = sd.TxPipe(ctx, 8, log2interp, output_format=fmt)
    tx.set_async(4)
    collector(ctx, tx)  # (created on first use: its initial state goes up once)
    h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
    got = run_async(tx, calls, 4)
    h1, d1 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
    esz = 2 if fmt == "s8" else 4
    assert h1 - h0 == sum(c.shape[0] for call in calls for c in call) * 512
    frames = sum(len(g[2]) for call in got for g in call)
    assert frames > 8
    assert d1 - d0 == frames * ((SPF << log2interp) * esz + 16 + 508)
    assert mismatches(ctx) == 0


def test_contract(oracle, ctx, reflib):
    """EBUSY (nothing submitted, ring full, in flight with wait = 0); a collect without room keeps the batch; every refusal while
    datagram batches are in flight consumes nothing, and the reverse refusals"""
    import sdrdaemon_amd as sd
    from sdrdaemon_amd._lib import check

    S = 32
    rs = np.random.RandomState(31)
    tx = sd.TxPipe(ctx, S, 4)
    chains = [tgd.RefChain(reflib, oracle) for _ in range(S)]
    assert tx.collect_datagrams(wait=False) is None  # nothing submitted
    tx.set_async(2)
    big = [np.asarray(tgd.stream_dgrams(oracle, rs, 8, 32), np.uint8) for _ in range(S)]
    small = [tgd.bank_calls(oracle, 600 + k, S=S, ncalls=1)[0] for k in range(3)]
    tx.submit_datagrams(big)
    assert tx.collect_datagrams(wait=False) is None  # (~0.3 GB to interpolate and download: still in flight)
    tx.submit_datagrams(small[0])
    with pytest.raises(sd.SdrHipError) as e:
        tx.submit_datagrams(small[1])  # ring full
    assert e.value.code == EBUSY
    # refusals with batches in flight: SDRHIP_EINVAL, nothing consumed
    fb = collector(ctx, tx)
    frames = np.stack([np.stack(tg.make_frames(oracle, rs, 1, 0, s)) for s in range(S)])
    for call in (lambda: tx.submit(frames), lambda: tx.collect(), lambda: tx.process(frames),
                 lambda: tx.process_datagrams(small[1]), lambda: tx.set_output_format("s8"), lambda: tx.set_async(4),
                 lambda: check(ctx.lib.sdrhip_tx_set_pipelined(tx.h, 1)), lambda: check(ctx.lib.sdrhip_fecbuf_reset(fb))):
        with pytest.raises(sd.SdrHipError) as e:
            call()
        assert e.value.code == EINVAL
    # too little room: the batch stays, n_frames holds the counts
    with pytest.raises(sd.SdrHipError) as e:
        tx.collect_datagrams(max_frames=3)
    assert e.value.code == EINVAL and tx.last_n_frames == [9] * S
    got = [tx.collect_datagrams(max_frames=9)]
    got.append(tx.collect_datagrams())
    check_chain(got, chains, [big, small[0]], 4)
    # the reverse: a batch of received frames in flight, a pipelined batch waiting
    tx.submit(frames)
    with pytest.raises(sd.SdrHipError) as e:
        tx.submit_datagrams(small[1])
    assert e.value.code == EINVAL
    fx = tx.collect()
    for s in range(S):
        assert np.array_equal(fx[s], chains[s].interpolate([frames[s][0][1:128, 4:].reshape(-1)], 4)), s
    check(ctx.lib.sdrhip_tx_set_pipelined(tx.h, 1))
    with pytest.raises(sd.SdrHipError) as e:
        tx.submit_datagrams(small[1])
    assert e.value.code == EINVAL
    check(ctx.lib.sdrhip_tx_set_pipelined(tx.h, 0))
    # nothing was consumed by any refusal: the next batches continue the reference chain
    got = run_async(tx, [small[1], small[2]], 2)
    check_chain(got, chains, [small[1], small[2]], 4)
    assert mismatches(ctx) == 0


def collector(ctx, tx):
    import ctypes as C

    from sdrdaemon_amd._lib import check

    h = C.c_void_p()
    check(ctx.lib.sdrhip_tx_collector(tx.h, C.byref(h)))
    return h


def test_sync_calls_around_an_async_run_and_reconfigure(oracle, ctx, reflib):
    """synchronous datagram calls before and after a run of batches continue the same streams (the collector's state is read back
    once after them); sdrhip_tx_reconfigure between submits applies to the later batches only; sdrhip_fecbuf_stats in between"""
    import sdrdaemon_amd as sd

    S = 5
    calls = tgd.bank_calls(oracle, 700, S=S, ncalls=8)
    plan = [("sync", 2), ("async", 2), ("async", 3), ("sync", 3), ("async", 0), ("async", 5), ("sync", 1), ("async", 4)]
    tx = sd.TxPipe(ctx, S, 2)
    chains = [tgd.RefChain(reflib, oracle) for _ in range(S)]
    tx.set_async(4)
    got, pend = [None] * len(plan), []
    for i, (kind, L) in enumerate(plan):
        assert tx.configure({"interp": L})
        if kind == "sync":
            while pend:
                got[pend.pop(0)] = tx.collect_datagrams()
            got[i] = tx.process_datagrams(calls[i])
        else:
            tx.submit_datagrams(calls[i])
            pend.append(i)
            if i == 2:  # (two batches in flight: the statistics after both)
                bank = sd.FECBufferBank(ctx, S)
                for c in calls[:3]:
                    bank.write_and_read(c)
                assert [tx.collector_stats(s) for s in range(S)] == [bank.stats(s) for s in range(S)]
    while pend:
        got[pend.pop(0)] = tx.collect_datagrams()
    for i, (kind, L) in enumerate(plan):
        for s in range(S):
            exp = chains[s].feed(calls[i][s], L)
            assert np.array_equal(got[i][s][0], exp), (i, s)
    assert mismatches(ctx) == 0


def test_two_threads_and_pinned_in_place(oracle, ctx, reflib):
    """a reader thread submits (packed sdrhip_host_alloc memory, uploaded in place), the main thread collects"""
    import sdrdaemon_amd as sd

    S, n = 8, 10
    calls = tgd.bank_calls(oracle, 800, S=S, ncalls=n)
    tx = sd.TxPipe(ctx, S, 3)
    tx.set_async(3)
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
            for b in bufs:
                while True:
                    try:
                        tx.submit_datagrams(b)
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
        r = tx.collect_datagrams(wait=False)
        if r is None:
            threading.Event().wait(0.0005)
            continue
        got.append(r)
    th.join()
    assert not err, err
    for a in pinned:
        ctx.host_free(a)
    check_chain(got, [tgd.RefChain(reflib, oracle) for _ in range(S)], calls, 3)
    assert mismatches(ctx) == 0
