"""Per-stream reset (sdrhip_*_reset_streams): one stream of a bank begins again while the others run on.

The model of a reset stream is a FRESH reference object -- oracle decimators / interpolators, the collector model of
test_gpu_fecbuf, the hub and Tx chains of test_gpu_rx_datagrams / test_gpu_tx_datagrams (the reference's SDRdaemonFECBuffer, the
compiled-reference decimators, the oracle framer and encoder) -- fed what the stream gets after the reset; the model of every other
stream is the same object fed without interruption.  Nothing is compared against the library's own output.  Everything is byte-exact.

Shapes: a few thousand samples per call for the banks; F = 16129 decimated samples per frame, so the pipes run at decimate4 /
decimate2 with calls of one to two frames."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_rx_datagrams as tr
import test_gpu_rx_follow_meta as tf
import test_gpu_tx_datagrams as tt

pytestmark = pytest.mark.gpu

F = 16129
ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)
reflib = tt.reflib
EMPTY = np.zeros((0, 512), np.uint8)


@pytest.fixture(autouse=True, scope="module")
def torch_first():
    """torch brings its device runtime up before the reference's FEC buffer library is first used (as test_gpu_rx_datagrams)"""
    import torch

    torch.zeros(1).cuda()


def iq(seed, S, n):
    return np.random.RandomState(seed).randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)


MASKS = ["zero", "middle", "ones", "null"]


def apply_mask(kind, S, by_list, by_null):
    """resets the streams of the mask `kind` through the Python surface (NULL: the C entry itself); -> the set of streams reset"""
    if kind == "null":
        by_null()
        return set(range(S))
    streams = {"zero": [], "middle": [S // 2], "ones": list(range(S))}[kind]
    by_list(streams)
    return set(streams)


# ------------------------------------------------------------------------------------------------ banks: call A, reset, call B
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("S", [1, 3, 65])
def test_decimators(oracle, ctx, S, mask):
    import sdrdaemon_amd as sd

    xa, xb = iq(1, S, 3000 + 16), iq(2, S, 2048 + 37)
    for bias in (sd.HB_EO1, sd.HB_DB):
        for L, fcpos in ((4, sd.FC_CEN), (4, sd.FC_INF), (1, sd.FC_SUP)):
            d = sd.Decimators(ctx, S, bias)
            ya, _ = d.decimate(L, fcpos, 16, xa)
            hit = apply_mask(mask, S, lambda st: d.reset(streams=st),
                             lambda: sd.engine.check(ctx.lib.sdrhip_decimators_reset_streams(d.h, None)))
            yb, ssb = d.decimate(L, fcpos, 16, xb)
            for s in range(S):
                od = oracle.decimators(bias)
                ea, _ = od.decimate(L, fcpos, 16, xa[s])
                assert np.array_equal(ya[s], ea), (bias, L, fcpos, s, "A")
                if s in hit:
                    od = oracle.decimators(bias)
                eb, es = od.decimate(L, fcpos, 16, xb[s])
                assert es == ssb and np.array_equal(yb[s], eb), (bias, L, fcpos, s, s in hit)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("S", [1, 3, 65])
def test_interpolators(oracle, ctx, S, mask):
    import sdrdaemon_amd as sd

    xa, xb = iq(3, S, 300), iq(4, S, 257)
    for L in (2, 6):
        p = sd.Interpolators(ctx, S)
        ya = p.interpolate(L, xa)
        hit = apply_mask(mask, S, lambda st: p.reset(streams=st),
                         lambda: sd.engine.check(ctx.lib.sdrhip_interpolators_reset_streams(p.h, None)))
        yb = p.interpolate(L, xb)
        for s in range(S):
            oi = oracle.interpolators()
            assert np.array_equal(ya[s], oi.interpolate(L, xa[s])), (L, s, "A")
            if s in hit:
                oi = oracle.interpolators()
            assert np.array_equal(yb[s], oi.interpolate(L, xb[s])), (L, s, s in hit)


@pytest.mark.parametrize("calls_before", [1, 2])
def test_both_halves_of_the_double_buffer_read_as_reset(oracle, ctx, calls_before):
    """after the reset a ragged call feeds the reset stream nothing (it "keeps its history as it was", copied from whichever half
    is current: one or two calls before the reset put either half there), then a call feeds it: fresh-state output"""
    import sdrdaemon_amd as sd

    S, L = 3, 4
    d = sd.Decimators(ctx, S, sd.HB_EO1)
    ods = [oracle.decimators(0) for _ in range(S)]
    for k in range(calls_before):
        x = iq(10 + k, S, 4096)
        y, _ = d.decimate(L, sd.FC_CEN, 16, x)
        for s in range(S):
            assert np.array_equal(y[s], ods[s].decimate(L, sd.FC_CEN, 16, x[s])[0])
    d.reset(streams=[1])
    ods[1] = oracle.decimators(0)
    xc = iq(20, S, 2048)
    yc, _, _ = d.decimate_ragged(L, sd.FC_CEN, 16, xc, [2048, 0, 1024 + 16])
    xd = iq(21, S, 2048 + 48)
    yd, _ = d.decimate(L, sd.FC_CEN, 16, xd)
    for s, n in enumerate([2048, 0, 1024 + 16]):
        if n:
            assert np.array_equal(np.asarray(yc[s])[:n >> L], ods[s].decimate(L, sd.FC_CEN, 16, xc[s, :n])[0]), s
        assert np.array_equal(yd[s], ods[s].decimate(L, sd.FC_CEN, 16, xd[s])[0]), s


def test_matrix_core_path_after_a_partial_reset(oracle, ctx):
    """stage0_int16 is bank-wide: an inf call and a centred call shorter than the history leave rotate-sums in m_decimator2's history
    of every stream; a partial reset must not make the bank believe that history fits int16 again.  The next call is forced onto the
    matrix cores at the smallest size test_gpu_decim_mfma uses (span 1024)."""
    import sdrdaemon_amd as sd

    S, L = 3, 4
    d = sd.Decimators(ctx, S, sd.HB_EO1)
    ods = [oracle.decimators(0) for _ in range(S)]
    for (l, fcpos, n, seed) in ((3, sd.FC_INF, 4096, 30), (L, sd.FC_CEN, 32, 31)):
        x = iq(seed, S, n)
        y, _ = d.decimate(l, fcpos, 16, x)
        for s in range(S):
            assert np.array_equal(y[s], ods[s].decimate(l, fcpos, 16, x[s])[0]), (l, s)
    d.reset(streams=[1])
    ods[1] = oracle.decimators(0)
    ctx.set_option("decim_path", "mfma")
    ctx.set_option("mfma_span", 1024)
    try:
        x = iq(32, S, 200001)
        y, _ = d.decimate(L, sd.FC_CEN, 16, x)
        assert d.last_plan()["path"] == "mfma"
    finally:
        ctx.set_option("decim_path", "auto")
        ctx.set_option("mfma_span", 0)
    for s in range(S):
        e = ods[s].decimate(L, sd.FC_CEN, 16, x[s])[0]
        assert np.array_equal(y[s], e), (s, np.argwhere(np.asarray(y[s]) != e)[:4])


# ------------------------------------------------------------------------------------------------ FEC buffer bank
@pytest.mark.parametrize("arrivals", [140, 50])
def test_fecbuf_bank(oracle, ctx, arrivals):
    """three streams, stream 1 reset in mid-frame after more / fewer than 128 arrivals of its open frame"""
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(arrivals)
    R = 32
    per = []
    for s in range(3):
        dg = []
        for fr in tg.make_frames(oracle, rs, 4, R, 100 * s + 7):
            dg += tg.lossy(rs, list(fr), 5)
        per.append(dg + [np.full(512, 0xEE, np.uint8)])
    n1 = 155 + arrivals  # (155 datagrams per frame: one whole frame, then `arrivals` of the next)
    bank = sd.FECBufferBank(ctx, 3)
    first = tg.run_bank(bank, [p[:n1] for p in per], [100, n1 - 100])
    bank.reset(streams=[1])
    st = bank.stats(1)
    assert (st["cur_nb_blocks"], st["cur_nb_recovery"], st["min_nb_blocks"], st["max_nb_recovery"]) == (0, 0, 256, 0)
    assert st["current_meta"][:20] == tg.INIT_META and st["output_meta"][:20] == tg.INIT_META
    rest = tg.run_bank(bank, [p[n1:] for p in per], [7, 300, 400])
    cut = tg.Model(oracle).run(per[1][:n1])
    assert first[1][2] == cut.recs and all(np.array_equal(a, b) for a, b in zip(first[1][0], cut.frames))
    fresh = tg.Model(oracle).run(per[1][n1:])
    assert rest[1][2][0]["frame_index"] == -1 and rest[1][2][0]["block_count"] == 0 and not rest[1][0][0].any()
    got = [tuple(a + b for a, b in zip(first[s], rest[s])) for s in range(3)]
    got[1] = rest[1]
    tg.check_against_model(bank, got, [tg.Model(oracle).run(per[0]), fresh, tg.Model(oracle).run(per[2])])


# ------------------------------------------------------------------------------------------------ Rx pipe, sample-fed
def frame_index(frame):
    return int(frame[1, 0]) | (int(frame[1, 1]) << 8)


class RxModel:
    """per stream a HubChain; restart(s) = a new sdrdaemonrx process for stream s"""

    def __init__(self, lib, oracle, S, L, fcpos, R):
        self.new = lambda: tr.HubChain(lib, oracle)
        self.ch = [self.new() for _ in range(S)]
        self.L, self.fcpos, self.R = L, fcpos, R

    def restart(self, s):
        self.ch[s] = self.new()

    def samples(self, x, counts, sec, usec):
        return [c.samples(x[s, :counts[s]], self.L, self.fcpos, self.R, sec, usec) for s, c in enumerate(self.ch)]

    def dgrams(self, chunk, sec, usec):
        return [c.dgrams(chunk[s], self.L, self.fcpos, self.R, sec, usec) for s, c in enumerate(self.ch)]


def check_streams(frames, counts, exp, where):
    assert [int(c) for c in counts] == [len(e) for e in exp], (where, list(counts), [len(e) for e in exp])
    for s, e in enumerate(exp):
        tr.check_frames(np.asarray(frames[s])[:len(e)], e, (where, s))


@pytest.mark.parametrize("R", [0, 8])
@pytest.mark.parametrize("entry", ["process", "process_ragged"])
def test_rx_pipe_samples(oracle, ctx, reflib, entry, R):
    """a reset in mid-frame: the reset stream's frames start again at m_frameCount 0 and its open frame is never delivered (the
    fresh chain has no such frame); sdrhip_rx_process takes the ragged step afterwards; pipelined mode and uniform batches keep
    refusing an unaligned bank"""
    import sdrdaemon_amd as sd

    S, L = 3, 2
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    m = RxModel(reflib, oracle, S, L, sd.FC_CEN, R)
    f = F << L
    plan = [[3 * f // 2] * S, [6 * f // 5] * S, [f] * S] if entry == "process" else [[3 * f // 2, 7 * f // 10, 11 * f // 5 + 3],
                                                                                    [4 * f // 5, 13 * f // 10, 0], [f // 2, f, f // 3]]
    seen = []
    for k, counts in enumerate(plan):
        x = iq(40 + k, S, max(counts))
        if entry == "process":
            out = rx.process(x, 100 + k, 7)
            nf = [v.shape[0] for v in rx.frames_view_ragged()] if k else [out.shape[1]] * S
        else:
            out, nf = rx.process_ragged(x, counts, 100 + k, 7)
        exp = m.samples(x, counts, 100 + k, 7)
        check_streams(out, nf, exp, (entry, R, k))
        seen.append([frame_index(e[0]) if e else None for e in exp])
        if k == 0:
            rx.reset_streams([1])
            m.restart(1)
            with pytest.raises(sd.SdrHipError):
                sd.engine.check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 1))
            with pytest.raises(sd.SdrHipError):
                rx.submit(x[:, :64])
    # stream 1 counts from 0 again behind the reset -- the frame it had open (uniform calls: with index 1) is never delivered --,
    # stream 0 goes on
    assert seen[1][1] == 0 and seen[1][0] == 1 and (entry != "process" or seen[0][1] == 0), seen


def test_rx_pipe_null_mask_is_the_whole_pipe_reset(oracle, ctx, reflib):
    import sdrdaemon_amd as sd

    S, L, R = 3, 2, 8
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    m = RxModel(reflib, oracle, S, L, sd.FC_CEN, R)
    n = (3 * F // 2) << L
    for k in range(2):
        x = iq(50 + k, S, n)
        out = rx.process(x, k, 0)
        check_streams(out, [out.shape[1]] * S, m.samples(x, [n] * S, k, 0), k)
        rx.reset_streams()
        for s in range(S):
            m.restart(s)
    sd.engine.check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 1))  # (every stream stands at the same position again)


def test_rx_pipe_whole_reset_after_the_windows_moved_apart(oracle, ctx, reflib):
    """a partial reset, then ragged calls that complete 3 / 0 / 1 and 2 / 0 / 0 frames (every stream's window slides by its own
    count), then the whole-pipe reset: every stream stands where a fresh handle's stands, so uniform batches and pipelined mode are
    accepted again and the uniform step's output is that of fresh chains"""
    import sdrdaemon_amd as sd

    S, L, R = 3, 2, 8
    f = F << L
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    m = RxModel(reflib, oracle, S, L, sd.FC_CEN, R)
    x = iq(55, S, 3 * f // 2)
    out = rx.process(x, 1, 2)
    check_streams(out, [out.shape[1]] * S, m.samples(x, [3 * f // 2] * S, 1, 2), "uniform")
    rx.reset_streams([1])
    m.restart(1)
    done = []
    for k, counts in enumerate([[16 * f // 5, 2 * f // 5, 11 * f // 10], [21 * f // 10, 0, 3 * f // 10]]):
        x = iq(56 + k, S, max(counts))
        out, nf = rx.process_ragged(x, counts, 10 + k, 3)
        check_streams(out, nf, m.samples(x, counts, 10 + k, 3), ("ragged", k))
        done.append([int(v) for v in nf])
    assert done == [[3, 0, 1], [2, 0, 0]], done
    with pytest.raises(sd.SdrHipError):
        sd.engine.check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 1))
    rx.reset_streams()
    for s in range(S):
        m.restart(s)
    x = iq(58, S, 3 * f // 2)
    rx.submit(x, 20, 4)  # (a uniform batch: refused while the streams stand apart)
    got = rx.collect()
    check_streams(got, [got.shape[1]] * S, m.samples(x, [3 * f // 2] * S, 20, 4), "batch")
    assert got.shape[1] == 1
    sd.engine.check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 1))
    rx.pipelined = True
    x = iq(59, S, f)
    assert rx.process(x, 21, 4).shape[1] == 0  # (pipelined: this call's frames come with the next call, or the flush)
    got = rx.flush()
    exp = m.samples(x, [f] * S, 21, 4)
    assert [len(e) for e in exp] == [1] * S and frame_index(exp[0][0]) == 1
    check_streams(got, [got.shape[1]] * S, exp, "pipelined")


def test_rx_pipe_guards(oracle, ctx, reflib):
    """EINVAL while a uniform batch is being filled and while pipelined frames wait; the calls that follow show nothing changed"""
    import sdrdaemon_amd as sd

    S, L, R = 3, 2, 8
    n = (3 * F // 4) << L
    xs = [iq(60 + k, S, n) for k in range(4)]
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    m = RxModel(reflib, oracle, S, L, sd.FC_CEN, R)
    rx.set_async(depth=2, blocks=2)
    rx.submit(xs[0], 5, 6)
    with pytest.raises(sd.SdrHipError) as e:
        rx.reset_streams([1])
    assert e.value.code == -1 and "being filled" in str(e.value)
    rx.submit(xs[1], 0, 0)
    got = rx.collect()
    exp = m.samples(np.concatenate([xs[0], xs[1]], axis=1), [2 * n] * S, 5, 6)
    check_streams(got, [got.shape[1]] * S, exp, "batch")
    assert got.shape[1] == 1

    rp = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R, pipelined=True)
    mp = RxModel(reflib, oracle, S, L, sd.FC_CEN, R)
    exp = []
    for k in range(2):
        assert rp.process(xs[k], k, 1).shape[1] == 0
        exp.append(mp.samples(xs[k], [n] * S, k, 1))
    assert [len(e) for e in exp[1]] == [1] * S
    with pytest.raises(sd.SdrHipError) as e:
        rp.reset_streams([0])
    assert e.value.code == -1 and "flush" in str(e.value)
    with pytest.raises(sd.SdrHipError):
        rp.reset_streams()
    got = rp.flush()
    check_streams(got, [got.shape[1]] * S, exp[1], "flush")
    rp.reset_streams([0])  # (nothing waits any more)
    mp.restart(0)
    with pytest.raises(sd.SdrHipError):  # (an unaligned bank needs the ragged step, which is not pipelined: nothing consumed)
        rp.process(xs[2], 9, 1)
    sd.engine.check(ctx.lib.sdrhip_rx_set_pipelined(rp.h, 0))
    rp.pipelined = False
    out = rp.process(xs[2], 9, 1)
    exp = mp.samples(xs[2], [n] * S, 9, 1)
    assert [len(e) for e in exp] == [0, 1, 1]
    check_streams(out, [v.shape[0] for v in rp.frames_view_ragged()], exp, "after")


# ------------------------------------------------------------------------------------------------ Rx pipe, datagram-fed
def follow_streams(oracle, seed, S, nframes):
    """per stream: nframes incoming frames with a real meta block (centre frequency and rate distinct per stream, fecblk 4), a few
    blocks other than block 0 lost; -> per stream the list of per-frame datagram lists"""
    rs = np.random.RandomState(seed)
    per = []
    for s in range(S):
        frames = tf.incoming(oracle, rs, [(900000 + s, 2000000 + 2 * s)] * nframes, 4, int(rs.randint(0, 65536)))
        per.append([[f[i] for i in range(132) if i not in set((1 + rs.choice(131, 3, replace=False)).tolist())] for f in frames])
    return per


def dgram_calls(per, cuts):
    """cuts: (frame, datagrams into it) positions; -> per call, per stream an (n, 512) array"""
    out = []
    for dgs in per:
        flat = np.asarray([d for f in dgs for d in f], np.uint8).reshape(-1, 512)
        starts = np.cumsum([0] + [len(f) for f in dgs])
        b = [0] + [int(starts[k]) + off for k, off in cuts] + [flat.shape[0]]
        out.append([flat[b[i]:b[i + 1]] for i in range(len(b) - 1)])
    return [[c[i] for c in out] for i in range(len(cuts) + 1)]


def dgram_model(oracle, reflib, S, L, R):
    """the reference side of test_rx_pipe_datagrams (no GPU): per call and stream (frames, the two meta words each must carry)"""
    per = follow_streams(oracle, 70 + R, S, 10)
    calls = dgram_calls(per, [(2, 60), (3, 20)])
    host = [(tf.CFG_FC, tf.CFG_RATE)] * S
    chains = [tf.FollowChain(reflib, oracle, host[s]) for s in range(S)]
    models = [tg.Model(oracle) for _ in range(S)]
    exp = []
    for i, chunk in enumerate(calls):
        if i == 1:  # (the reset: a new process for stream 1)
            chains[1], models[1] = tf.FollowChain(reflib, oracle, host[1]), tg.Model(oracle)
        row = []
        for s in range(S):
            models[s].run(chunk[s])
            row.append(chains[s].call(chunk[s], L, 2, R, 200 + i, 11 * s, tf.rule(models[s].out_meta, L, host[s])))
        exp.append(row)
        if i == 0:
            assert [len(c.rem) for c in chains] == [3] * S and all(c.pending > 0 for c in chains)  # (a carry and an open frame to lose)
    # what the case is about: behind the reset stream 1 counts its frames from 0 again, the first of them opened under the host's
    # values (no incoming meta yet), a later one under the incoming values; the others never fall back to the host's
    after = [(f, w) for i in (1, 2) for f, w in zip(*exp[i][1])]
    assert len(after) >= 2 and frame_index(after[0][0]) == 0 and after[0][1] == host[1] and after[-1][1] == (900001, 2000002 >> L)
    assert all(w == (900000, 2000000 >> L) for i in range(3) for w in exp[i][0][1]) and sum(len(exp[i][0][0]) for i in range(3)) >= 2
    return exp, chains, models, host, calls


@pytest.mark.parametrize("R", [0, 8])
@pytest.mark.parametrize("entry", ["process_datagrams", "submit_datagrams"])
def test_rx_pipe_datagrams(oracle, ctx, reflib, entry, R):
    """follow-meta on.  Call 0 ends 60 datagrams into incoming frame 2 (an open collector slot, a carry of 3, an open outgoing frame),
    then stream 1 is reset; call 1 brings the rest of frame 2 (its block 0 came before the reset) and the head of frame 3: the fresh
    collector releases the zero initial slot and the headless frame 2, neither with a meta block, so the frames stream 1 opens in
    call 1 announce the HOST's values; call 2 releases frames with block 0 and the incoming values are back.  The asynchronous entry
    gets the reset between two submits with nothing collected."""
    import sdrdaemon_amd as sd

    S, L = 3, 2
    exp, chains, models, host, calls = dgram_model(oracle, reflib, S, L, R)
    rx, host_rx = tf.make_bank(ctx, S, log2decim=L, nb_fec=R)
    assert host_rx == host
    got = []
    for i, chunk in enumerate(calls):
        if entry == "process_datagrams":
            got.append(tr.run_call(rx, chunk, 200 + i, [11 * s for s in range(S)], device=i % 2 == 0))
        else:
            rx.submit_datagrams(chunk, 200 + i, [11 * s for s in range(S)])
        if i == 0:
            assert list(rx.carry()) == [3] * S
            rx.reset_streams([1])
            assert list(rx.carry()) == [3, 0, 3]
    if entry == "submit_datagrams":
        got = [rx.collect_datagrams() for _ in calls]
        assert rx.collect_datagrams(wait=False) is None
    assert list(rx.carry()) == [len(c.rem) for c in chains]
    for i in range(len(calls)):
        for s in range(S):
            frames, ew = exp[i][s]
            tr.check_frames(got[i][s][0], frames, (entry, R, i, s))
            for k, w in enumerate(ew):
                assert tf.meta_of(got[i][s][0][k])[:2] == w and tf.crc_ok(got[i][s][0][k]), (i, s, k)
    for s in range(S):
        assert rx.collector_stats(s)["output_meta"][:20] == models[s].out_meta, s
    assert got[1][1][1][0]["frame_index"] == -1 and got[1][1][1][0]["block_count"] == 0  # (the zero initial slot)
    if entry == "submit_datagrams":
        v = C.c_uint64()
        assert ctx.lib.sdrhip_ctx_get_counter(ctx.h, b"fecbuf_shadow_mismatch", C.byref(v)) == 0 and v.value == 0


# ------------------------------------------------------------------------------------------------ Tx pipe
def test_tx_pipe_process(oracle, ctx):
    import sdrdaemon_amd as sd

    S, L = 3, 2
    rs = np.random.RandomState(80)
    tx = sd.TxPipe(ctx, S, L)
    ois = [oracle.interpolators() for _ in range(S)]
    for k in range(3):
        fr = np.stack([np.stack(tg.make_frames(oracle, rs, 1, 0, k)) for _ in range(S)])
        out = tx.process(fr)
        for s in range(S):
            pay = np.ascontiguousarray(fr[s, :, 1:, 4:]).view(np.int16).reshape(-1, 2)
            assert np.array_equal(out[s], ois[s].interpolate(L, pay)), (k, s)
        if k == 0:
            tx.reset_streams([1])
            ois[1] = oracle.interpolators()
        if k == 1:
            tx.reset_streams()
            ois = [oracle.interpolators() for _ in range(S)]


@pytest.mark.parametrize("entry", ["process_datagrams", "submit_datagrams"])
def test_tx_pipe_datagrams(oracle, ctx, reflib, entry):
    """interpolate4, a reset of stream 1 in mid-frame (between two submits with nothing collected for the asynchronous entry)"""
    import sdrdaemon_amd as sd

    S, L = 3, 2
    rs = np.random.RandomState(81)
    per = [tt.stream_dgrams(oracle, rs, 4, 32) for _ in range(S)]
    calls = [[np.asarray(p[:200], np.uint8).reshape(-1, 512) for p in per], [np.asarray(p[200:], np.uint8).reshape(-1, 512) for p in per]]
    tx = sd.TxPipe(ctx, S, L)
    chains = [tt.RefChain(reflib, oracle) for _ in range(S)]
    got = []
    for i, chunk in enumerate(calls):
        if entry == "process_datagrams":
            got += tt.run_calls(tx, [chunk], device=i == 0)
        else:
            tx.submit_datagrams(chunk)
        if i == 0:
            tx.reset_streams([1])
    if entry == "submit_datagrams":
        got = [[(tt.as_np(a), tt.as_np(b), r) for a, b, r in tx.collect_datagrams()] for _ in calls]
    exp0 = [c.feed(calls[0][s], L) for s, c in enumerate(chains)]
    chains[1] = tt.RefChain(reflib, oracle)
    exp1 = [c.feed(calls[1][s], L) for s, c in enumerate(chains)]
    for i, exp in enumerate((exp0, exp1)):
        for s in range(S):
            assert got[i][s][0].shape == exp[s].shape and np.array_equal(got[i][s][0], exp[s]), (entry, i, s)
    assert got[1][1][2][0]["frame_index"] == -1 and exp1[1].shape[0] > (F << L)
    st = tx.collector_stats(1)
    assert st["min_nb_blocks"] <= 160 and tx.collector_stats(0)["max_nb_recovery"] >= 1
