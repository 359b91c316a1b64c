"""Per-stream sample size (sdrhip_rx_set_stream_bits / sdrhip_rx_get_stream_bits / sdrhip_decimate_ragged_bits).  The yardsticks are
the compiled reference decimators (else the oracle) asked per stream at that stream's size, and S one-stream twins,
sd.RxPipe(ctx, 1, sample_bits=bits[s], ...), fed stream s's input with its stamps; every comparison is byte equality.  The departure
order of the twins' frames is the literal simulation of the rounds of tests/test_gpu_rx_egress.py."""
import struct
import zlib

import numpy as np
import pytest

import test_gpu_rx_follow_meta as tf
from test_gpu_rx_egress import PLAN, ctx, dgram_calls, merge, mismatches, ragged_blocks, rounds, stamps, torch_first  # noqa: F401  (fixtures)
from test_gpu_rx_stream_fec import code, rows_of

pytestmark = pytest.mark.gpu

F = 16129
EBUSY, EINVAL = -6, -1
BITS = [8, 12, 16, 10, 13]      # RTL-SDR / HackRF, Airspy / BladeRF, the test source, and two sizes either side of decimate16's 12
HUB_FEC = [0, 1, 32, 127, 4]    # the egress cases' counts of tests/test_gpu_rx_stream_fec.py


def frame_bits(L, b):
    """the size Decimators::decimateN returns (Decimators.cpp:43-44 ...): grows by L, capped at 16"""
    return b if L == 0 else min(b + L, 16)


def yardstick(oracle):
    from oracle_lib import Reference

    return Reference("eo1").decimators() if Reference.available("eo1") else oracle.decimators()


class Twins:
    """S one-stream pipes, stream s with its own sample_bits (and, where given, fecblk, centre frequency and rate)"""

    def __init__(self, ctx, bits, fec=None, fc=None, rate=None, **cfg):
        import sdrdaemon_amd as sd

        self.p = []
        for s, b in enumerate(bits):
            kw = dict(cfg, sample_bits=b)
            if fec is not None:
                kw["nb_fec"] = fec[s]
            if fc is not None:
                kw["center_frequency_khz"] = fc[s]
            if rate is not None:
                kw["sample_rate"] = rate[s]
            self.p.append(sd.RxPipe(ctx, 1, **kw))

    def ragged(self, x, counts, secs, usecs):
        return [p.process(np.ascontiguousarray(x[s][:counts[s]]), int(secs[s]), int(usecs[s])) for s, p in enumerate(self.p)]

    def datagrams(self, chunk, secs, usecs):
        return [p.process_datagrams([chunk[s]], int(secs[s]), int(usecs[s]))[0] for s, p in enumerate(self.p)]

    def reconfigure(self, bits=None, **kw):
        for s, p in enumerate(self.p):
            p.reconfigure(**(dict(kw, sample_bits=bits[s]) if bits is not None else kw))


def per_stream(got, nf):
    """process_ragged's delivery as a list of each stream's frames (the fecblk array set: it is one already)"""
    return got if isinstance(got, list) else [got[s, :nf[s]] for s in range(len(nf))]


def same(got, exp, where):
    assert len(got) == len(exp), where
    for s, (g, e) in enumerate(zip(got, exp)):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape, (where, s, g.shape, e.shape)
        assert g.tobytes() == e.tobytes(), (where, s)


def bytes_8_9(fr):
    """(sampleBytes, sampleBits) of a frame's meta block (block 0: a 4-byte header, then MetaDataFEC)"""
    return int(fr[0, 4 + 8]), int(fr[0, 4 + 9])


def says(frames, L, bits, where):
    """every frame of every stream says its stream's decimated size, under a CRC that holds"""
    for s, g in enumerate(frames):
        fb = frame_bits(L, bits[s])
        for f, fr in enumerate(np.asarray(g)):
            meta = fr[0, 4:28].tobytes()
            assert bytes_8_9(fr) == ((fb - 1) // 8 + 1, fb), (where, s, f, bytes_8_9(fr), fb)
            assert struct.unpack("<I", meta[20:24])[0] == zlib.crc32(meta[:20]), (where, s, f)


# ------------------------------------------------------------------------------------------------ 1. the decimator bank, every kernel
DEC_CASES = [(L, 2, "valu") for L in range(7)] + [(L, fc, "valu") for L in (1, 2, 3, 5) for fc in (0, 1)] + [(L, 2, "mfma") for L in range(2, 7)]


@pytest.mark.parametrize("L,fc,path", DEC_CASES)
def test_decimator_bank_per_stream_sizes(ctx, oracle, L, fc, path):
    """decimate_ragged with a size per stream against Reference.decimators().decimate(L, fc, bits[s], x) per stream, the returned
    sizes included.  Sizes: 16-L-1, 16-L, 16-L+1 (the norm / trunk crossover) beside 8, 12 and 16.  Two calls (state carries over);
    counts with 0, one below 2^L, streams long enough for matrix-core wave groups (mfma: span 64 << L) and one on pieces alone.
    Even streams get full-scale int16 input (the truncation wraps), odd ones amplitudes within their size"""
    import sdrdaemon_amd as sd

    u, sp = 1 << L, 64 << L
    sizes = [min(max(b, 1), 16) for b in (16 - L - 1, 16 - L, 16 - L + 1)] + [8, 12, 16]
    S = len(sizes)
    A, B, m = 40 * sp + 3 * u + 1, 23 * sp + u, 3 * sp + 5  # (m: shorter than head + 8 spans -- no wave group, pieces alone)
    calls = [[A, B, m, u - 1, 0, A + u + 3], [B, m, A, A, B, 0]]
    ctx.set_option("decim_path", path)
    ctx.set_option("mfma_span", sp if path == "mfma" else 0)
    try:
        bank = sd.Decimators(ctx, S)
        refs = [yardstick(oracle) for _ in range(S)]
        rs = np.random.RandomState(31 * L + fc)
        for k, counts in enumerate(calls):
            x = np.zeros((S, max(counts), 2), np.int16)
            for s in range(S):
                hi = 32768 if s % 2 == 0 else 1 << (sizes[s] - 1)
                x[s, :counts[s]] = rs.randint(-hi, hi, size=(counts[s], 2))
            out, n_out, new = bank.decimate_ragged(L, fc, sizes, x, counts)
            assert list(n_out) == [c >> L for c in counts], k
            for s in range(S):
                # (the by-reference size of a call that decimates nothing: asked of a fresh object -- the reference's loop bound wraps at n < 2^L)
                exp_size = yardstick(oracle).decimate(L, fc, sizes[s], np.zeros((4 * u, 2), np.int16))[1]
                assert new[s] == exp_size == frame_bits(L, sizes[s]), (k, s, new[s], exp_size)
                if counts[s] >= u:
                    y, ss = refs[s].decimate(L, fc, sizes[s], np.ascontiguousarray(x[s, :counts[s]]))
                    assert ss == new[s] and y.shape[0] == n_out[s], (k, s)
                    assert np.array_equal(np.asarray(out[s, :n_out[s]]), y), (k, s, sizes[s])
            plan = bank.last_plan()
            cascade = L >= 1 and (fc == 2 or L >= 3)
            if path == "mfma":
                assert plan["path"] == "mfma" and plan["wps"] > 0, (k, plan)
            else:
                assert plan["path"] == ("valu" if cascade else None), (k, plan)
        # a scalar size calls the bank-wide entry as before: one size back, and the samples of an array of equal entries
        x = rs.randint(-32768, 32768, size=(S, 70 * u + 1, 2)).astype(np.int16)
        cnt = [70 * u + 1 - s for s in range(S)]
        o1, n1, s1 = sd.Decimators(ctx, S).decimate_ragged(L, fc, 12, x, cnt)
        o2, n2, s2 = sd.Decimators(ctx, S).decimate_ragged(L, fc, [12] * S, x, cnt)
        assert isinstance(s1, int) and s1 == frame_bits(L, 12) and s2 == [s1] * S and list(n1) == list(n2)
        for s in range(S):
            assert np.array_equal(np.asarray(o1[s, :n1[s]]), np.asarray(o2[s, :n2[s]])), s
    finally:
        ctx.set_option("decim_path", "auto")
        ctx.set_option("mfma_span", 0)


# ------------------------------------------------------------------------------------------------ 2. reference chain
@pytest.mark.parametrize("L", [0, 4])
def test_reference_chain(ctx, oracle, L):
    """per stream: the reference decimators at bits[s], the oracle framer with sample_bytes / sample_bits from the decimator's
    returned size, frame_encode.  Bytes 8, 9 and the CRC explicitly; every stream completes a frame or more per call over 3 calls"""
    import sdrdaemon_amd as sd

    bits, R = BITS, 8
    S = len(bits)
    bank = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, sample_bits=16, nb_fec=R, center_frequency_khz=435000, sample_rate=625000)
    bank.set_stream_bits(bits)
    for s in range(S):
        assert bank.stream_bits(s) == (bits[s], frame_bits(L, bits[s]))
    decs = [yardstick(oracle) for _ in range(S)]
    framers = [None] * S
    rs = np.random.RandomState(10 + L)
    total = 0
    for k in range(3):
        counts = [((F + 11 * s + 5 * k + 1) << L) + (s % 2) * L for s in range(S)]
        x = rs.randint(-32768, 32768, size=(S, max(counts), 2)).astype(np.int16)
        secs, usecs = [1000 + 10 * k + s for s in range(S)], [37 * k + s for s in range(S)]
        got, nf = bank.process_ragged(x, counts, secs, usecs)
        assert min(nf) >= 1, (k, list(nf))
        for s in range(S):
            y, ss = decs[s].decimate(L, sd.FC_CEN, bits[s], np.ascontiguousarray(x[s, :counts[s]]))
            assert ss == frame_bits(L, bits[s])
            if framers[s] is None:
                framers[s] = oracle.framer(nb_fec_blocks=R, sample_bytes=(ss - 1) // 8 + 1, sample_bits=ss)
            framers[s].s.tv_sec, framers[s].s.tv_usec = secs[s], usecs[s]
            exp = framers[s].write(y)
            assert nf[s] == exp.shape[0], (k, s)
            for f in range(exp.shape[0]):
                fr = np.asarray(got[s, f])
                meta = fr[0, 4:28].tobytes()
                assert (meta[8], meta[9]) == ((ss - 1) // 8 + 1, ss), (k, s, f)
                assert struct.unpack("<I", meta[20:24])[0] == zlib.crc32(meta[:20]) == oracle.crc32(meta[:20]), (k, s, f)
                assert np.array_equal(fr[:128], exp[f]), (k, s, f)
                assert np.array_equal(fr[128:], oracle.frame_encode(exp[f], R)), (k, s, f)
                total += 1
    assert total >= 3 * S


# ------------------------------------------------------------------------------------------------ 3. process_ragged against twins
STORIES = {
    "decimate2_cen": dict(L=1, fc=2, L2=2, opts={}),
    "decimate8_inf": dict(L=3, fc=0, L2=4, opts={}),
    "decimate16_cen_valu": dict(L=4, fc=2, L2=3, opts={"decim_path": "valu"}),
    "decimate16_cen_mfma_direct": dict(L=4, fc=2, L2=3, opts={"decim_path": "mfma", "mfma_span": 1024, "rx_direct": "1"}),
    "decimate16_cen_mfma_k2r": dict(L=4, fc=2, L2=3, opts={"decim_path": "mfma", "mfma_span": 1024, "rx_direct": "0"}),
}
RESTORE = {"decim_path": "auto", "mfma_span": 0, "rx_direct": "1", "rx_window": 0}


@pytest.mark.parametrize("story", sorted(STORIES))
def test_twins_process_ragged(ctx, story):
    """unequal counts; rx_window = 1, so the windows pass the area's end every few calls; the zero-copy view after call 1; stream 1
    idle in call 2; the array changed in front of call 3 with every frame open (the open frame keeps bytes 8 and 9 it was opened
    with, the samples take the new shift at once); stream 3 reset in front of call 4 (the array stays); reconfigure(log2decim)
    in front of call 5 (stream_bits reports the new frame_bits); NULL in front of call 6"""
    import sdrdaemon_amd as sd

    c = STORIES[story]
    L, fc = c["L"], c["fc"]
    bits0, bits1 = BITS, [12, 16, 8, 13, 9]
    S = len(bits0)
    plan = [[2, 1, 3, 1, 2], [1, 2, 1, 2, 1], [2, 0, 1, 1, 2], [2, 2, 2, 2, 2], [2, 2, 1, 1, 1], [1, 2, 2, 1, 2], [1, 1, 1, 2, 1]]
    for k, v in dict(c["opts"], rx_window=1).items():
        ctx.set_option(k, v)
    try:
        cfg = dict(log2decim=L, fcpos=fc, nb_fec=8)
        bank, twins = sd.RxPipe(ctx, S, sample_bits=14, **cfg), Twins(ctx, bits0, **cfg)
        bank.set_stream_bits(bits0)
        bits = bits0
        rs = np.random.RandomState(2 + L)
        for k, frames in enumerate(plan):
            if k == 3:
                bank.set_stream_bits(bits1)
                twins.reconfigure(bits1)
                prev, bits = bits, bits1
            if k == 4:
                bank.reset_streams([3])
                twins.p[3].reset_streams()
                assert bank.stream_bits(3) == (bits[3], frame_bits(L, bits[3]))
            if k == 5:
                bank.reconfigure(log2decim=c["L2"])
                twins.reconfigure(log2decim=c["L2"])
                L = c["L2"]
                assert [bank.stream_bits(s) for s in range(S)] == [(b, frame_bits(L, b)) for b in bits]
            if k == 6:
                bank.set_stream_bits(None)
                twins.reconfigure([14] * S)
                bits = [14] * S
                assert bank.stream_bits(0) == (14, frame_bits(L, 14))
            xs, counts = ragged_blocks(rs, S, L, frames, k == 0)  # (k = 0 leaves every stream's frame open from then on)
            if k == 2:
                counts[1], xs[1] = 0, xs[1][:0]
            secs, usecs = stamps(k, S)
            got, nf = bank.process_ragged(rows_of(xs, counts), counts, secs, usecs)
            exp = twins.ragged(xs, counts, secs, usecs)
            got = per_stream(got, nf)
            same(got, exp, (story, k))
            assert list(nf) == [e.shape[0] for e in exp]
            if k == 1:
                same([v.cpu().numpy() for v in bank.frames_view_ragged()], exp, (story, "view"))
            if k == 3:  # the frame that was open across the change says the old size, the next one the new
                for s in range(S):
                    assert bytes_8_9(np.asarray(got[s][0]))[1] == frame_bits(L, prev[s]), (story, s)
                    assert bytes_8_9(np.asarray(got[s][1]))[1] == frame_bits(L, bits[s]), (story, s)
            elif k in (0, 1, 2):
                says(got, L, bits, (story, k))
            if "mfma" in story and k < 5:
                assert bank.last_plan()["path"] == "mfma" and bank.last_plan()["wps"] > 0, (k, bank.last_plan())
            if "valu" in story:
                assert bank.last_plan()["path"] == "valu", (k, bank.last_plan())
    finally:
        for k in dict(c["opts"], rx_window=1):
            ctx.set_option(k, RESTORE[k])


# ------------------------------------------------------------------------------------------------ 4. the other entries
@pytest.mark.parametrize("follow", [False, True], ids=["follow_off", "follow_on"])
def test_twins_process_datagrams(oracle, ctx, follow):
    """the datagram entry.  follow off: PLAN's batches (a stream fed nothing in some calls, 0 .. 3 frames released) at L = 0 and 1.
    follow on: incoming frames with real meta blocks (the eight sender kinds of tests/test_gpu_rx_follow_meta.py); KF's CRC is
    formed over each stream's own third word, the size stays the stream's own (rule 5).  Frames, records, carry and collector
    statistics equal the twins' after every call"""
    import sdrdaemon_amd as sd

    for L in ((0,) if follow else (0, 1)):
        calls = tf.follow_calls(oracle, 31, L, 3, 3) if follow else dgram_calls(oracle)
        S = len(calls[0])
        bits = (BITS + [9, 16, 8])[:S]
        cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
        bank, twins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, bits, **cfg)
        bank.set_stream_bits(bits)
        if follow:
            bank.set_follow_meta(True)
            for p in twins.p:
                p.set_follow_meta(True)
        total = 0
        for i, chunk in enumerate(calls):
            secs, usecs = stamps(i, S)
            got = bank.process_datagrams(chunk, secs, usecs)
            exp = twins.datagrams(chunk, secs, usecs)
            same([g for g, _ in got], [e for e, _ in exp], ("dg", follow, L, i))
            says([g for g, _ in got], L, bits, ("dg", follow, L, i))
            assert [r for _, r in got] == [r for _, r in exp], i
            assert list(bank.carry()) == [int(p.carry()[0]) for p in twins.p], i
            for s in range(S):
                assert bank.collector_stats(s) == twins.p[s].collector_stats(0), (i, s)
            total += sum(np.asarray(g).shape[0] for g, _ in got)
        assert total >= S
    assert mismatches(ctx) == 0


@pytest.mark.parametrize("L,tagged,depth", [(0, False, 1), (1, True, 4), (1, False, 4), (0, True, 1)])
def test_stream_order_datagram_batches(oracle, ctx, L, tagged, depth):
    """submit_datagrams / _tagged and collect_datagrams at depth 1 and 4: frames and records equal the twins'; carry and collector
    statistics equal the twins' after every batch"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S = len(calls[0])
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    a, twins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, BITS, **cfg)
    a.set_stream_bits(BITS)
    a.set_async(depth=depth)
    got, exp = [], []
    for i, chunk in enumerate(calls):
        secs, usecs = stamps(i, S)
        while True:
            try:
                if tagged:
                    arr, tags = merge(chunk, 60 + i, skip=3)
                    a.submit_datagrams_tagged(arr, tags, secs, usecs)
                else:
                    a.submit_datagrams(chunk, secs, usecs)
                break
            except sd.SdrHipError as e:
                assert e.code == EBUSY
                got.append(a.collect_datagrams())
        exp.append(twins.datagrams(chunk, secs, usecs))
        assert list(a.carry()) == [int(p.carry()[0]) for p in twins.p], i
        for s in range(S):
            assert a.collector_stats(s) == twins.p[s].collector_stats(0), (i, s)
    while len(got) < len(calls):
        got.append(a.collect_datagrams())
    for i, (g, e) in enumerate(zip(got, exp)):
        same([f for f, _ in g], [f for f, _ in e], (L, tagged, i))
        says([f for f, _ in g], L, BITS, (L, tagged, i))
        assert [r for _, r in g] == [r for _, r in e], i
    assert mismatches(ctx) == 0


def test_stream_order_ragged_batches(ctx):
    """submit_ragged / collect_ragged, two blocks per batch: the twins fed the batch's summed counts"""
    import sdrdaemon_amd as sd

    L, S = 1, 5
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    a, twins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, BITS, **cfg)
    a.set_stream_bits(BITS)
    a.set_async(depth=2, blocks=2)
    rs = np.random.RandomState(9)
    for i in range(0, len(PLAN), 2):
        blocks = [ragged_blocks(rs, S, L, PLAN[i + j], i + j == 0) for j in (0, 1)]
        for xs, counts in blocks:
            a.submit_ragged(np.concatenate(xs).reshape(-1), counts, 100 + i, i)
        both = [np.concatenate([blocks[0][0][s], blocks[1][0][s]]) for s in range(S)]
        tot = [blocks[0][1][s] + blocks[1][1][s] for s in range(S)]
        exp = twins.ragged(both, tot, [100 + i] * S, [i] * S)
        got = a.collect_ragged()
        same(got, exp, ("ragged batch", i))
        says(got, L, BITS, ("ragged batch", i))
    assert a.collect_ragged(wait=False) is None


def twin_rounds(exp):
    return rounds([np.asarray(e) for e in exp])


@pytest.mark.parametrize("L,tagged,depth", [(0, False, 1), (1, True, 4)])
def test_egress_with_differing_fecblk(oracle, ctx, L, tagged, depth):
    """set_stream_bits together with set_stream_fec [0, 1, 32, 127, 4] and set_egress: array, tags, n_frames, last_stream_blocks
    and records equal rounds() over the twins' frames; d2h_bytes per batch exact; carry and statistics as the twins'"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S = len(calls[0])
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, BITS, fec=HUB_FEC, **cfg)
    a.set_stream_fec(HUB_FEC)
    a.set_stream_bits(BITS)
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
    for i, e in enumerate(exp):
        dg, tags, nf, records = got[i]
        e_dg, e_tags = twin_rounds([fr for fr, _ in e])
        assert list(nf) == [np.asarray(fr).shape[0] for fr, _ in e], i
        assert dg.shape == e_dg.shape and np.array_equal(tags, e_tags) and dg.tobytes() == e_dg.tobytes(), i
        assert records == [r for _, r in e], i
        assert down[i] == sum(int(nf[s]) * (128 + HUB_FEC[s]) * 512 for s in range(S)) + sum(len(r) for _, r in e) * 16, i
    assert mismatches(ctx) == 0


def test_egress_ragged_batches_with_differing_fecblk(ctx):
    """sample-fed batches, two blocks per batch, with both arrays and set_egress: the rounds over the twins fed the batch's summed
    counts; the download is exactly the datagrams"""
    import sdrdaemon_amd as sd

    L, S = 1, 5
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a, twins = sd.RxPipe(ctx, S, nb_fec=8, **cfg), Twins(ctx, BITS, fec=HUB_FEC, **cfg)
    a.set_stream_fec(HUB_FEC)
    a.set_stream_bits(BITS)
    a.set_async(depth=2, blocks=2)
    a.set_egress("round_robin")
    rs = np.random.RandomState(19)
    for i in range(0, len(PLAN), 2):
        blocks = [ragged_blocks(rs, S, L, PLAN[i + j], i + j == 0) for j in (0, 1)]
        d0 = ctx.counter("d2h_bytes")
        for xs, counts in blocks:
            a.submit_ragged(np.concatenate(xs).reshape(-1), counts, 100 + i, i)
        down = ctx.counter("d2h_bytes") - d0
        both = [np.concatenate([blocks[0][0][s], blocks[1][0][s]]) for s in range(S)]
        tot = [blocks[0][1][s] + blocks[1][1][s] for s in range(S)]
        exp = twins.ragged(both, tot, [100 + i] * S, [i] * S)
        dg, tags, nf, records = a.collect_egress()
        e_dg, e_tags = twin_rounds(exp)
        assert list(nf) == [np.asarray(e).shape[0] for e in exp], i
        assert dg.shape == e_dg.shape and np.array_equal(tags, e_tags) and dg.tobytes() == e_dg.tobytes(), i
        assert records is None and down == dg.shape[0] * 512, i
    assert a.collect_egress(wait=False) is None


# ------------------------------------------------------------------------------------------------ 5. all three arrays at once
def test_meta_fec_and_bits_together(oracle, ctx):
    """set_stream_meta, set_stream_fec and set_stream_bits on one bank against twins configured with all three: process_ragged, then
    a departure-order datagram batch"""
    import sdrdaemon_amd as sd

    L, S = 1, 5
    fcs, rates = [100000 + 7 * s for s in range(S)], [250000, 625000, 1000000, 48000, 2400000]
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a = sd.RxPipe(ctx, S, nb_fec=8, sample_bits=15, center_frequency_khz=1, sample_rate=2, **cfg)
    twins = Twins(ctx, BITS, fec=HUB_FEC, fc=fcs, rate=rates, **cfg)
    a.set_stream_bits(BITS)
    a.set_stream_fec(HUB_FEC)
    a.set_stream_meta(fcs, rates)
    rs = np.random.RandomState(41)
    for k, frames in enumerate([[2, 1, 1, 2, 1], [1, 2, 0, 1, 2]]):
        xs, counts = ragged_blocks(rs, S, L, frames, k == 0)
        secs, usecs = stamps(k, S)
        got, nf = a.process_ragged(rows_of(xs, counts), counts, secs, usecs)
        same(got, twins.ragged(xs, counts, secs, usecs), ("three", k))
        says(got, L, BITS, ("three", k))
        for s, g in enumerate(got):
            for fr in np.asarray(g):
                assert tf.meta_of(fr)[:2] == (fcs[s], rates[s]) and fr[0, 15] == HUB_FEC[s], (k, s)
    a.set_egress("round_robin")
    calls = dgram_calls(oracle)
    for i in (0, 1, 2):
        secs, usecs = stamps(i, S)
        a.submit_datagrams(calls[i], secs, usecs)
        exp = twins.datagrams(calls[i], secs, usecs)
        dg, tags, nf, records = a.collect_egress()
        e_dg, e_tags = twin_rounds([fr for fr, _ in exp])
        assert dg.tobytes() == e_dg.tobytes() and np.array_equal(tags, e_tags), i
        assert records == [r for _, r in exp], i
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 6. equal entries
def test_equal_entries_through_the_array(oracle, ctx):
    """an array of equal entries delivers the bytes of the pipe whose config carries that size; NULL restores cfg.sample_bits"""
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S, L = len(calls[0]), 1
    a = sd.RxPipe(ctx, S, log2decim=L, nb_fec=8, sample_bits=16)
    b = sd.RxPipe(ctx, S, log2decim=L, nb_fec=8, sample_bits=12)
    a.set_stream_bits([12] * S)
    rs = np.random.RandomState(1)
    for k, frames in enumerate([[1, 2, 0, 1, 1], [2, 1, 1, 0, 2]]):
        xs, counts = ragged_blocks(rs, S, L, frames, k == 0)
        ga, na = a.process_ragged(rows_of(xs, counts), counts, 3, 4)
        gb, nb = b.process_ragged(rows_of(xs, counts), counts, 3, 4)
        assert list(na) == list(nb)
        same(per_stream(ga, na), per_stream(gb, nb), ("equal", k))
    a.submit_datagrams(calls[3], 1, 2)
    b.submit_datagrams(calls[3], 1, 2)
    ea, eb = a.collect_datagrams(), b.collect_datagrams()
    assert sum(f.shape[0] for f, _ in eb) > 0
    same([f for f, _ in ea], [f for f, _ in eb], "stream order")
    a.set_stream_bits(None)
    b.reconfigure(sample_bits=16)
    assert a.stream_bits(2) == (16, 16)
    x = rs.randint(-32768, 32768, size=(S, (2 * F + 9) << L, 2)).astype(np.int16)
    ga, gb = a.process(x, 5, 6), b.process(x, 5, 6)  # (bank-wide again: the uniform entry is open)
    assert ga.shape == gb.shape and ga.shape[1] >= 2 and ga.tobytes() == gb.tobytes()
    says(list(ga[:, 1:]), L, [16] * S, "bank-wide again")  # (the first frame was open across the change: it says 12 + 1)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_consume_nothing(ctx):
    """each refused call leaves the pipe where it was: the next accepted call still matches the twins"""
    import sdrdaemon_amd as sd

    L, S = 1, 5
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    a, twins = sd.RxPipe(ctx, S, sample_bits=16, **cfg), Twins(ctx, [16] * S, **cfg)
    rs = np.random.RandomState(14)
    step = [0]

    def accepted():
        xs, counts = ragged_blocks(rs, S, L, [1, 2, 1, 0, 1], step[0] == 0)
        secs, usecs = stamps(step[0], S)
        step[0] += 1
        got, nf = a.process_ragged(rows_of(xs, counts), counts, secs, usecs)
        same(per_stream(got, nf), twins.ragged(xs, counts, secs, usecs), ("accepted", step[0]))
        return xs, counts

    accepted()
    assert code(a.set_stream_bits, [8, 12, 0, 16, 16]) == EINVAL and code(a.set_stream_bits, [8, 12, 17, 16, 16]) == EINVAL
    assert [a.stream_bits(s)[0] for s in range(S)] == [16] * S  # (nothing changed)
    assert ctx.lib.sdrhip_rx_set_stream_bits(None, None) == EINVAL
    accepted()
    a.set_stream_bits(BITS)
    twins.reconfigure(BITS)
    xs, counts = accepted()
    # ---- the uniform entries and pipelined mode
    x = rows_of(xs, counts)[:, :64]
    assert code(a.process, x) == EINVAL and code(a.submit, x) == EINVAL
    assert ctx.lib.sdrhip_rx_set_pipelined(a.h, 1) == EINVAL
    assert code(a.set_stream_bits, [8, 12, 17, 16, 16]) == EINVAL and a.stream_bits(2) == (16, 16)
    accepted()
    # ---- the setter with a batch in flight is allowed: the batch keeps the values it was launched with
    a.set_async(depth=2)
    xs, counts = ragged_blocks(rs, S, L, [1, 0, 2, 1, 1], False)
    a.submit_ragged(np.concatenate(xs).reshape(-1), counts, 11, 12)
    a.set_stream_bits([9] * S)
    exp = twins.ragged(xs, counts, [11] * S, [12] * S)
    same(a.collect_ragged(), exp, "in flight")
    twins.reconfigure([9] * S)
    accepted()
    # ---- a pipelined pipe
    p = sd.RxPipe(ctx, 2, pipelined=True, **cfg)
    assert code(p.set_stream_bits, [8, 12]) == EINVAL and p.stream_bits(1) == (16, 16)


# ------------------------------------------------------------------------------------------------ 8. export / import
def test_export_import_with_the_array_set_on_both_banks(ctx):
    """stream 1 of bank A moves to stream 0 of bank B, both with their own arrays: it continues with the destination's bits, like a
    twin that was reconfigured at the same point; the frame that was open across the move says the size it was opened with"""
    import sdrdaemon_amd as sd

    L = 1
    bits_a, bits_b = [8, 12, 16], [13, 10]
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    A, B = sd.RxPipe(ctx, 3, **cfg), sd.RxPipe(ctx, 2, **cfg)
    ta, tb = Twins(ctx, bits_a, **cfg), Twins(ctx, bits_b, **cfg)
    A.set_stream_bits(bits_a)
    B.set_stream_bits(bits_b)
    rs = np.random.RandomState(52)

    def run(bank, twins, frames, k, first):
        S = len(twins.p)
        xs, counts = ragged_blocks(rs, S, L, frames, first)
        secs, usecs = stamps(k, S)
        got, nf = bank.process_ragged(rows_of(xs, counts), counts, secs, usecs)
        got = per_stream(got, nf)
        same(got, twins.ragged(xs, counts, secs, usecs), ("move", k, S))
        return got

    run(A, ta, [1, 2, 1], 0, True)
    run(B, tb, [2, 1], 0, True)
    blob = A.export_stream(1)
    B.import_stream(0, blob)
    assert B.stream_bits(0) == (13, 14) and A.stream_bits(1) == (12, 13)  # (configuration: untouched by the move)
    moved = ta.p[1]
    blob_t = moved.export_stream(0)
    t2 = sd.RxPipe(ctx, 1, sample_bits=12, **cfg)  # (A keeps running its stream 1: its twin goes on from a copy of the same state)
    t2.import_stream(0, blob_t)
    moved.reconfigure(sample_bits=13)
    tb.p[0], ta.p[1] = moved, t2
    for k in (1, 2):
        got = run(B, tb, [2, 1], k, False)
        if k == 1:
            assert bytes_8_9(np.asarray(got[0][0]))[1] == 13 and bytes_8_9(np.asarray(got[0][1]))[1] == 14
        run(A, ta, [1, 1, 2], k, False)
