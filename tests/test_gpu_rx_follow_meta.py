"""Outgoing meta that follows the incoming meta blocks (sdrhip_rx_set_follow_meta) of the Rx pipe fed raw FEC datagrams.

The rule (include/sdrhip.h): after a call's collection a stream's m_outputMeta is the meta block of the last released frame whose
block 0 was among its first 128 arrivals; if its sample rate is not 0, every frame the call's step opens carries its centre
frequency and its rate >> log2decim (also the clock of the stamps), else the host's values (the sdrhip_rx_set_stream_meta arrays,
else the configuration); an open frame keeps its block 0.

Incoming frames are real ones: the oracle framer over random samples with the sender's frequency and rate, frame_encode for the
incoming fecblk (1..8), blocks dropped.  The expected m_outputMeta comes from the Python collector model of test_gpu_fecbuf (held
there against sdrhip_fecbuf_stats), the expected frames from HubChain of test_gpu_rx_datagrams with its framer set to the rule's
values before each call.  Everything is byte-exact.

Shapes: F = 16129 samples per payload and per frame.  A bank of 8 streams gets 3 incoming frames per stream and call (5 at
decimation 16, where 16 payloads make one frame: fewer cannot complete the two frames the checks ask for, even behind `prime`)."""
import struct
import zlib

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_rx_datagrams as tr
import test_gpu_rx_datagrams_async as ta
import test_gpu_tx_datagrams as tt

pytestmark = pytest.mark.gpu

F = 16129
ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)
reflib = tt.reflib
CFG_FC, CFG_RATE = 435000, 625000  # (the defaults of RxPipe and of HubChain's framer)
KINDS = ["a", "a", "b", "c", "d", "e", "f", "g"]
A_META = {0: (3000000000, 10000000), 1: (4294967295, 48000)}
D_META, D_DECOY = (1296500, 250000), (777, 999999)
HOST_FC = [1000 + s for s in range(8)]
HOST_RATE = [2000000 + s for s in range(8)]


@pytest.fixture(autouse=True, scope="module")
def torch_first():
    """torch brings its device runtime up before the reference's FEC buffer library is first used (as test_gpu_rx_datagrams)"""
    import torch

    torch.zeros(1).cuda()


def meta_of(frame):
    """(centre frequency, sample rate, tv_sec, tv_usec) of a frame's meta block (block 0 behind its 4-byte header)"""
    w = np.frombuffer(np.ascontiguousarray(frame[0, 4:28]).tobytes(), dtype="<u4")
    return int(w[0]), int(w[1]), int(w[3]), int(w[4])


def crc_ok(frame):
    b = np.ascontiguousarray(frame[0, 4:28]).tobytes()
    return zlib.crc32(b[:20]) == struct.unpack("<I", b[20:24])[0]


def rule(out_meta, L, host):
    """what the frames a call opens announce, from the stream's m_outputMeta after the call's collection"""
    fc, rate = struct.unpack("<II", bytes(out_meta[:8]))
    return (fc, rate >> L) if rate else tuple(host)


def kind_meta(kind, s, k, per_call, L):
    """what the sender of stream s puts into incoming frame k"""
    if kind == "a":  # constant, distinct per stream (one frequency above 2^31, one all ones)
        return A_META[s]
    if kind == "b":  # changes with every frame
        return 200000 + 7 * k, 2000000 + 1000 * k
    if kind == "c":  # changes between calls
        return 300000 + k // per_call, 1000000 + 8000 * (k // per_call)
    if kind == "d":  # the odd frames lose their block 0 (repaired): their values must never show
        return D_DECOY if k % 2 else D_META
    if kind == "e":  # every block 0 lost
        return 555, 5555555
    if kind == "f":  # the sender says rate 0
        return 144800, 0
    return 10489750, (1 << L) - 1 if L else 1  # g: a rate below 2^L


def incoming(oracle, rs, metas, R_in, fi0):
    """one frame of 128 + R_in super blocks per entry of metas = (centre frequency, sample rate): a real meta block, protected"""
    fr = oracle.framer(nb_fec_blocks=R_in)
    fr.s.frame_count = fi0
    out = []
    for k, (fc, rate) in enumerate(metas):
        fr.s.center_frequency_khz, fr.s.sample_rate, fr.s.tv_sec, fr.s.tv_usec = fc, rate, 5000 + k, 7 * k
        f, = fr.write(rs.randint(-32768, 32768, size=(F, 2)).astype(np.int16))
        assert meta_of(f)[:2] == (fc, rate)
        out.append(np.concatenate([f, oracle.frame_encode(f, R_in)]))
    return out


_STREAMS = {}


def bank_streams(oracle, seed, L, per_call, ncalls):
    """per stream of the eight kinds: per incoming frame the list of its datagrams that arrive"""
    key = (seed, L, per_call, ncalls)
    if key not in _STREAMS:
        rs = np.random.RandomState(seed)
        per = []
        for s, kind in enumerate(KINDS):
            R_in = 1 + (3 * s) % 8
            nf = per_call * ncalls
            frames = incoming(oracle, rs, [kind_meta(kind, s, k, per_call, L) for k in range(nf)], R_in, int(rs.randint(0, 65536)))
            dgs = []
            for k, f in enumerate(frames):
                drop0 = kind == "e" or (kind == "d" and k % 2 == 1)
                nlost = max(int(rs.randint(0, R_in + 1)) - (1 if drop0 else 0), 0)
                lost = set((1 + rs.choice(127 + R_in, nlost, replace=False)).tolist()) | ({0} if drop0 else set())
                dgs.append([f[i] for i in range(128 + R_in) if i not in lost])
            per.append(dgs)
        _STREAMS[key] = per
    return _STREAMS[key]


def follow_calls(oracle, seed, L, per_call, ncalls, off_seed=0, cut_frames=None):
    """the streams cut into calls: cut i lies 1..99 datagrams (off_seed) into incoming frame i * per_call (cut_frames: these frames
    instead).  A frame is released by the first datagram of the next one, so whatever off_seed is, the same frames are released in
    the same calls"""
    per = bank_streams(oracle, seed, L, per_call, ncalls)
    ro = np.random.RandomState(1000 + off_seed)
    cut_frames = cut_frames or [i * per_call for i in range(1, ncalls)]
    cut = []
    for dgs in per:
        flat = np.asarray([d for f in dgs for d in f], np.uint8).reshape(-1, 512)
        starts = np.cumsum([0] + [len(f) for f in dgs])
        b = [0] + [int(starts[k]) + int(ro.randint(1, 100)) for k in cut_frames] + [flat.shape[0]]
        cut.append([flat[b[i]:b[i + 1]] for i in range(len(b) - 1)])
    return [[c[i] for c in cut] for i in range(len(cut_frames) + 1)]


class FollowChain(tr.HubChain):
    """HubChain whose framer announces the rule's values in the frames a call opens; keeps, for every outgoing frame, the two words
    it must carry (the frame open when a call begins keeps the words it was opened with)"""

    def __init__(self, lib, oracle, host):
        tr.HubChain.__init__(self, lib, oracle)
        self.fr.s.center_frequency_khz, self.fr.s.sample_rate = host
        self.pending, self.open_words = 0, None

    def track(self, n_dec, words):
        """n_dec decimated samples arrive under `words`: -> the words of the frames they complete"""
        total = self.pending + n_dec
        done = total // F
        out = []
        if done:
            out = ([self.open_words] if self.pending else []) + [words] * (done - (1 if self.pending else 0))
        if total % F and (done or not self.pending):
            self.open_words = words  # (the frame left open was opened by this call)
        self.pending = total % F
        return out

    def call(self, dg, L, fcpos, R, sec, usec, words):
        self.fr.s.center_frequency_khz, self.fr.s.sample_rate = words
        frames = self.dgrams(dg, L, fcpos, R, sec, usec)
        exp = self.track(self.fed >> L, words)
        assert len(exp) == len(frames)
        return frames, exp

    def dgrams(self, dg, L, fcpos, R, sec, usec):
        """HubChain.dgrams, keeping the number of samples the call feeds its decimator"""
        pay = self.col.collect(dg)
        if pay:
            self.rem = np.concatenate([self.rem] + [p.view(np.int16).reshape(-1, 2) for p in pay])
        self.fed = len(self.rem) // tr.unit(L, fcpos) * tr.unit(L, fcpos)
        x, self.rem = self.rem[:self.fed], self.rem[self.fed:]
        return self.samples(x, L, fcpos, R, sec, usec)


def make_bank(ctx, S, arrays=False, follow=True, **cfg):
    import sdrdaemon_amd as sd

    rx = sd.RxPipe(ctx, S, center_frequency_khz=CFG_FC, sample_rate=CFG_RATE, **cfg)
    host = [(CFG_FC, CFG_RATE)] * S
    if arrays:
        rx.set_stream_meta(HOST_FC[:S], HOST_RATE[:S])
        host = list(zip(HOST_FC[:S], HOST_RATE[:S]))
    if follow:
        rx.set_follow_meta()
    return rx, host


def model_step(rx, models, chunk, L, host):
    """the collector models over the call's datagrams (after the call): the bank's m_outputMeta agrees; -> the rule's values"""
    words = []
    for s, m in enumerate(models):
        m.run(chunk[s])
        assert rx.collector_stats(s)["output_meta"][:20] == m.out_meta, s
        words.append(rule(m.out_meta, L, host[s]))
    return words


# ------------------------------------------------------------------------------------------------ 1. the reference chain
SHAPES = {0: (3, 3), 2: (3, 4), 3: (4, 4), 4: (5, 4)}  # L -> incoming frames per call, calls


@pytest.mark.parametrize("L,fcpos,R,arrays", [(0, 2, 8, True), (2, 2, 32, False), (3, 0, 8, True), (4, 2, 8, False)])
def test_reference_chain(oracle, ctx, reflib, L, fcpos, R, arrays):
    """8 streams of the kinds (a)..(g), stream 1 fed nothing in call 1 (h); device and host datagrams alternate.  The fallback
    streams (e), (f) run with the set_stream_meta arrays set (arrays) and with the configuration alone"""
    S = 8
    per_call, ncalls = SHAPES[L]
    calls = [list(c) for c in follow_calls(oracle, 500, L, per_call, ncalls)]
    calls[2][1] = np.concatenate([calls[1][1], calls[2][1]])
    calls[1][1] = np.zeros((0, 512), np.uint8)
    rx, host = make_bank(ctx, S, arrays, log2decim=L, fcpos=fcpos, nb_fec=R)
    chains = [FollowChain(reflib, oracle, host[s]) for s in range(S)]
    models = [tg.Model(oracle) for _ in range(S)]
    if L >= 3:
        tr.prime([rx], chains, L, fcpos, R, 999, 1)
        for s, c in enumerate(chains):
            assert c.track(F - 300, host[s]) == []
    count, seen = [0] * S, [set() for _ in range(S)]
    for i, chunk in enumerate(calls):
        secs, usecs = [1000 + 10 * i + s for s in range(S)], [999990 - 37 * i - s for s in range(S)]
        got = tr.run_call(rx, chunk, secs, usecs, device=i % 2 == 0)
        words = model_step(rx, models, chunk, L, host)
        for s in range(S):
            exp, exp_words = chains[s].call(chunk[s], L, fcpos, R, secs[s], usecs[s], words[s])
            tr.check_frames(got[s][0], exp, (L, fcpos, i, s))
            for f, w in enumerate(exp_words):
                assert meta_of(got[s][0][f])[:2] == w, (i, s, f, meta_of(got[s][0][f]), w)
                assert crc_ok(got[s][0][f]), (i, s, f)
                seen[s].add(w)
            count[s] += len(exp)
        assert list(rx.carry()) == [len(c.rem) for c in chains]
        assert rx.stream_meta(3) == {"center_frequency_khz": host[3][0], "sample_rate": host[3][1]}  # (the host's values, always)
    print("frames per stream", count, "distinct words", [len(x) for x in seen])
    for s, kind in enumerate(KINDS):
        if kind in "abcdg":
            assert count[s] >= 2, (s, kind, count[s])
        primed = {host[s]} if L >= 3 else set()
        if kind == "a":
            assert seen[s] - primed == {(A_META[s][0], A_META[s][1] >> L)}, (s, seen[s])
        elif kind in "bc":
            assert len(seen[s] - primed) >= min(2, count[s] - len(primed)), (s, seen[s])  # (x8, x16: one frame behind the primed one)
        elif kind == "d":
            assert seen[s] - primed == {(D_META[0], D_META[1] >> L)}, seen[s]
        elif kind in "ef":
            assert count[s] >= 1 and seen[s] == {host[s]}, (s, seen[s])
        else:
            assert seen[s] - primed == {(10489750, 0 if L else 1)}, seen[s]


# ------------------------------------------------------------------------------------------------ 2. one-stream twins
def run_twins(ctx, oracle, calls, S, L, R, want_mfma=False):
    """the bank with follow on against one-stream pipes reconfigured before each call with the rule's values"""
    import torch

    import sdrdaemon_amd as sd

    bank, host = make_bank(ctx, S, log2decim=L, nb_fec=R)
    twins = [sd.RxPipe(ctx, 1, log2decim=L, nb_fec=R, center_frequency_khz=CFG_FC, sample_rate=CFG_RATE) for _ in range(S)]
    models = [tg.Model(oracle) for _ in range(S)]
    count, followed = [0] * S, 0
    for i, chunk in enumerate(calls):
        arg = [torch.from_numpy(c).cuda() for c in chunk] if i % 2 == 0 else chunk
        secs = [70 + 3 * i + s for s in range(S)]
        got = bank.process_datagrams(arg, secs, 999999)
        if want_mfma:
            plan = bank.last_plan()
            assert plan["path"] == "mfma" and plan["wps"] > 0, plan
        words = model_step(bank, models, chunk, L, host)
        for s in range(S):
            twins[s].reconfigure(center_frequency_khz=words[s][0], sample_rate=words[s][1])
            (e, recs), = twins[s].process_datagrams([arg[s]], secs[s], 999999)
            g, e = tt.as_np(got[s][0]), tt.as_np(e)
            assert recs == got[s][1] and g.shape == e.shape and np.array_equal(g, e), (i, s)
            count[s] += g.shape[0]
            followed += sum(1 for f in g if meta_of(f)[:2] != host[s])
    return count, followed


def test_bank_equals_reconfigured_one_stream_pipes(oracle, ctx):
    per_call, ncalls = SHAPES[2]
    count, followed = run_twins(ctx, oracle, follow_calls(oracle, 500, 2, per_call, ncalls), 8, 2, 32)
    assert min(count) >= 2 and followed >= 10, (count, followed)


# ------------------------------------------------------------------------------------------------ 3. the matrix cores
def plain_frames(m, fi0=0):
    """m loss-free frames of zero payload without recovery blocks: headers alone (what a probe call needs)"""
    dg = np.zeros((m, 128, 512), np.uint8)
    fi = (fi0 + np.arange(m)) & 0xFFFF
    dg[:, :, 0], dg[:, :, 1], dg[:, :, 2] = (fi & 0xFF)[:, None], (fi >> 8)[:, None], np.arange(128)[None, :]
    return dg.reshape(-1, 512)


def smallest_mfma_hub_call(ctx, S, L, **cfg):
    """the fewest incoming frames per stream and call for which the hub's decimator launch is the matrix-core one with wave groups"""
    import torch

    import sdrdaemon_amd as sd

    for m in (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
        probe = sd.RxPipe(ctx, S, log2decim=L, **cfg)
        probe.process_datagrams([torch.from_numpy(plain_frames(m)).cuda()] * S)
        ctx.synchronize()
        plan = probe.last_plan()
        probe.close()
        if plan["path"] == "mfma" and plan["wps"] > 0:
            return m
    pytest.fail("no hub call up to 64 frames per stream takes the matrix-core path")


@pytest.mark.parametrize("rx_direct", [1, 0])
def test_on_the_matrix_cores(oracle, ctx, rx_direct):
    """decim_path = mfma, L = 3, distinct incoming meta per stream.  rx_direct = 1: K1mr's pieces write block 0 from the shared
    record, the rewrite behind it must carry the followed values; 0: stream order + K2r"""
    ctx.set_option("decim_path", "mfma")
    ctx.set_option("rx_direct", rx_direct)
    S, L, R = 4, 3, 8
    m = smallest_mfma_hub_call(ctx, S, L, nb_fec=R)
    ncalls = -(-18 // m)  # (x8: 8 payloads make one outgoing frame, and the last incoming frame is not released: 18 give two)
    rs = np.random.RandomState(90 + rx_direct)
    per = []
    for s in range(S):
        frames = incoming(oracle, rs, [(700000 + s, 4000000 + 8 * s)] * (ncalls * m), 1, 100 * s)
        per.append([f[1:] if k % 5 == 3 else f[:128] for k, f in enumerate(frames)])  # (every fifth block 0 lost and repaired)
    calls = [[np.concatenate(per[s][i * m:(i + 1) * m]) for s in range(S)] for i in range(ncalls)]
    count, followed = run_twins(ctx, oracle, calls, S, L, R, want_mfma=True)
    print("frames per call and stream: %d incoming, %d calls; completed" % (m, ncalls), count, "followed", followed)
    assert min(count) >= 2 and followed == sum(count)  # (every call releases frames with their block 0: every frame follows)
    assert ctx.option("rx_direct") == str(rx_direct)


# ------------------------------------------------------------------------------------------------ 4. more than one wave of streams
def test_66_streams(oracle, ctx):
    import sdrdaemon_amd as sd

    S = 66
    rs = np.random.RandomState(66)
    chunk = []
    for s in range(S):
        frames = incoming(oracle, rs, [(1000 + s, 48000 + s)] * 2, 1, 7 * s)
        chunk.append(np.concatenate([frames[0][:128], frames[1][:128], plain_frames(1, 7 * s + 2)[:1]]))
    rx, _ = make_bank(ctx, S, log2decim=0, nb_fec=1)
    got = tr.run_call(rx, chunk, 12, 999999)
    for s in range(S):
        fr = got[s][0]
        assert fr.shape[0] == 3, (s, fr.shape)  # (the collector's initial slot and the two frames)
        for f in fr:
            assert meta_of(f)[:2] == (1000 + s, 48000 + s) and crc_ok(f), (s, meta_of(f))
            assert meta_of(f)[2] >= 12
        if s in (0, 63, 64, 65):
            for f in fr:
                assert np.array_equal(f[128:], oracle.frame_encode(f[:128], 1)), s


# ------------------------------------------------------------------------------------------------ 5. asynchronous batches
@pytest.mark.parametrize("strided", [False, True])
def test_async_batches(oracle, ctx, strided):
    """depth 3, three batches in flight, the flag toggled between the submits (on, off, on, on): a batch keeps the mode of its
    submit.  Byte equality with sdrhip_rx_process_datagrams on a twin that toggles between its calls; the link traffic of every
    submit equals that of a handle that never saw the flag"""
    S, L, R = 8, 0, 8
    per_call, ncalls = 3, 4
    calls = follow_calls(oracle, 500, L, per_call, ncalls)
    flags = [True, False, True, True]
    a, host = make_bank(ctx, S, follow=False, log2decim=L, nb_fec=R)
    b, _ = make_bank(ctx, S, follow=False, log2decim=L, nb_fec=R)
    c, _ = make_bank(ctx, S, follow=False, log2decim=L, nb_fec=R)
    a.set_async(depth=3)
    c.set_async(depth=3)
    keep, exp, got, traffic = [], [], [], {"a": [], "c": []}

    def submit(p, name, i):
        sec, usec = ta.stamps(i, S)
        c0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        ta.submit_raw(ctx, p, calls[i], sec, usec, strided, False, keep)
        traffic[name].append((ctx.counter("h2d_bytes") - c0[0], ctx.counter("d2h_bytes") - c0[1]))

    def step(i):
        sec, usec = ta.stamps(i, S)
        a.set_follow_meta(flags[i])
        b.set_follow_meta(flags[i])
        submit(a, "a", i)
        exp.append(b.process_datagrams(calls[i], sec, usec))
        assert list(a.carry()) == list(b.carry()), i

    for i in range(3):
        step(i)
    a.set_follow_meta(False)  # (every batch is in flight: they keep their modes)
    for i in range(3):
        got.append(a.collect_datagrams())
    for s in range(S):
        assert a.collector_stats(s) == b.collector_stats(s), s
    step(3)
    for s in range(S):
        assert a.collector_stats(s) == b.collector_stats(s), s
    got.append(a.collect_datagrams())
    for i in range(ncalls):
        submit(c, "c", i)
        if i >= 2:
            c.collect_datagrams()
    for _ in range(2):
        assert c.collect_datagrams() is not None
    models = [tg.Model(oracle) for _ in range(S)]
    for i in range(ncalls):
        for s in range(S):
            models[s].run(calls[i][s])
            g, e = got[i][s][0], np.asarray(exp[i][s][0])
            assert got[i][s][1] == exp[i][s][1], (i, s)
            assert g.shape == e.shape and g.tobytes() == e.tobytes(), (i, s)
            assert g.shape[0] >= 2, (i, s)
            want = rule(models[s].out_meta, L, host[s]) if flags[i] else host[s]
            assert all(meta_of(f)[:2] == want for f in g), (i, s, want)  # (x1: every frame of a batch is opened by it)
    assert traffic["a"] == traffic["c"], traffic
    assert ta.mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 6. cut invariance
def test_cut_invariance(oracle, ctx):
    """one datagram sequence per stream cut two ways that release the same frames in the same calls (the cuts move inside a frame):
    the same outgoing frames; cut a third way, into two calls: the same m_outputMeta at the end"""
    S, L, R = 8, 2, 8
    per_call, ncalls = SHAPES[L]
    runs, metas = [], []
    for off_seed, cut_frames in ((0, None), (1, None), (2, [5])):
        calls = follow_calls(oracle, 500, L, per_call, ncalls, off_seed, cut_frames)
        rx, _ = make_bank(ctx, S, log2decim=L, nb_fec=R)
        out = [[] for _ in range(S)]
        for i, chunk in enumerate(calls):
            got = tr.run_call(rx, chunk, 5, 6, device=i % 2 == 1)
            for s in range(S):
                out[s].append(got[s][0])
        runs.append([np.concatenate(o) for o in out])
        metas.append([rx.collector_stats(s)["output_meta"] for s in range(S)])
    models = [tg.Model(oracle) for _ in range(S)]
    for chunk in follow_calls(oracle, 500, L, per_call, ncalls):
        for s in range(S):
            models[s].run(chunk[s])
    for s in range(S):
        assert runs[0][s].shape[0] >= 2
        assert np.array_equal(runs[0][s], runs[1][s]), s
        assert metas[0][s] == metas[1][s] == metas[2][s] and metas[0][s][:20] == models[s].out_meta, s
    assert any(not np.array_equal(runs[0][s], runs[2][s]) for s in (2, 3))  # (other calls: other frames carry a changing meta)


# ------------------------------------------------------------------------------------------------ 7. the untouched default
def test_flag_off_is_untouched(oracle, ctx, reflib):
    """never touched, and set then cleared: the bytes of the hub chain with the configuration's values, the same plan"""
    S, L, R = 8, 2, 8
    per_call, ncalls = SHAPES[L]
    calls = follow_calls(oracle, 500, L, per_call, ncalls)[:3]
    plain, _ = make_bank(ctx, S, follow=False, log2decim=L, nb_fec=R)
    cleared, _ = make_bank(ctx, S, follow=True, log2decim=L, nb_fec=R)
    cleared.set_follow_meta(False)
    chains = [tr.HubChain(reflib, oracle) for _ in range(S)]
    total = 0
    for i, chunk in enumerate(calls):
        p, q = tr.run_call(plain, chunk, 8, i), tr.run_call(cleared, chunk, 8, i)
        assert plain.last_plan() == cleared.last_plan()
        for s in range(S):
            assert p[s][1] == q[s][1] and np.array_equal(p[s][0], q[s][0]), (i, s)
            tr.check_frames(p[s][0], chains[s].dgrams(chunk[s], L, 2, R, 8, i), (i, s))
            assert all(meta_of(f)[:2] == (CFG_FC, CFG_RATE) for f in p[s][0]), (i, s)
            total += p[s][0].shape[0]
    assert total >= S
