"""The sample size that follows the incoming meta blocks (sdrhip_rx_set_follow_bits) of the Rx pipe fed raw FEC datagrams.

The rule (include/sdrhip.h): after a call's collection a stream's m_outputMeta is the meta block of the last released frame whose
block 0 was among its first 128 arrivals; if its sampleBits byte b is 1..16, every sample the call's step decimates for the stream
takes the shift pair of (log2decim, b) and every frame the step opens says the decimated size b' in bytes 8 and 9, else the stream
keeps the host's size (its entry of the sdrhip_rx_set_stream_bits array, else cfg.sample_bits); an open frame keeps its block 0.

Incoming frames are real ones: the oracle framer with the sender's frequency, rate and size, frame_encode for the incoming fecblk
(1..8), blocks dropped.  The expected m_outputMeta comes from the Python collector model of test_gpu_fecbuf, held against
sdrhip_fecbuf_stats after every call; the expected frames from one-stream twins, sd.RxPipe(ctx, 1, ...) with the flag off,
reconfigured before each call with the sample_bits the rule gives and fed the same datagrams (their own collectors release the
same samples).  Everything is byte-exact.

Shapes: F = 16129 samples per payload and per frame; 8 streams, 3 incoming frames per stream and call (5 at decimation 16, behind a
sample-fed call that leaves every open frame 300 samples short, so that the few payloads complete two frames)."""
import struct
import zlib

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_rx_datagrams as tr
import test_gpu_rx_datagrams_async as ta
import test_gpu_rx_follow_meta as tf
import test_gpu_rx_stream_bits as tb
import test_gpu_tx_datagrams as tt
from test_gpu_dgram_tagged import merge
from test_gpu_rx_egress import rounds

pytestmark = pytest.mark.gpu

F = 16129
ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)
torch_first = tf.torch_first
CFG_FC, CFG_RATE, CFG_BITS = tf.CFG_FC, tf.CFG_RATE, 14
HOST_BITS = [9, 10, 11, 13, 15, 7, 6, 5]  # (the set_stream_bits array: no entry is a size its stream's sender says)
KINDS = ["8", "12", "16", "x", "c", "d", "e", "z"]
C_BITS, D_BITS, D_DECOY = [12, 8, 16, 10, 13, 9], 12, 5
Z_BITS = [0, 17, 255]
RESTORE = {"decim_path": "auto", "mfma_span": 0, "rx_direct": "1"}


def sender_meta(s):
    return 700000 + s, 2000000 + 8 * s


def kind_bits(kind, k, per_call, L):
    """the sampleBits byte the sender of a stream of this kind puts into incoming frame k"""
    if kind in ("8", "12", "16"):  # RTL-SDR / HackRF, Airspy / BladeRF, the test source
        return int(kind)
    # (a walk of period 3 inside a call, shifted by one from call to call: the last frame a call releases -- frame per_call - 1 of
    # its own, the cut lies behind the head of the next -- walks too, at 3 and at 5 frames per call)
    j = (k % per_call + k // per_call + 1) % 3
    if kind == "x":  # changes with every frame, across the step between norm and trunk: 16 - L - 1, 16 - L, 16 - L + 1
        return min(max(16 - L - 1 + j, 1), 16)
    if kind == "c":  # changes between calls
        return C_BITS[(k // per_call) % len(C_BITS)]
    if kind == "d":  # the odd frames lose their block 0 (repaired): their size must never show
        return D_DECOY if k % 2 else D_BITS
    if kind == "e":  # every block 0 lost
        return 8
    return Z_BITS[j]  # z: a sender that says 0, 17 and 255


def rule_bits(out_meta, host):
    b = out_meta[9]
    return b if 1 <= b <= 16 else host


def incoming(oracle, rs, s, bits, R_in, fi0, full_scale):
    """one frame of 128 + R_in super blocks per entry of bits: a real meta block that says that size (every other frame with an
    indicator nibble in sampleBytes, which the rule does not read), protected.  full_scale: int16 payload over the whole range,
    else within 12 bits"""
    fr = oracle.framer(nb_fec_blocks=R_in)
    fr.s.frame_count = fi0
    fr.s.center_frequency_khz, fr.s.sample_rate = sender_meta(s)
    hi = 32768 if full_scale else 2048
    out = []
    for k, b in enumerate(bits):
        fr.s.sample_bits, fr.s.sample_bytes, fr.s.tv_sec, fr.s.tv_usec = b, (((b - 1) // 8 + 1) & 0xF) | (0x10 if k % 2 else 0), 5000 + k, 7 * k
        f, = fr.write(rs.randint(-hi, hi, size=(F, 2)).astype(np.int16))
        assert int(f[0, 4 + 9]) == b
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
            frames = incoming(oracle, rs, s, [kind_bits(kind, k, per_call, L) for k in range(nf)], R_in, int(rs.randint(0, 65536)), s % 2 == 0)
            dgs = []
            for k, f in enumerate(frames):
                drop0 = kind == "e" or (kind == "d" and k % 2 == 1)
                nlost = max(int(rs.randint(0, R_in + 1)) - (1 if drop0 else 0), 0)
                lost = set((1 + rs.choice(127 + R_in, nlost, replace=False)).tolist()) | ({0} if drop0 else set())
                dgs.append([f[i] for i in range(128 + R_in) if i not in lost])
            per.append(dgs)
        _STREAMS[key] = per
    return _STREAMS[key]


def bits_calls(oracle, seed, L, per_call, ncalls, off_seed=0, idle=True):
    """the streams cut into calls: cut i lies 1..99 datagrams (off_seed) into incoming frame i * per_call.  A frame is released by
    the first datagram of the next one, so whatever off_seed is, the same frames are released in the same calls.  idle: stream 1
    is fed nothing in call 1 (its datagrams arrive in call 2)"""
    per = bank_streams(oracle, seed, L, per_call, ncalls)
    ro = np.random.RandomState(1000 + off_seed)
    cut = []
    for dgs in per:
        flat = np.asarray([d for f in dgs for d in f], np.uint8).reshape(-1, 512)
        starts = np.cumsum([0] + [len(f) for f in dgs])
        b = [0] + [int(starts[i * per_call]) + int(ro.randint(1, 100)) for i in range(1, ncalls)] + [flat.shape[0]]
        cut.append([flat[b[i]:b[i + 1]] for i in range(ncalls)])
    calls = [[c[i] for c in cut] for i in range(ncalls)]
    if idle:
        calls[2][1] = np.concatenate([calls[1][1], calls[2][1]])
        calls[1][1] = np.zeros((0, 512), np.uint8)
    return calls


def make_twins(ctx, host_bits, fec=None, **cfg):
    import sdrdaemon_amd as sd

    return [sd.RxPipe(ctx, 1, center_frequency_khz=CFG_FC, sample_rate=CFG_RATE, sample_bits=b, **dict(cfg, **({"nb_fec": fec[s]} if fec else {})))
            for s, b in enumerate(host_bits)]


def prime(bank, twins, L, short=300):
    """a sample-fed call (the flag is ignored: the host's sizes) that leaves every open frame `short` decimated samples from full"""
    S, n = len(twins), (F - short) << L
    x = np.random.RandomState(5).randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)
    assert not np.asarray(bank.process_ragged(x, [n] * S, 999, 1)[1]).any()
    for s, p in enumerate(twins):
        assert not np.asarray(p.process_ragged(x[s:s + 1], [n], 999, 1)[1]).any()


def model_step(rx, models, chunk, host_bits):
    """the collector models over the call's datagrams (after the call): the bank's m_outputMeta agrees; -> the rule's sizes"""
    sizes = []
    for s, m in enumerate(models):
        m.run(chunk[s])
        assert rx.collector_stats(s)["output_meta"][:20] == m.out_meta, s
        sizes.append(rule_bits(m.out_meta, host_bits[s]))
    return sizes


def frame_says(fr):
    """(sampleBytes, sampleBits) of a frame, its CRC held"""
    meta = np.ascontiguousarray(fr[0, 4:28]).tobytes()
    assert struct.unpack("<I", meta[20:24])[0] == zlib.crc32(meta[:20])
    return meta[8], meta[9]


def run_against_twins(ctx, oracle, calls, L, fcpos, R, arrays, want_mfma=False, follow_meta=False, primed=False):
    """the bank with the flag on against the twins; -> per stream the sampleBits bytes its frames said, in order"""
    import torch

    import sdrdaemon_amd as sd

    S = len(calls[0])
    cfg = dict(log2decim=L, fcpos=fcpos, nb_fec=R)
    bank = sd.RxPipe(ctx, S, center_frequency_khz=CFG_FC, sample_rate=CFG_RATE, sample_bits=CFG_BITS, **cfg)
    host_bits = HOST_BITS[:S] if arrays else [CFG_BITS] * S
    if arrays:
        bank.set_stream_bits(host_bits)
    bank.set_follow_bits()
    if follow_meta:
        bank.set_follow_meta()
    twins = make_twins(ctx, host_bits, **cfg)
    if primed:
        prime(bank, twins, L)
    models = [tg.Model(oracle) for _ in range(S)]
    said = [[] for _ in range(S)]
    for i, chunk in enumerate(calls):
        arg = [torch.from_numpy(c).cuda() for c in chunk] if i % 2 == 0 else chunk
        secs, usecs = ta.stamps(i, S)
        got = bank.process_datagrams(arg, secs, usecs)
        if want_mfma:
            plan = bank.last_plan()
            assert plan["path"] == "mfma" and plan["wps"] > 0, plan
        sizes = model_step(bank, models, chunk, host_bits)
        for s in range(S):
            assert bank.stream_bits(s) == (host_bits[s], tb.frame_bits(L, host_bits[s]))  # (the host's values, always)
            kw = dict(sample_bits=sizes[s])
            if follow_meta:
                kw["center_frequency_khz"], kw["sample_rate"] = tf.rule(models[s].out_meta, L, (CFG_FC, CFG_RATE))
            twins[s].reconfigure(**kw)
            (e, recs), = twins[s].process_datagrams([arg[s]], secs[s], usecs[s])
            g, e = tt.as_np(got[s][0]), tt.as_np(e)
            assert recs == got[s][1] and g.shape == e.shape, (i, s, g.shape, e.shape)
            assert g.tobytes() == e.tobytes(), (i, s, sizes[s])
            for f in g:
                sb, bits = frame_says(f)
                assert sb == (bits - 1) // 8 + 1, (i, s)
                if not follow_meta:
                    assert tf.meta_of(f)[:2] == (CFG_FC, CFG_RATE), (i, s)  # (the new flag alone: frequency and rate stay the host's)
                said[s].append(bits)
        assert list(bank.carry()) == [int(p.carry()[0]) for p in twins], i
    return said, host_bits


def check_kinds(said, host_bits, L, primed):
    """what the frames said, by kind: the followed size where the rule gives one, the host's where it does not"""
    fb = tb.frame_bits
    print("sampleBits said per stream", said)
    for s, kind in enumerate(KINDS):
        seen = said[s][1:] if primed else said[s]  # (a primed frame was opened by the sample-fed call: the host's size)
        assert len(said[s]) >= 2, (s, kind, said[s])
        if primed:
            assert said[s][0] == fb(L, host_bits[s]), (s, said[s])
        if kind in ("8", "12", "16"):
            assert set(seen) == {fb(L, int(kind))}, (s, seen)
        elif kind == "x":
            assert set(seen) <= {fb(L, min(max(16 - L - 1 + j, 1), 16)) for j in range(3)} and len(set(seen)) >= (2 if L < 4 else 1), (s, seen)
        elif kind == "c":
            assert set(seen) <= {fb(L, b) for b in C_BITS} and len(set(seen)) >= (2 if L < 4 else 1), (s, seen)
        elif kind == "d":
            assert set(seen) == {fb(L, D_BITS)}, (s, seen)
        else:  # e, z: the fallback
            assert set(seen) == {fb(L, host_bits[s])}, (s, kind, seen)


# ------------------------------------------------------------------------------------------------ 1. the bank against its twins
SHAPES = {0: (3, 3), 1: (3, 4), 4: (5, 4)}  # L -> incoming frames per call, calls
PATHS = {
    "decimate1": dict(L=0, arrays=True, opts={}),
    "decimate2_k1r": dict(L=1, arrays=False, opts={"decim_path": "valu"}),
    "decimate16_k1mr_direct": dict(L=4, arrays=True, opts={"decim_path": "mfma", "mfma_span": 1024, "rx_direct": "1"}),
    "decimate16_k1mr_k2r": dict(L=4, arrays=False, opts={"decim_path": "mfma", "mfma_span": 1024, "rx_direct": "0"}),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_bank_equals_reconfigured_one_stream_pipes(oracle, ctx, path):
    """8 streams of the kinds above; device and host datagrams alternate; stream 1 is fed nothing in call 1.  The fallback streams
    (e, z) run with the set_stream_bits array set (arrays) and with cfg.sample_bits alone.  A size that changes between two calls
    (c, x) does so under an open outgoing frame from decimate2 on: the twin's frame keeps the block 0 it was opened with, its
    samples take the new shift at once"""
    c = PATHS[path]
    L = c["L"]
    per_call, ncalls = SHAPES[L]
    for k, v in c["opts"].items():
        ctx.set_option(k, v)
    try:
        said, host_bits = run_against_twins(ctx, oracle, bits_calls(oracle, 700, L, per_call, ncalls), L, 2, 8, c["arrays"],
                                            want_mfma="k1mr" in path, primed=L >= 3)
        check_kinds(said, host_bits, L, L >= 3)
        if "k1mr" in path:
            assert ctx.option("rx_direct") == c["opts"]["rx_direct"]
    finally:
        for k in c["opts"]:
            ctx.set_option(k, RESTORE[k])


# ------------------------------------------------------------------------------------------------ 2. both flags
def test_both_flags_on(oracle, ctx):
    """KF behind KFb: the record it forms (frequency, rate >> log2decim, CRC) contains the followed bytes 8 and 9 -- against twins
    given frequency, rate and size"""
    L = 1
    per_call, ncalls = SHAPES[L]
    said, host_bits = run_against_twins(ctx, oracle, bits_calls(oracle, 700, L, per_call, ncalls), L, 2, 8, True, follow_meta=True)
    check_kinds(said, host_bits, L, False)


# ------------------------------------------------------------------------------------------------ 3. more than one wave of streams
def test_66_streams(oracle, ctx):
    """the second workgroup: stream s's sender says 1 + s % 16; at decimate1 the samples are the payload << (16 - size)"""
    import sdrdaemon_amd as sd

    S = 66
    rs = np.random.RandomState(66)
    chunk, pay = [], []
    for s in range(S):
        frames = incoming(oracle, rs, s, [1 + s % 16] * 2, 1, 7 * s, True)
        chunk.append(np.concatenate([frames[0][:128], frames[1][:128], tf.plain_frames(1, 7 * s + 2)[:1]]))
        pay.append([np.ascontiguousarray(f[1:128, 4:]).reshape(-1).view(np.int16) for f in frames])
    rx = sd.RxPipe(ctx, S, log2decim=0, nb_fec=1, sample_bits=16)
    rx.set_follow_bits()
    got = tr.run_call(rx, chunk, 12, 999999)
    for s in range(S):
        fr = got[s][0]
        b = 1 + s % 16
        assert fr.shape[0] == 3, (s, fr.shape)  # (the collector's initial slot and the two frames)
        for k, f in enumerate(fr):
            assert frame_says(f) == ((b - 1) // 8 + 1, b), (s, k, frame_says(f))
            if k:
                want = (pay[s][k - 1].astype(np.int32) << (16 - b)).astype(np.int16)
                assert np.array_equal(np.ascontiguousarray(f[1:128, 4:]).reshape(-1).view(np.int16), want), (s, k)
        if s in (0, 63, 64, 65):
            for f in fr:
                assert np.array_equal(f[128:], oracle.frame_encode(f[:128], 1)), s


# ------------------------------------------------------------------------------------------------ 4. asynchronous batches
def test_async_batches(oracle, ctx):
    """depth 3, three batches in flight, the flag toggled between the submits (on, off, on, on): a batch keeps the mode of its
    submit.  Byte equality with sdrhip_rx_process_datagrams on a twin bank that toggles between its calls; the link traffic of
    every submit equals that of a handle that never saw the flag"""
    import sdrdaemon_amd as sd

    S, L, R = 8, 0, 8
    calls = bits_calls(oracle, 700, L, 3, 4, idle=False)
    flags = [True, False, True, True]
    a, b, c = [sd.RxPipe(ctx, S, log2decim=L, nb_fec=R, sample_bits=CFG_BITS) for _ in range(3)]
    a.set_async(depth=3)
    c.set_async(depth=3)
    keep, exp, got, traffic = [], [], [], {"a": [], "c": []}

    def submit(p, name, i):
        sec, usec = ta.stamps(i, S)
        c0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        ta.submit_raw(ctx, p, calls[i], sec, usec, False, False, keep)
        traffic[name].append((ctx.counter("h2d_bytes") - c0[0], ctx.counter("d2h_bytes") - c0[1]))

    def step(i):
        sec, usec = ta.stamps(i, S)
        a.set_follow_bits(flags[i])
        b.set_follow_bits(flags[i])
        submit(a, "a", i)
        exp.append(b.process_datagrams(calls[i], sec, usec))
        assert list(a.carry()) == list(b.carry()), i

    for i in range(3):
        step(i)
    a.set_follow_bits(False)  # (every batch is in flight: they keep their modes)
    for i in range(3):
        got.append(a.collect_datagrams())
    step(3)
    got.append(a.collect_datagrams())
    for i in range(4):
        submit(c, "c", i)
        if i >= 2:
            c.collect_datagrams()
    for _ in range(2):
        assert c.collect_datagrams() is not None
    models = [tg.Model(oracle) for _ in range(S)]
    for i in range(4):
        for s in range(S):
            models[s].run(calls[i][s])
            g, e = np.asarray(got[i][s][0]), np.asarray(exp[i][s][0])
            assert got[i][s][1] == exp[i][s][1], (i, s)
            assert g.shape == e.shape and g.tobytes() == e.tobytes(), (i, s)
            assert g.shape[0] >= 2, (i, s)
            want = rule_bits(models[s].out_meta, CFG_BITS) if flags[i] else CFG_BITS
            assert all(frame_says(f)[1] == want for f in g), (i, s, want)  # (x1: every frame of a batch is opened by it)
    assert traffic["a"] == traffic["c"], traffic
    assert ta.mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 5. tagged submit, egress
def test_tagged_submit_and_egress_with_differing_fecblk(oracle, ctx):
    """submit_datagrams_tagged and collect_egress with set_stream_fec and set_stream_bits arrays and the flag on: array, tags and
    records equal the rounds over the twins' frames (each twin with its stream's fecblk and the rule's size)"""
    import sdrdaemon_amd as sd

    S, L = 8, 1
    fec = [0, 1, 32, 127, 4, 8, 2, 16]
    per_call, ncalls = SHAPES[L]
    calls = bits_calls(oracle, 700, L, per_call, ncalls)
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a = sd.RxPipe(ctx, S, nb_fec=8, center_frequency_khz=CFG_FC, sample_rate=CFG_RATE, sample_bits=CFG_BITS, **cfg)
    a.set_stream_fec(fec)
    a.set_stream_bits(HOST_BITS)
    a.set_follow_bits()
    a.set_async(depth=2)
    a.set_egress("round_robin")
    twins = make_twins(ctx, HOST_BITS, fec=fec, **cfg)
    models = [tg.Model(oracle) for _ in range(S)]
    total, followed = 0, 0
    for i, chunk in enumerate(calls):
        secs, usecs = ta.stamps(i, S)
        arr, tags = merge(chunk, 60 + i, skip=3)
        a.submit_datagrams_tagged(arr, tags, secs, usecs)
        exp = []
        for s in range(S):
            models[s].run(chunk[s])
            size = rule_bits(models[s].out_meta, HOST_BITS[s])
            followed += size != HOST_BITS[s]
            twins[s].reconfigure(sample_bits=size)
            exp.append(twins[s].process_datagrams([chunk[s]], secs[s], usecs[s])[0])
        dg, out_tags, nf, records = a.collect_egress()
        e_dg, e_tags = rounds([np.asarray(fr) for fr, _ in exp])
        assert list(nf) == [np.asarray(fr).shape[0] for fr, _ in exp], i
        assert dg.shape == e_dg.shape and np.array_equal(out_tags, e_tags) and dg.tobytes() == e_dg.tobytes(), i
        assert records == [r for _, r in exp], i
        total += int(sum(nf))
    assert total >= 2 * S and followed >= 12, (total, followed)
    assert ta.mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 6. reset of one stream
def test_reset_of_one_stream_falls_back_then_follows_again(oracle, ctx):
    """three streams whose senders say 8, decimate1.  Stream 1 loses every block 0 of call 2 (repaired).  Without a reset its
    m_outputMeta still says 8 and it goes on following; reset in front of call 2 its m_outputMeta is MetaDataFEC::init() again: the
    frames of call 2 say the host's size, those of call 3 (a block 0 released) 8 again"""
    import sdrdaemon_amd as sd

    S, per_call, ncalls = 3, 3, 4
    rs = np.random.RandomState(12)
    cut = []
    for s in range(S):
        frames = incoming(oracle, rs, s, [8] * (per_call * ncalls), 2, 50 * s, s != 2)
        dgs = [f[1:] if s == 1 and per_call * 2 <= k < per_call * 3 else f[:129] for k, f in enumerate(frames)]
        flat, starts = np.concatenate(dgs), np.cumsum([0] + [len(d) for d in dgs])
        # (cut at the frame boundary itself: call i holds exactly its own frames' datagrams, the last frame of a call is released by the next)
        cut.append([flat[starts[i * per_call]:starts[(i + 1) * per_call]] for i in range(ncalls)])
    calls = [[c[i] for c in cut] for i in range(ncalls)]
    for reset in (False, True):
        cfg = dict(log2decim=0, nb_fec=4)
        bank = sd.RxPipe(ctx, S, sample_bits=CFG_BITS, **cfg)
        bank.set_follow_bits()
        twins = make_twins(ctx, [CFG_BITS] * S, **cfg)
        models = [tg.Model(oracle) for _ in range(S)]
        said = []
        for i, chunk in enumerate(calls):
            if reset and i == 2:
                bank.reset_streams([1])
                twins[1].reset_streams()
                models[1] = tg.Model(oracle)
            got = tr.run_call(bank, chunk, 40 + i, 5, device=i % 2 == 1)
            sizes = model_step(bank, models, chunk, [CFG_BITS] * S)
            for s in range(S):
                twins[s].reconfigure(sample_bits=sizes[s])
                (e, recs), = twins[s].process_datagrams([chunk[s]], 40 + i, 5)
                assert recs == got[s][1] and got[s][0].tobytes() == tt.as_np(e).tobytes(), (reset, i, s)
            said.append([frame_says(f)[1] for f in got[1][0]])
        print("reset" if reset else "no reset", "stream 1 said", said)
        assert min(len(x) for x in said[1:]) >= 2, said
        assert set(said[1]) == {8} and set(said[3]) == {8}, said
        # (without the reset call 2 releases the last frame of call 1, whose block 0 arrived, and m_outputMeta goes on saying 8; the
        # reset drops that frame with the collector, and call 2 releases the initial slot and a frame whose block 0 was repaired)
        assert set(said[2]) == ({CFG_BITS} if reset else {8}), (reset, said)


# ------------------------------------------------------------------------------------------------ 7. cut invariance
def test_cut_invariance(oracle, ctx):
    """one datagram sequence per stream cut two ways that release the same frames in the same calls (the cuts move inside a
    frame): the same outgoing frames and the same m_outputMeta"""
    import sdrdaemon_amd as sd

    S, L, R = 8, 1, 8
    per_call, ncalls = SHAPES[L]
    runs, metas = [], []
    for off_seed in (0, 1):
        calls = bits_calls(oracle, 700, L, per_call, ncalls, off_seed, idle=False)
        rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R, sample_bits=CFG_BITS)
        rx.set_follow_bits()
        out = [[] for _ in range(S)]
        for i, chunk in enumerate(calls):
            got = tr.run_call(rx, chunk, 5, 6, device=i % 2 == 1)
            for s in range(S):
                out[s].append(got[s][0])
        runs.append([np.concatenate(o) for o in out])
        metas.append([rx.collector_stats(s)["output_meta"] for s in range(S)])
    a, b = bits_calls(oracle, 700, L, per_call, ncalls, 0, idle=False), bits_calls(oracle, 700, L, per_call, ncalls, 1, idle=False)
    assert any(a[1][s].shape != b[1][s].shape for s in range(S))  # (the cuts do differ)
    for s in range(S):
        assert runs[0][s].shape[0] >= 2
        assert np.array_equal(runs[0][s], runs[1][s]), s
        assert metas[0][s] == metas[1][s], s


# ------------------------------------------------------------------------------------------------ 8. the untouched default
def test_flag_off_is_untouched(oracle, ctx):
    """never touched, and set then cleared: equal bytes, the same plan, every frame says the host's size -- and differs from what
    the flag would give"""
    import sdrdaemon_amd as sd

    S, L, R = 8, 1, 8
    per_call, ncalls = SHAPES[L]
    calls = bits_calls(oracle, 700, L, per_call, ncalls)[:3]
    plain, cleared, on = [sd.RxPipe(ctx, S, log2decim=L, nb_fec=R, sample_bits=CFG_BITS) for _ in range(3)]
    cleared.set_follow_bits()
    cleared.set_follow_bits(False)
    on.set_follow_bits()
    total, differ = 0, 0
    for i, chunk in enumerate(calls):
        p, q, r = tr.run_call(plain, chunk, 8, i), tr.run_call(cleared, chunk, 8, i), tr.run_call(on, chunk, 8, i)
        assert plain.last_plan() == cleared.last_plan()
        for s in range(S):
            assert p[s][1] == q[s][1] and np.array_equal(p[s][0], q[s][0]), (i, s)
            assert all(frame_says(f)[1] == tb.frame_bits(L, CFG_BITS) for f in p[s][0]), (i, s)
            total += p[s][0].shape[0]
            differ += p[s][0].shape == r[s][0].shape and not np.array_equal(p[s][0], r[s][0])
    assert total >= S and differ >= 5, (total, differ)
