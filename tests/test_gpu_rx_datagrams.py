"""The Rx pipe fed raw FEC datagrams (sdrhip_rx_process_datagrams) against the hub chain, stream by stream: the reference's own
SDRdaemonFECBuffer (oracle/_ref/libsdrref_fecbuf_hip.so) fed datagram by datagram, its released payloads appended to a Python
remainder buffer, the largest multiple of the decimation unit through the compiled-reference (or oracle) decimators, the oracle
framer with the call's stamps and frame_encode.  Bit-exact everywhere: frames, recovery blocks, meta blocks, frameIndex; the
records must equal a FECBufferBank's on the same calls."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_tx_datagrams as tt

pytestmark = pytest.mark.gpu

F = 16129
ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)
reflib = tt.reflib


@pytest.fixture(autouse=True, scope="module")
def torch_first():
    """torch brings its device runtime up before the reference's FEC buffer library is first used (the order every test of
    test_gpu_tx_datagrams keeps: device tensors first, RefChain afterwards); the other way round torch finds no device"""
    import torch

    torch.zeros(1).cuda()


def unit(L, fcpos):
    return 4 if L == 1 and fcpos != 2 else 1 << L


class HubChain:
    """one stream of the hub: SDRdaemonFECBuffer -> remainder buffer -> Downsampler -> UDPSinkFEC framing -> cm256_encode"""

    def __init__(self, lib, oracle, hb=0, sample_rate=625000):
        from oracle_lib import Reference

        self.lib, self.oracle = lib, oracle
        self.col = tt.RefChain(lib, oracle)
        flavour = "db" if hb else "eo1"
        self.dec = Reference(flavour).decimators() if Reference.available(flavour) else oracle.decimators(hb)
        self.fr = oracle.framer(center_frequency_khz=435000, sample_rate=sample_rate)
        self.rem = np.zeros((0, 2), np.int16)

    def reset_collector(self):
        self.col = tt.RefChain(self.lib, self.oracle)
        self.rem = np.zeros((0, 2), np.int16)

    def samples(self, x, L, fcpos, R, sec, usec):
        """sample-fed call (sdrhip_rx_process_ragged): past the remainder buffer"""
        if len(x) >> L == 0:
            return []
        y, ss = self.dec.decimate(L, fcpos, 16, np.ascontiguousarray(x))
        s = self.fr.s
        s.nb_fec_blocks, s.sample_bytes, s.sample_bits, s.tv_sec, s.tv_usec = R, (ss - 1) // 8 + 1, ss, sec, usec
        return [np.concatenate([f, self.oracle.frame_encode(f, R)]) if R else f for f in self.fr.write(y)]

    def dgrams(self, dg, L, fcpos, R, sec, usec):
        pay = self.col.collect(dg)
        if pay:
            self.rem = np.concatenate([self.rem] + [p.view(np.int16).reshape(-1, 2) for p in pay])
        n = len(self.rem) // unit(L, fcpos) * unit(L, fcpos)
        x, self.rem = self.rem[:n], self.rem[n:]
        return self.samples(x, L, fcpos, R, sec, usec)


def run_call(rx, chunk, sec=0, usec=0, device=True, bank=None, max_released=None):
    """chunk: per stream an (n, 512) uint8 array -> per stream (frames, records) as numpy"""
    import torch

    arg = [torch.from_numpy(c).cuda() for c in chunk] if device else chunk
    got = [(tt.as_np(fr), recs) for fr, recs in rx.process_datagrams(arg, sec, usec, max_released)]
    if bank is not None:
        ref = bank.write_and_read(arg)
        for s, (_, recs) in enumerate(got):
            assert recs == ref[s][2], s
    return got


def check_frames(got, exp, where):
    assert got.shape[0] == len(exp), (where, got.shape[0], len(exp))
    for f, e in enumerate(exp):
        assert np.array_equal(got[f], e), (where, f)


def prime(pipes, chains, L, fcpos, R, sec=0, usec=0, short=300):
    """a sample-fed call that leaves every stream's open frame `short` decimated samples from full, so that the few payloads a
    test can afford complete frames at high decimation too (sample-fed calls go past the remainder buffer: HubChain.samples).
    pipes: one bank, or one-stream handles"""
    S, n = len(chains), (F - short) << L
    x = np.random.RandomState(5).randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)
    if len(pipes) == 1:
        _, nf = pipes[0].process_ragged(x, [n] * S, sec, usec)
        assert not nf.any()
    else:
        for s, p in enumerate(pipes):
            assert not p.process_ragged(x[s:s + 1], [n], sec, usec)[1].any()
    for s, c in enumerate(chains):
        assert c.samples(x[s], L, fcpos, R, sec, usec) == []


_CALLS = {}


def bank_calls(oracle, seed, S=8, ncalls=4, nframes=(3, 7)):
    """tt.bank_calls (incoming fecblk 1 / 32 / 64 / 127, random losses, lost recovery rows on streams 6 and 7), kept per seed"""
    key = (seed, S, ncalls, nframes)
    if key not in _CALLS:
        _CALLS[key] = tt.bank_calls(oracle, seed, S=S, ncalls=ncalls, nframes=nframes)
    return _CALLS[key]


CASES = [(L, 2) for L in range(7)] + [(L, fc) for L in (1, 2, 4) for fc in (0, 1)]


@pytest.mark.parametrize("hb", [0, 1])
@pytest.mark.parametrize("L,fcpos", CASES)
def test_parity_with_the_reference_chain(oracle, ctx, reflib, L, fcpos, hb):
    """8 streams, incoming fecblk 1 / 32 / 64 / 127 with random losses, 3-4 calls cut at random points; every decimation and
    position with both half-band variants, outgoing nb_fec 8 and 32 alternating over the cases"""
    import sdrdaemon_amd as sd

    S = 8
    R = 8 if (L + fcpos + hb) % 2 else 32
    calls = bank_calls(oracle, 300 + L % 2, ncalls=3 + L % 2)
    rx = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, hb_variant=hb, nb_fec=R)
    bank = sd.FECBufferBank(ctx, S)
    chains = [HubChain(reflib, oracle, hb) for _ in range(S)]
    if L >= 3:
        prime([rx], chains, L, fcpos, R, 999, 1)
    total, held = 0, 0
    for i, chunk in enumerate(calls):
        secs, usecs = [1000 + 10 * i + s for s in range(S)], [37 * i + s for s in range(S)]
        got = run_call(rx, chunk, secs, usecs, bank=bank)
        for s in range(S):
            check_frames(got[s][0], chains[s].dgrams(chunk[s], L, fcpos, R, secs[s], usecs[s]), (L, fcpos, hb, i, s))
            total += got[s][0].shape[0]
        assert list(rx.carry()) == [len(c.rem) for c in chains]
        held += int(rx.carry().sum())
    assert total >= S and (held > 0 or L == 0)


@pytest.mark.parametrize("L,fcpos", [(1, 0), (3, 2), (6, 2)])
def test_cut_invariance(oracle, ctx, reflib, L, fcpos):
    """one datagram sequence per stream cut into 1, 3 and 7 calls: the same frames, the same carry at the end"""
    import sdrdaemon_amd as sd

    S = 4
    rs = np.random.RandomState(41 + L)
    per = [tt.stream_dgrams(oracle, rs, 4 + s % 2, [32, 64][s % 2], lose_rows=40 if s == 3 else 0) for s in range(S)]
    runs, carries, mid = [], [], 0
    for ncalls in (1, 3, 7):
        rs = np.random.RandomState(7 * ncalls)
        cut = [tt.split(rs, per[s], ncalls) for s in range(S)]
        rx = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, nb_fec=8, sample_rate=0)
        if L >= 3:
            prime([rx], [HubChain(reflib, oracle, sample_rate=0) for _ in range(S)], L, fcpos, 8, 5, 6)
        out = [[] for _ in range(S)]
        for i in range(ncalls):
            got = run_call(rx, [cut[s][i] for s in range(S)], 5, 6)
            for s in range(S):
                out[s].append(got[s][0])
            if i < ncalls - 1:
                mid += int(rx.carry().sum())
        runs.append([np.concatenate(o) for o in out])
        carries.append(list(rx.carry()))
    assert mid > 0  # (some intermediate call held samples back: what the sample-fed entries would have dropped)
    for s in range(S):
        assert runs[0][s].shape[0] >= 1
        assert np.array_equal(runs[0][s], runs[1][s]) and np.array_equal(runs[0][s], runs[2][s]), s
    assert carries[0] == carries[1] == carries[2]


def test_bank_equals_one_stream_handles(oracle, ctx, reflib):
    import sdrdaemon_amd as sd

    S, L = 8, 3
    calls = bank_calls(oracle, 300, ncalls=3)
    bank = sd.RxPipe(ctx, S, log2decim=L, nb_fec=32)
    ones = [sd.RxPipe(ctx, 1, log2decim=L, nb_fec=32) for _ in range(S)]
    prime([bank], [HubChain(reflib, oracle) for _ in range(S)], L, 2, 32)
    prime(ones, [HubChain(reflib, oracle) for _ in range(S)], L, 2, 32)
    total = 0
    for i, chunk in enumerate(calls):
        got = run_call(bank, chunk, [i + s for s in range(S)], 9)
        for s in range(S):
            (fr, recs), = run_call(ones[s], [chunk[s]], i + s, 9)
            assert recs == got[s][1] and np.array_equal(fr, got[s][0]), (i, s)
            total += fr.shape[0]
        assert list(bank.carry()) == [int(o.carry()[0]) for o in ones]
    assert total >= S


def test_einval_retry(oracle, ctx, reflib):
    import torch

    import sdrdaemon_amd as sd

    S, L = 8, 1
    calls = bank_calls(oracle, 301, ncalls=4)[:2]
    cfg = dict(log2decim=L, nb_fec=32)
    free = sd.RxPipe(ctx, S, **cfg)
    rx = sd.RxPipe(ctx, S, **cfg)
    chains = [HubChain(reflib, oracle) for _ in range(S)]
    full = [run_call(free, c, 3, 4) for c in calls]
    need = [len(x[1]) for x in full[1]]
    assert max(need) >= 2
    got = [run_call(rx, calls[0], 3, 4)]
    before = list(rx.carry())
    with pytest.raises(sd.SdrHipError) as e:
        rx.process_datagrams([torch.from_numpy(c).cuda() for c in calls[1]], 3, 4, max_released=max(need) - 1)
    assert e.value.code == -1 and rx.last_n_released == need and list(rx.carry()) == before
    # a frame stride too small for the stream with the most frames: the same refusal, nothing consumed
    buf, counts, _ = sd.engine._datagram_batch(calls[1])
    most = max(x[0].shape[0] for x in full[1])
    assert most >= 1
    fb = (128 + 32) * 512
    out = np.zeros((S, most, 160, 512), np.uint8)
    info = (sd.engine.FECBufferFrame * (S * max(need)))()
    nd, nr, nf = (C.c_size_t * S)(*counts), (C.c_size_t * S)(), (C.c_size_t * S)()
    st = (C.c_uint32 * S)(*[3] * S)
    rc = ctx.lib.sdrhip_rx_process_datagrams(rx.h, buf.ctypes.data, nd, buf.shape[1] * 512, st, st, max(need), out.ctypes.data,
                                             most * fb - 1, info, nr, nf, sd.MEM_HOST)
    assert rc == -1 and list(nr) == need and list(rx.carry()) == before
    got.append(run_call(rx, calls[1], 3, 4))
    for i in range(2):
        for s in range(S):
            assert np.array_equal(got[i][s][0], full[i][s][0]) and got[i][s][1] == full[i][s][1], (i, s)
            check_frames(got[i][s][0], chains[s].dgrams(calls[i][s], L, 2, 32, 3, 4), (i, s))


def test_host_memory_equals_device_memory_and_moves_no_samples(oracle, ctx):
    """host calls give the device calls' bytes, and the link carries datagrams up and frames down: what remains is far below one
    payload round trip (64 516 bytes per released frame)"""
    import sdrdaemon_amd as sd

    S, L, R = 8, 2, 8
    calls = bank_calls(oracle, 300, ncalls=3)
    dev, host = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R), sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    big = 0
    for i, chunk in enumerate(calls):
        a = run_call(dev, chunk, 8, i)
        ctx.synchronize()
        up0, down0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        released = max(sum(len(x[1]) for x in a), 0)
        b = run_call(host, chunk, 8, i, device=False, max_released=max(len(x[1]) for x in a))
        up, down = ctx.counter("h2d_bytes") - up0, ctx.counter("d2h_bytes") - down0
        for s in range(S):
            assert a[s][1] == b[s][1] and np.array_equal(a[s][0], b[s][0]), (i, s)
        nframes, ndg = sum(x[0].shape[0] for x in b), sum(c.shape[0] for c in chunk)
        bound = 1024 * (released + S)
        print("call %d: released %d, frames %d, d2h %d (frames %d), h2d %d (datagrams %d), bound %d"
              % (i, released, nframes, down, nframes * (128 + R) * 512, up, 512 * ndg, bound))
        assert 0 <= down - nframes * (128 + R) * 512 < bound
        assert 0 <= up - 512 * ndg < bound
        big = max(big, released)
    assert big >= 16


def test_mixed_with_sample_fed_calls_reconfigure_and_reset(oracle, ctx, reflib):
    import sdrdaemon_amd as sd

    S = 4
    calls = bank_calls(oracle, 302, S=S, ncalls=6, nframes=(6, 9))
    rs = np.random.RandomState(9)
    cfg = dict(L=3, fcpos=2, R=16)
    rx = sd.RxPipe(ctx, S, log2decim=3, fcpos=2, nb_fec=16)
    chains = [HubChain(reflib, oracle) for _ in range(S)]

    def dg(i):
        got = run_call(rx, calls[i], 20 + i, i)
        for s in range(S):
            check_frames(got[s][0], chains[s].dgrams(calls[i][s], cfg["L"], cfg["fcpos"], cfg["R"], 20 + i, i), ("dg", i, s))
        assert list(rx.carry()) == [len(c.rem) for c in chains]

    def ragged(counts, sec):
        x = rs.randint(-32768, 32768, size=(S, max(counts), 2)).astype(np.int16)
        held = list(rx.carry())
        g, nf = rx.process_ragged(x, counts, sec, 1)
        for s in range(S):
            check_frames(g[s, :nf[s]], chains[s].samples(x[s, :counts[s]], cfg["L"], cfg["fcpos"], cfg["R"], sec, 1), ("ragged", sec, s))
        assert list(rx.carry()) == held  # (sample-fed calls neither read nor clear the remainder)

    def reconf(**kw):
        assert int(rx.carry().sum()) > 0  # (a remainder is held across the change)
        rx.reconfigure(**{dict(L="log2decim", R="nb_fec", fcpos="fcpos")[k]: v for k, v in kw.items()})
        cfg.update(kw)

    dg(0)
    ragged([(F << 3) // 2 + 3, 0, (F << 3) + 9, 17], 40)
    dg(1)
    reconf(L=5)
    dg(2)
    ragged([5, (F << 5), 64, 0], 41)
    reconf(R=40)
    dg(3)
    reconf(L=1, fcpos=0)  # (U = 4: a remainder of up to 31 samples feeds whole fours on the next call)
    dg(4)
    for s in range(S):
        assert rx.collector_stats(s)["cur_nb_blocks"] >= 0
    rx.reset_collector()
    assert list(rx.carry()) == [0] * S
    for c in chains:
        c.reset_collector()
    dg(5)


def test_mode_guards(oracle, ctx, reflib):
    import torch

    import sdrdaemon_amd as sd

    S, L = 4, 4
    calls = bank_calls(oracle, 303, S=S, ncalls=3)
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=32)
    chains = [HubChain(reflib, oracle) for _ in range(S)]

    def good(i):
        got = run_call(rx, calls[i], 1, 2)
        for s in range(S):
            check_frames(got[s][0], chains[s].dgrams(calls[i][s], L, 2, 32, 1, 2), (i, s))

    arg = [torch.from_numpy(c).cuda() for c in calls[1]]
    # pipelined mode (while the streams still stand together): refused, nothing consumed
    tt.check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 1))
    with pytest.raises(sd.SdrHipError) as e:
        rx.process_datagrams(arg, 1, 2)
    assert e.value.code == -1
    tt.check(ctx.lib.sdrhip_rx_set_pipelined(rx.h, 0))
    prime([rx], chains, L, 2, 32, 1, 2)
    good(0)
    held = list(rx.carry())
    # a ragged batch being filled: refused, nothing consumed; the batch itself goes through the same histories
    rx.set_async(depth=2, blocks=2)
    x = np.random.RandomState(3).randint(-32768, 32768, size=(S, 64 << L, 2)).astype(np.int16)
    rx.submit_ragged(x, [64 << L] * S, 1, 2)
    with pytest.raises(sd.SdrHipError) as e:
        rx.process_datagrams(arg, 1, 2)
    assert e.value.code == -1 and list(rx.carry()) == held
    batch = rx.collect_ragged(wait=True)
    for s in range(S):
        check_frames(batch[s], chains[s].samples(x[s], L, 2, 32, 1, 2), ("batch", s))
    good(1)
    good(2)


def test_realistic_shape(oracle, ctx, reflib):
    """8 streams x 16 released frames in one call at decimate16_cen, nb_fec 32 (whatever path the planner takes)"""
    import sdrdaemon_amd as sd

    S, L, R = 8, 4, 32
    rs = np.random.RandomState(77)
    per = []
    for s in range(S):
        dg = []
        for f in tg.make_frames(oracle, rs, 16, 32, int(rs.randint(0, 65536))):
            lost = set(rs.choice(160, 24, replace=False).tolist())
            dg += [f[i] for i in range(160) if i not in lost]
        dg.append(np.full(512, 0xEE, np.uint8))
        per.append(np.asarray(dg, np.uint8))
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    chains = [HubChain(reflib, oracle) for _ in range(S)]
    total = 0
    for i in range(2):  # (the second call: the trailing datagram's frame is released, one more payload each)
        got = run_call(rx, per, 100 + i, 0)
        print("call %d plan:" % i, rx.last_plan(), "carry", list(rx.carry()))
        for s in range(S):
            assert len(got[s][1]) == 17
            check_frames(got[s][0], chains[s].dgrams(per[s], L, 2, R, 100 + i, 0), (i, s))
            total += got[s][0].shape[0]
    assert total == S * 2  # (34 payloads of 16129 samples / 16 = 2.125 frames)
