"""The Tx pipe fed raw datagrams (sdrhip_tx_process_datagrams) against sdrdaemontx's receive chain, stream by stream: the
reference's own SDRdaemonFECBuffer (oracle/_ref/libsdrref_fecbuf_hip.so) fed datagram by datagram, its released getSlotData
concatenated, then the oracle's interpolators (pinned to the compiled reference by the goldens).  Records and meta blocks must
equal the FEC buffer bank's on the same input."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_ref_fecbuffer as tr

pytestmark = pytest.mark.gpu


class RefChain:
    """one stream of sdrdaemontx: the reference's SDRdaemonFECBuffer + the oracle's interpolators (one Upsampler)"""

    def __init__(self, lib, oracle):
        self.lib = lib
        self.h = C.c_void_p(lib.sdrref_fecbuf_new())
        self.itp = oracle.interpolators()
        self.first = True
        self.data = np.zeros(127 * 508, np.uint8)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.sdrref_fecbuf_free(self.h)
            self.h = None

    def collect(self, dgrams):
        out = []
        ln = C.c_size_t(0)
        for d in dgrams:
            d = np.ascontiguousarray(d, np.uint8)
            if self.lib.sdrref_fecbuf_write_and_read(self.h, d.ctypes.data, self.data.ctypes.data, C.byref(ln)):
                # (the initial slot: uninitialised memory in the reference, zero in the library -- include/sdrhip.h)
                out.append(np.zeros(127 * 508, np.uint8) if self.first else self.data.copy())
                self.first = False
        return out

    def interpolate(self, frames, log2interp):
        if not len(frames):
            return np.zeros((0, 2), np.int16)
        return self.itp.interpolate(log2interp, np.concatenate(frames).view(np.int16).reshape(-1, 2))

    def feed(self, dgrams, log2interp):
        return self.interpolate(self.collect(dgrams), log2interp)


@pytest.fixture
def ctx():
    import sdrdaemon_amd as sd

    assert sd.device_count() > 0
    c = sd.Context(0)
    c.set_option("dec_strict", 1)  # (the reference's copy-back holes)
    return c


@pytest.fixture(scope="module")
def reflib():
    return tr._load("libsdrref_fecbuf_hip.so")


def stream_dgrams(oracle, rs, nframes, R, lose_rows=0):
    """nframes frames of 128 + R blocks with random losses (lose_rows: recovery rows 0 .. lose_rows - 1 lost as well, so that the
    decoder needs rows >= 32), then one datagram of the next frame (it releases the last one)"""
    dg = []
    for fr in tg.make_frames(oracle, rs, nframes, R, int(rs.randint(0, 65536))):
        lost = set(rs.choice(128, int(rs.randint(0, max(R - lose_rows, 1) + 1)), replace=False).tolist())
        lost |= set(range(128, 128 + min(lose_rows, R)))
        dg += [fr[i] for i in range(128 + R) if i not in lost]
    if nframes:
        dg.append(np.full(512, 0xEE, np.uint8))
    return dg


def split(rs, dg, ncalls):
    """a stream's datagrams cut into ncalls pieces at random points (pieces may be empty)"""
    cuts = sorted(rs.randint(0, len(dg) + 1, ncalls - 1).tolist()) if dg else [0] * (ncalls - 1)
    b = [0] + cuts + [len(dg)]
    return [np.asarray(dg[b[i]:b[i + 1]], np.uint8).reshape(-1, 512) for i in range(ncalls)]


def as_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run_calls(tx, calls, device=True, bank=None, max_frames=None):
    """calls: per call, per stream an (n, 512) uint8 array -> per call, per stream (iq, block0, records) as numpy"""
    import torch

    out = []
    for chunk in calls:
        arg = [torch.from_numpy(c).cuda() for c in chunk] if device else chunk
        res = tx.process_datagrams(arg, max_frames)
        got = [(as_np(iq), as_np(b0), recs) for iq, b0, recs in res]
        if bank is not None:
            ref = bank.write_and_read(arg)
            for s, (_, b0, recs) in enumerate(got):
                assert recs == ref[s][2], s
                assert np.array_equal(b0, as_np(ref[s][1])), s
        out.append(got)
    return out


def check_chain(got, chains, calls, log2interp):
    for i, chunk in enumerate(calls):
        for s, ch in enumerate(chains):
            exp = ch.feed(chunk[s], log2interp)
            iq = got[i][s][0]
            assert iq.shape == exp.shape, (i, s, iq.shape, exp.shape)
            assert np.array_equal(iq, exp), (i, s, int(np.argmax(np.any(iq != exp, axis=1))))


def bank_calls(oracle, seed, S=8, ncalls=4, nframes=(3, 7)):
    rs = np.random.RandomState(seed)
    Rs = [1, 32, 64, 127]
    per = []
    for s in range(S):
        R = Rs[s % 4]
        per.append(split(rs, stream_dgrams(oracle, rs, int(rs.randint(*nframes)), R, lose_rows=40 if R >= 64 and s % 8 >= 4 else 0), ncalls))
    return [[per[s][i] for s in range(S)] for i in range(ncalls)]


@pytest.mark.parametrize("log2interp", [0, 1, 2, 3, 4, 5, 6])
def test_parity_with_the_reference_chain(oracle, ctx, reflib, log2interp):
    import sdrdaemon_amd as sd

    calls = bank_calls(oracle, 100 + log2interp, ncalls=3 + log2interp % 2)
    tx = sd.TxPipe(ctx, 8, log2interp)
    got = run_calls(tx, calls, bank=sd.FECBufferBank(ctx, 8))
    assert any(len(got[i][s][2]) > 1 for i in range(len(calls)) for s in range(8))
    check_chain(got, [RefChain(reflib, oracle) for _ in range(8)], calls, log2interp)


@pytest.mark.parametrize("path,log2interp", [("wave", 2), ("wave", 6), ("valu", 1), ("valu", 4)])
def test_ragged_extremes(oracle, ctx, reflib, path, log2interp):
    """stream 0 never releases a frame, stream 1 alternates nothing / many, stream 2 starts in the last call; segments of 256
    inputs: many segments per stream and ragged segment ends"""
    import sdrdaemon_amd as sd

    ctx.set_option("interp_path", path)
    ctx.set_option("interp_span", 256)
    rs = np.random.RandomState(7)
    S, ncalls = 5, 4
    empty = np.zeros((0, 512), np.uint8)
    per = [[empty] * ncalls]
    d1 = split(rs, stream_dgrams(oracle, rs, 6, 32), 2)
    per.append([d1[0], empty, d1[1], empty])
    per.append([empty] * (ncalls - 1) + [np.asarray(stream_dgrams(oracle, rs, 3, 64, 36), np.uint8).reshape(-1, 512)])
    for s in range(3, S):
        per.append(split(rs, stream_dgrams(oracle, rs, 4, 32), ncalls))
    calls = [[per[s][i] for s in range(S)] for i in range(ncalls)]
    tx = sd.TxPipe(ctx, S, log2interp)
    got = run_calls(tx, calls)
    assert all(got[i][0][0].shape[0] == 0 for i in range(ncalls))
    check_chain(got, [RefChain(reflib, oracle) for _ in range(S)], calls, log2interp)


def test_einval_retry(oracle, ctx, reflib):
    import sdrdaemon_amd as sd

    calls = bank_calls(oracle, 31, ncalls=2)
    full = run_calls(sd.TxPipe(ctx, 8, 4), calls)
    tx = sd.TxPipe(ctx, 8, 4)
    got = run_calls(tx, calls[:1])
    need = [len(x[2]) for x in full[1]]
    assert max(need) >= 2
    import torch

    with pytest.raises(sd.SdrHipError) as e:
        tx.process_datagrams([torch.from_numpy(c).cuda() for c in calls[1]], max_frames=max(need) - 1)
    assert e.value.code == -1 and tx.last_n_frames == need
    got += run_calls(tx, calls[1:])
    for i in range(len(calls)):
        for s in range(8):
            assert np.array_equal(got[i][s][0], full[i][s][0]), (i, s)
            assert got[i][s][2] == full[i][s][2]
    check_chain(got, [RefChain(reflib, oracle) for _ in range(8)], calls, 4)


def test_host_device_reconfigure_and_tx_process(oracle, ctx, reflib):
    """host and device memory agree; sdrhip_tx_reconfigure between datagram calls and sdrhip_tx_process calls in between feed the
    same histories, like the reference's one Upsampler per stream"""
    import torch

    import sdrdaemon_amd as sd

    S = 4
    calls = bank_calls(oracle, 57, S=S, ncalls=4)
    rs = np.random.RandomState(58)
    steps = [("dg", 0, 3), ("rx", None, 3), ("dg", 1, 5), ("dg", 2, 5), ("rx", None, 2), ("dg", 3, 4)]
    frames = {k: [tg.make_frames(oracle, rs, 2, 0, 100 * k + s) for s in range(S)] for k in range(len(steps))}
    res = {}
    for device in (True, False):
        tx = sd.TxPipe(ctx, S, 3)
        outs = []
        for k, (kind, i, L) in enumerate(steps):
            assert tx.configure({"interp": L})
            if kind == "dg":
                outs.append([x[0] for x in run_calls(tx, [calls[i]], device=device)[0]])
            else:
                rx = np.stack([np.stack(frames[k][s]) for s in range(S)])
                o = tx.process(torch.from_numpy(rx).cuda() if device else rx)
                outs.append([as_np(o[s]) for s in range(S)])
        res[device] = outs
    for k in range(len(steps)):
        for s in range(S):
            assert np.array_equal(res[True][k][s], res[False][k][s]), (k, s)
    chains = [RefChain(reflib, oracle) for _ in range(S)]
    for k, (kind, i, L) in enumerate(steps):
        for s in range(S):
            if kind == "dg":
                exp = chains[s].feed(calls[i][s], L)
            else:
                exp = chains[s].interpolate([f[1:128, 4:].reshape(-1) for f in frames[k][s]], L)
            assert np.array_equal(res[True][k][s], exp), (k, s)


def test_mode_guards_and_collector_stats(oracle, ctx, reflib):
    import torch

    import sdrdaemon_amd as sd

    S = 4
    calls = bank_calls(oracle, 77, S=S, ncalls=3)
    tx = sd.TxPipe(ctx, S, 2)
    bank = sd.FECBufferBank(ctx, S)
    chains = [RefChain(reflib, oracle) for _ in range(S)]
    got = run_calls(tx, calls[:1], bank=bank)
    check_chain(got, chains, calls[:1], 2)
    arg = [torch.from_numpy(c).cuda() for c in calls[1]]
    # pipelined: refused, nothing consumed
    check(ctx.lib.sdrhip_tx_set_pipelined(tx.h, 1))
    with pytest.raises(sd.SdrHipError) as e:
        tx.process_datagrams(arg)
    assert e.value.code == -1
    check(ctx.lib.sdrhip_tx_set_pipelined(tx.h, 0))
    # an asynchronous batch in flight: refused, nothing consumed; the batch itself goes through the same histories
    rs = np.random.RandomState(78)
    fr = [tg.make_frames(oracle, rs, 1, 0, 500 + s) for s in range(S)]
    tx.set_async(2)
    tx.submit(np.stack([np.stack(f) for f in fr]))
    with pytest.raises(sd.SdrHipError) as e:
        tx.process_datagrams(arg)
    assert e.value.code == -1
    a = tx.collect()
    for s in range(S):
        assert np.array_equal(a[s], chains[s].interpolate([fr[s][0][1:128, 4:].reshape(-1)], 2)), s
    got = run_calls(tx, calls[1:], bank=bank)
    check_chain(got, chains, calls[1:], 2)
    for s in range(S):
        assert tx.collector_stats(s) == bank.stats(s), s


def check(rc):
    from sdrdaemon_amd._lib import check as chk

    chk(rc)


@pytest.mark.parametrize("R,lose_rows", [(32, 0), (64, 36)])
def test_bench_shape(oracle, ctx, reflib, R, lose_rows):
    """64 streams x 16 frames at x16 in one call: samples by SHA-256 against the reference chain; rows < 32 and rows >= 32"""
    import torch

    import sdrdaemon_amd as sd

    rs = np.random.RandomState(5 + R)
    S = 64
    per = []
    for s in range(S):
        dg = []
        for f in tg.make_frames(oracle, rs, 16, R, int(rs.randint(0, 65536))):
            lost = set(rs.choice(128 + R, 24, replace=False).tolist()) if not lose_rows else \
                set(rs.choice(128, 20, replace=False).tolist()) | set(range(128, 128 + lose_rows))
            dg += [f[i] for i in range(128 + R) if i not in lost]
        dg.append(np.full(512, 0xEE, np.uint8))
        per.append(np.asarray(dg, np.uint8))
    tx = sd.TxPipe(ctx, S, 4)
    res = tx.process_datagrams([torch.from_numpy(p).cuda() for p in per])
    assert all(len(r[2]) == 17 for r in res)
    if lose_rows:
        assert all(r["recovery_count"] >= 20 for x in res for r in x[2][1:])
    for s in range(S):
        exp = RefChain(reflib, oracle).feed(per[s], 4)
        iq = res[s][0].cpu().numpy()
        assert iq.shape == exp.shape
        assert hashlib.sha256(iq.tobytes()).hexdigest() == hashlib.sha256(exp.tobytes()).hexdigest(), s
