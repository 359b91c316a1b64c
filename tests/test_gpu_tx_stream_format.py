"""Per-stream output format of the Tx pipe (sdrhip_tx_set_stream_format / TxPipe.set_stream_formats): HackRF (int8) and int16 sinks in
one bank, K5x / K6x (interp_mixed_kernels.hip).

The expected bytes are always those of one-stream TxPipe twins with output_format = fmt[s] fed the same input, call after call; for
stream 0 they are also the oracle's interpolators, with >> 8 where the stream is S8 (HackRFSink.cpp:671-672).  The handle under test
is never its own yardstick."""
import ctypes as C

import numpy as np
import pytest
import torch

import sdrdaemon_amd as sd
import test_gpu_dgram_tagged as tgt
import test_gpu_iq8 as iq8
import test_gpu_tx_datagrams as tdg

pytestmark = pytest.mark.gpu

EINVAL, EALIGN = -1, -4
NF = 16129  # samples per frame
DT = {"s16": np.int16, "s8": np.int8}
SENT = 0x5A


@pytest.fixture
def ctx():
    assert sd.device_count() > 0
    return sd.Context(0)


_batches = {}


def batch(oracle, S, F, seed):
    """tx_batch of test_gpu_iq8, computed once per shape and shared (never written to)"""
    key = (S, F, seed)
    if key not in _batches:
        _batches[key] = iq8.tx_batch(oracle, np.random.RandomState(seed), S, F)
    return _batches[key]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def twin(ctx, fmt, L, **kw):
    return sd.TxPipe(ctx, 1, L, output_format=fmt, **kw)


def same(got, exp, where=""):
    """a list of per-stream arrays against the twins' (n, 2) arrays: dtype, shape, bytes"""
    assert len(got) == len(exp), where
    for s, (g, e) in enumerate(zip(got, exp)):
        g, e = host(g), host(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (where, s, g.dtype, e.dtype, g.shape, e.shape)
        assert np.array_equal(g, e), (where, s)


# --------------------------------------------------------------------------- 1. synchronous parity
FORMAT_SETS = (["s16", "s8", "s16"], ["s8", "s16", "s8"], ["s8"] * 3, ["s16"] * 3)


@pytest.mark.parametrize("L,path,S,F", [(L, "wave", 3, 1) for L in range(7)] + [(L, "valu", 3, 1) for L in (3, 4, 6)] +
                         [(4, "wave", 3, 3), (2, "wave", 1, 1)])
def test_sync_parity(ctx, oracle, L, path, S, F):
    """host and device memory, two calls in a row on one handle (the histories carry over); 16 129 samples per frame: the odd end"""
    ctx.set_option("interp_path", path)
    rx, ys = batch(oracle, 3, F, 40 + F)
    rx, ys = rx[:S], ys[:S]
    rxd = torch.from_numpy(np.ascontiguousarray(rx)).cuda()
    # the twins: every stream in both formats, the host call then the device call
    tw = {}
    for s in range(S):
        for f in ("s16", "s8"):
            t = twin(ctx, f, L)
            a, b = t.process(rx[s:s + 1]), t.process(rxd[s:s + 1])
            ctx.synchronize()
            tw[s, f] = (a[0], host(b)[0])
    # stream 0 against the oracle's interpolators (both calls: the histories carry over)
    oi = oracle.interpolators()
    exp = [oi.interpolate(L, ys[0]), oi.interpolate(L, ys[0])] if L else [ys[0], ys[0]]
    for call in range(2):
        assert np.array_equal(tw[0, "s16"][call], exp[call])
        assert np.array_equal(tw[0, "s8"][call], iq8.narrow(exp[call]))
    for fmts in FORMAT_SETS:
        fmts = fmts[:S]
        p = sd.TxPipe(ctx, S, L)
        p.set_stream_formats(fmts)
        assert [p.stream_format(s) for s in range(S)] == fmts
        g0 = p.process(rx)
        g1 = p.process(rxd)
        ctx.synchronize()
        assert isinstance(g0, list) and isinstance(g1, list)
        same(g0, [tw[s, fmts[s]][0] for s in range(S)], (fmts, "host"))
        same(g1, [tw[s, fmts[s]][1] for s in range(S)], (fmts, "device"))
        assert all(g.shape == ((F * NF) << L, 2) and g.dtype == DT[f] for g, f in zip(g0, fmts))


# --------------------------------------------------------------------------- 2. row bounds
def raw_process(ctx, p, rxd, out, base_off, stride):
    n = C.c_size_t(0)
    return ctx.lib.sdrhip_tx_process(p.h, C.c_void_p(rxd.data_ptr()), None, rxd.shape[1], rxd.shape[1] * 128 * 512,
                                     C.c_void_p(out.data_ptr() + base_off), stride, C.byref(n), sd.MEM_DEVICE)


@pytest.mark.parametrize("L", [0, 3])
def test_row_bounds(ctx, oracle, L):
    """device output pre-filled with a sentinel, at the smallest legal stride and at a padded one: an S8 row keeps it from byte 2 * n
    to the row's end, an S16 row in its padding; a misaligned base or a stride that is no multiple of 4: SDRHIP_EALIGN, nothing written"""
    S, fmts = 3, ["s16", "s8", "s8"]
    rx, _ = batch(oracle, 3, 1, 41)
    rxd = torch.from_numpy(np.ascontiguousarray(rx)).cuda()
    n = NF << L
    tw = [twin(ctx, f, L).process(rx[s:s + 1])[0] for s, f in enumerate(fmts)]
    for stride in ((n + 3) & ~3, ((n + 3) & ~3) + 12):
        p = sd.TxPipe(ctx, S, L)
        p.set_stream_formats(fmts)
        out = torch.full((S * stride * 4 + 64,), SENT, dtype=torch.uint8, device="cuda")
        # refused: nothing written, the interpolator did not move
        assert raw_process(ctx, p, rxd, out, 4, stride) == EALIGN
        assert raw_process(ctx, p, rxd, out, 0, stride + 2) == EALIGN
        ctx.synchronize()
        assert bool((out == SENT).all())
        assert raw_process(ctx, p, rxd, out, 0, stride) == 0
        ctx.synchronize()
        o = out.cpu().numpy()
        assert (o[S * stride * 4:] == SENT).all()
        for s, f in enumerate(fmts):
            row = o[4 * s * stride:4 * (s + 1) * stride]
            nb = n * (4 if f == "s16" else 2)
            assert np.array_equal(row[:nb].view(DT[f]).reshape(n, 2), tw[s]), (stride, s)
            assert (row[nb:] == SENT).all(), (stride, s)


# --------------------------------------------------------------------------- 3. pipelined mode
def test_pipelined(ctx, oracle):
    S, fmts = 3, ["s8", "s16", "s8"]
    rx1, _ = batch(oracle, 3, 1, 41)
    rx2, _ = batch(oracle, 3, 2, 42)
    p = sd.TxPipe(ctx, S, 4, pipelined=True)
    p.set_stream_formats(fmts)
    tw = [twin(ctx, f, 4, pipelined=True) for f in fmts]
    got, exp = [], [[] for _ in range(S)]
    for i, x in enumerate([rx1, rx2, rx1]):
        if i == 2:
            for q in [p] + tw:
                assert q.configure({"interp": 3})
        got.append(p.process(x))
        for s in range(S):
            exp[s].append(tw[s].process(x[s:s + 1])[0])
        if i == 0:  # a batch waits: refused, nothing changed
            with pytest.raises(sd.SdrHipError) as e:
                p.set_stream_formats(["s16"] * S)
            assert e.value.code == EINVAL and [p.stream_format(s) for s in range(S)] == fmts
            with pytest.raises(sd.SdrHipError):
                p.set_stream_formats(None)
    got.append(p.flush())
    for s in range(S):
        exp[s].append(tw[s].flush()[0])
    assert got[0][0].shape == (0, 2) and got[1][0].shape == (NF << 4, 2) and got[3][0].shape == (NF << 3, 2)
    for i in range(4):
        same(got[i], [exp[s][i] for s in range(S)], i)
    p.set_stream_formats(["s16", "s16", "s8"])  # accepted behind the flush
    assert p.stream_format(0) == "s16"


# --------------------------------------------------------------------------- 4. submit / collect
def test_submit_collect(ctx, oracle):
    S, L = 3, 2
    rx1, _ = batch(oracle, 3, 1, 41)
    rx2, _ = batch(oracle, 3, 2, 42)
    p = sd.TxPipe(ctx, S, L)
    p.set_async(depth=2)
    tws = {f: [twin(ctx, f, L) for _ in range(S)] for f in ("s16", "s8")}  # (every twin sees every batch: the histories stay in step)
    for t in tws["s16"] + tws["s8"]:
        t.set_async(depth=2)
    for ring, fmts in enumerate((["s16", "s8", "s16"], ["s8", "s8", "s16"])):
        p.set_stream_formats(fmts)  # (between two drained rings)
        for x in (rx2, rx1):
            p.submit(x)
            for f in tws:
                for s in range(S):
                    tws[f][s].submit(x[s:s + 1])
        with pytest.raises(sd.SdrHipError) as e:  # in flight: refused
            p.set_stream_formats(["s16"] * S)
        assert e.value.code == EINVAL and [p.stream_format(s) for s in range(S)] == fmts
        for nfr in (2, 1):
            g, g0 = p.collect(block0=True)
            assert isinstance(g, list) and g0.shape == (S, nfr, 508)
            for s in range(S):
                rs = {f: tws[f][s].collect(block0=True) for f in tws}
                e, e0 = rs[fmts[s]]
                same([g[s]], [e[0]], (ring, nfr, s))
                assert g[s].shape == ((nfr * NF) << L, 2) and np.array_equal(g0[s], e0[0])
        assert p.collect(wait=False) is None


# --------------------------------------------------------------------------- 5. / 6. the datagram entries
def ragged(oracle, seed):
    rs = np.random.RandomState(seed)
    # (ragged counts of 3, 1, 0 and 2 frames sent: one stream without a datagram; what a call releases is read off the twins)
    return [np.asarray(tdg.stream_dgrams(oracle, rs, k, 16), np.uint8).reshape(-1, 512) for k in (3, 1, 0, 2)]


DG_FMTS = ["s8", "s16", "s16", "s8"]


def same_dg(got, exp, where):
    """per stream (iq, block0, records) against the one-stream twins' results"""
    for s, (g, e) in enumerate(zip(got, exp)):
        same([g[0]], [e[0][0]], (where, s))
        assert np.array_equal(host(g[1]), host(e[0][1])) and g[2] == e[0][2], (where, s)


@pytest.mark.parametrize("L,path", [(0, "wave"), (1, "wave"), (4, "wave"), (6, "wave"), (3, "valu")])
def test_process_datagrams_ragged(ctx, oracle, L, path):
    ctx.set_option("interp_path", path)
    S, per = 4, ragged(oracle, 100 + L)
    for device in (False, True):
        dg = [torch.from_numpy(d).cuda() for d in per] if device else per
        p = sd.TxPipe(ctx, S, L)
        p.set_stream_formats(DG_FMTS)
        got = p.process_datagrams(dg)
        exp = [twin(ctx, f, L).process_datagrams([dg[s]]) for s, f in enumerate(DG_FMTS)]
        ctx.synchronize()
        K = [len(e[0][2]) for e in exp]
        assert p.last_n_frames == K and K[2] == 0 and len(set(K)) == 4, K
        same_dg(got, exp, device)
        assert [g[0].shape[0] for g in got] == [(k * NF) << L for k in K]
    # device output with sentinels (the C entry): rows untouched past each stream's own count, x1 (K6x) included
    buf, counts, _ = sd.engine._datagram_batch([torch.from_numpy(d).cuda() for d in per])
    F = max(K)
    stride = (((F * NF) << L) + 3) & ~3
    out = torch.full((S * stride * 4 + 64,), SENT, dtype=torch.uint8, device="cuda")
    b0 = torch.zeros((S, F, 508), dtype=torch.uint8, device="cuda")
    info = (sd.engine.FECBufferFrame * (S * F))()
    nd, nf = (C.c_size_t * S)(*counts), (C.c_size_t * S)()
    p = sd.TxPipe(ctx, S, L)
    p.set_stream_formats(DG_FMTS)
    assert ctx.lib.sdrhip_tx_process_datagrams(p.h, C.c_void_p(buf.data_ptr()), nd, buf.shape[1] * 512, C.c_void_p(out.data_ptr() + 16), stride, F,
                                               C.c_void_p(b0.data_ptr()), info, nf, sd.MEM_DEVICE) == 0  # (any 16-byte aligned base)
    ctx.synchronize()
    o = out.cpu().numpy()
    assert (o[:16] == SENT).all() and list(nf) == K
    o = o[16:]
    for s, f in enumerate(DG_FMTS):
        row = o[4 * s * stride:4 * (s + 1) * stride]
        nb = ((int(nf[s]) * NF) << L) * (4 if f == "s16" else 2)
        assert np.array_equal(row[:nb].view(DT[f]).reshape(-1, 2), host(exp[s][0][0])), s
        assert (row[nb:] == SENT).all(), s
    assert (o[4 * S * stride:] == SENT).all()


@pytest.mark.parametrize("L,tagged", [(0, False), (4, False), (3, True), (0, True)])
def test_submit_datagrams(ctx, oracle, L, tagged):
    """the ragged batch, three batches in flight: samples, records and meta blocks are the twins'"""
    S = 4
    calls = [ragged(oracle, 200 + 10 * L + i) for i in range(3)]
    p = sd.TxPipe(ctx, S, L)
    p.set_stream_formats(DG_FMTS)
    tw = [twin(ctx, f, L) for f in DG_FMTS]
    for i, per in enumerate(calls):
        if tagged:
            arr, tags = tgt.merge(per, i, skip=5)
            p.submit_datagrams_tagged(arr, tags)
        else:
            p.submit_datagrams(per)
    with pytest.raises(sd.SdrHipError):  # in flight: refused
        p.set_stream_formats(None)
    for i, per in enumerate(calls):
        got = p.collect_datagrams()
        exp = [tw[s].process_datagrams([per[s]]) for s in range(S)]
        assert sum(len(g[2]) for g in got) > 0 and len(got[2][2]) == 0
        same_dg(got, exp, i)
    assert p.collect_datagrams(wait=False) is None
    p.set_stream_formats(None)


# --------------------------------------------------------------------------- 7. the four-wave workgroup shape
def test_four_wave_workgroups(ctx, oracle):
    """64 streams x 8 frames at x4 with the default span: nseg * nstreams = 64 * 64 = 4096, the workgroups of four waves"""
    S, F, L = 64, 8, 2
    rx3, _ = batch(oracle, 3, F, 48)
    rx = np.ascontiguousarray(rx3[np.arange(S) % 3])
    fmts = ["s8" if s % 2 else "s16" for s in range(S)]
    p = sd.TxPipe(ctx, S, L)
    p.set_stream_formats(fmts)
    got = p.process(torch.from_numpy(rx).cuda())
    ctx.synchronize()
    assert len(got) == S
    for s in (0, 1, 63):
        same([got[s]], [twin(ctx, fmts[s], L).process(rx[s:s + 1])[0]], s)


# --------------------------------------------------------------------------- 8. byte counters
def test_byte_counters(ctx, oracle):
    """against an all-S16 array on the same input the download shrinks by 2 bytes per sample of the S8 streams; the upload is equal"""
    S, L = 3, 3
    rx1, _ = batch(oracle, 3, 1, 41)
    per = ragged(oracle, 300)[:3]
    fm = ["s8", "s16", "s8"]
    K = [len(r[2]) for r in sd.TxPipe(ctx, S, L).process_datagrams(per)]  # frames a call releases per stream
    assert K[0] > 0 and K[2] == 0

    def deltas(fmts, run):
        p = sd.TxPipe(ctx, S, L)
        p.set_stream_formats(fmts)
        h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        run(p)
        return ctx.counter("h2d_bytes") - h0, ctx.counter("d2h_bytes") - d0

    def submit(p):
        p.submit(rx1)
        p.collect()

    def submit_dg(p):
        p.submit_datagrams(per)
        assert [len(r[2]) for r in p.collect_datagrams()] == K

    n = NF << L
    for run, s8_samples in ((lambda p: p.process(rx1), 2 * n), (submit, 2 * n), (submit_dg, (K[0] + K[2]) * n),
                            (lambda p: p.process_datagrams(per), (K[0] + K[2]) * n)):
        (h_m, d_m), (h_a, d_a) = deltas(fm, run), deltas(["s16"] * S, run)
        assert h_m == h_a > 0, (h_m, h_a)
        assert d_a - d_m == 2 * s8_samples, (d_a, d_m, s8_samples)


# --------------------------------------------------------------------------- 9. nothing else moves
def _counts(ctx):
    return [ctx.kernel_timing_read(k)[1] for k in range(5)]


def test_nothing_else_moves(ctx, oracle):
    """set_stream_formats(None) gives the bank-wide handle's output again, in its stride unit; a handle that never saw the setter and
    one that set and cleared it show the same launch counts per class (no convert-class launch), as a bank-wide handle did before"""
    S, L = 3, 4
    rx1, _ = batch(oracle, 3, 1, 41)
    per = ragged(oracle, 300)[:3]
    res = []
    for touched in (False, True):
        p = sd.TxPipe(ctx, S, L, output_format="s8")
        if touched:
            p.set_stream_formats(["s16", "s8", "s16"])
            p.set_stream_formats(None)
            assert p.stream_format(0) == "s8"
        ctx.kernel_timing(True)
        _counts(ctx)
        a = p.process(rx1)
        b = p.process_datagrams(per)
        ctx.synchronize()
        res.append((a, b, _counts(ctx)))
        ctx.kernel_timing(False)
    (a0, b0, c0), (a1, b1, c1) = res
    assert isinstance(a1, np.ndarray) and a1.dtype == np.int8 and a1.shape == (S, NF << L, 2) and np.array_equal(a0, a1)
    for (g, gb, gr), (e, eb, er) in zip(b1, b0):
        assert g.dtype == np.int8 and np.array_equal(g, e) and np.array_equal(gb, eb) and gr == er
    assert c0 == c1 and c0[1] > 0 and c0[4] == 0, (c0, c1)
    # an array of equal entries: the bytes of that bank-wide format
    q = sd.TxPipe(ctx, S, L)
    q.set_stream_formats(["s8"] * S)
    same(q.process(rx1), list(a0), "equal entries")
    # refused values change nothing
    fm = [q.stream_format(s) for s in range(S)]
    assert ctx.lib.sdrhip_tx_set_stream_format(q.h, (C.c_int * S)(0, 1, 2)) == EINVAL  # U8 is no Tx format
    assert ctx.lib.sdrhip_tx_set_stream_format(q.h, (C.c_int * S)(0, 2, 7)) == EINVAL
    f = C.c_int(9)
    assert ctx.lib.sdrhip_tx_get_stream_format(q.h, S, C.byref(f)) == EINVAL and f.value == 9
    assert [q.stream_format(s) for s in range(S)] == fm
    with pytest.raises(ValueError):
        q.set_stream_formats(["s8", "u8", "s8"])
    with pytest.raises(ValueError):
        q.set_stream_formats(["s8"])


# --------------------------------------------------------------------------- 10. lifecycle
def test_lifecycle(ctx, oracle):
    S, L = 3, 3
    fmts = ["s16", "s8", "s16"]
    rx1, _ = batch(oracle, 3, 1, 41)
    rx2, _ = batch(oracle, 3, 2, 42)
    # reset_streams on one stream of a mixed bank: the array stays in force, the stream begins again
    p = sd.TxPipe(ctx, S, L)
    p.set_stream_formats(fmts)
    tw = [twin(ctx, f, L) for f in fmts]
    p.process(rx2)
    for s in range(S):
        tw[s].process(rx2[s:s + 1])
    p.reset_streams([1])
    tw[1] = twin(ctx, "s8", L)
    assert [p.stream_format(s) for s in range(S)] == fmts
    same(p.process(rx1), [tw[s].process(rx1[s:s + 1])[0] for s in range(S)], "reset")
    # a stream exported from an all-S16 bank continues in slot 1 of the mixed bank byte for byte as S8
    src = sd.TxPipe(ctx, 2, L)
    src.process(rx2[:2])
    blob = src.export_stream(0)
    cont = twin(ctx, "s8", L)  # the same history, delivered as S8 from here on
    cont.process(rx2[:1])
    p.import_stream(1, blob)
    tw[1] = cont
    x = np.ascontiguousarray(rx1[[0, 2, 1]])
    same(p.process(x), [tw[s].process(x[s:s + 1])[0] for s in range(S)], "import")
    assert [p.stream_format(s) for s in range(S)] == fmts
