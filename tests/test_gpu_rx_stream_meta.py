"""Per-stream centre frequency and sample rate of an Rx bank (sdrhip_rx_set_stream_meta / sdrhip_rx_get_stream_meta).

Stream s of a bank must produce, byte for byte, what a one-stream pipe produces whose config carries stream s's two values: the
meta block (bytes 0..7, the CRC over its own 20 bytes, a time stamp advanced by the stream's OWN sample clock) and the recovery
blocks computed over it.  Checked against the compiled reference decimators + the oracle framer / encoder, and against one-stream
twins on every device site that forms a meta record (K2 / K2r, K2 inside the encoder's launch, the VALU cascade's frame epilogue
also under the matrix-core launch, the three encoders that derive block 0 themselves), through every entry: immediate, pipelined +
flush, ragged, the asynchronous uniform / ragged / datagram batches, the datagram-fed hub, and a TestSource bank followed per
stream.

Shapes: F = 16129 decimated samples per frame, 4 streams, calls of (2 F + 100) << L samples: every stream opens at least two
frames per call and one frame stays open across calls.  Rates: 0 (no advance), 8000 (a frame lasts 2.016 s: the stamp crosses
seconds and the microsecond carry), 625000, 10^7 >> L.  One frequency lies above 2^31 (a signed slip would show)."""
import numpy as np
import pytest
import torch

import sdrdaemon_amd as sd

pytestmark = pytest.mark.gpu

F = 16129
S = 4
FREQS = [435000, 3000000000, 1, 1296500]
FREQS_B = [144800, 7, 4294967295, 10489750]


def rates(L):
    return [0, 8000, 625000, 10000000 >> L]


def rates_b(L):
    return [48000, 0, 250000 >> L, 2048000]


def call_len(L):
    return ((2 * F + 100) << L) + 3 & ~3  # (device rows: a multiple of 4 samples)


@pytest.fixture
def ctx():
    assert sd.device_count() > 0
    return sd.Context(0)


def rand_iq(rs, nstreams, n):
    return rs.randint(-32768, 32768, size=(nstreams, n, 2)).astype(np.int16)


def make_twins(ctx, fcs, srs, nstreams=S, **cfg):
    """one one-stream pipe per stream, configured bank-wide with that stream's values: the expected result of a bank"""
    return [sd.RxPipe(ctx, 1, center_frequency_khz=fcs[s], sample_rate=srs[s], **cfg) for s in range(nstreams)]


def meta_of(frame):
    """(centre frequency, sample rate, tv_sec, tv_usec) of a frame's meta block (block 0 behind its 4-byte header)"""
    w = np.frombuffer(np.ascontiguousarray(frame[0, 4:28]).tobytes(), dtype="<u4")
    return int(w[0]), int(w[1]), int(w[3]), int(w[4])


def as_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ------------------------------------------------------------------------------------------------ 1. the reference chain
@pytest.mark.skipif(not __import__("oracle_lib").Reference.available("eo1"), reason="compiled reference not built")
@pytest.mark.parametrize("entry", ["uniform", "ragged"])
@pytest.mark.parametrize("L,fcpos,R", [(4, sd.FC_CEN, 32), (3, sd.FC_INF, 8), (0, sd.FC_CEN, 0)])
def test_against_reference_chain(ctx, oracle, L, fcpos, R, entry):
    """per stream: the compiled reference decimators, the oracle framer with that stream's frequency, rate and stamps, frame_encode"""
    from oracle_lib import Reference

    rs = np.random.RandomState(10 * L + R)
    bank = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, sample_bits=16, nb_fec=R)
    bank.set_stream_meta(FREQS, rates(L))
    refs = [Reference("eo1").decimators() for _ in range(S)]
    framers = [None] * S
    got, exp = [[] for _ in range(S)], [[] for _ in range(S)]
    for k in range(3):
        n = call_len(L)
        counts = [n] * S if entry == "uniform" else [n - s * (3 << L) - s for s in range(S)]
        x = rand_iq(rs, S, n)
        if entry == "uniform":
            secs, usecs = [1000 + 10 * k] * S, [999990 - k] * S
            g = bank.process(x, secs[0], usecs[0])
            nf = [g.shape[1]] * S
        else:
            secs, usecs = [1000 + 10 * k + s for s in range(S)], [999990 - 37 * k - s for s in range(S)]
            g, nf = bank.process_ragged(x, counts, secs, usecs)
        for s in range(S):
            assert nf[s] >= 2, (k, s, nf[s])
            got[s].extend(list(g[s, :nf[s]]))
            y, ss = refs[s].decimate(L, fcpos, 16, np.ascontiguousarray(x[s, :counts[s]]))
            if framers[s] is None:
                framers[s] = oracle.framer(center_frequency_khz=FREQS[s], sample_rate=rates(L)[s], nb_fec_blocks=R,
                                           sample_bytes=(ss - 1) // 8 + 1, sample_bits=ss)
            framers[s].s.tv_sec, framers[s].s.tv_usec = secs[s], usecs[s]
            exp[s].extend(list(framers[s].write(y)))
    for s in range(S):
        assert len(got[s]) == len(exp[s]) >= 6, s
        for f in range(len(exp[s])):
            assert meta_of(got[s][f])[:2] == (FREQS[s], rates(L)[s]), (s, f)
            assert np.array_equal(got[s][f][:128], exp[s][f]), (s, f, meta_of(got[s][f]), meta_of(exp[s][f]))
            if R:
                assert np.array_equal(got[s][f][128:], oracle.frame_encode(exp[s][f], R)), (s, f)


# ------------------------------------------------------------------------------------------------ 2. one-stream twins, site by site
def smallest_mfma_call(ctx, L, **cfg):
    """the smallest call of m frames + 100 samples for which the bank's launch is the matrix-core one with wave groups"""
    for m in (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128):
        n = (m * F + 100) << L
        probe = sd.RxPipe(ctx, S, log2decim=L, **cfg)
        probe.process_view(torch.zeros((S, n, 2), dtype=torch.int16, device="cuda"))
        ctx.synchronize()
        plan = probe.last_plan()
        probe.close()
        if plan["path"] == "mfma" and plan["wps"] > 0:
            return n
    pytest.fail("no call up to 128 frames per stream takes the matrix-core path")


def run_twins(ctx, cfg, n, ncalls, pipelined=False, seed=0, want_path=None):
    L = cfg["log2decim"]
    rs = np.random.RandomState(seed)
    bank = sd.RxPipe(ctx, S, pipelined=pipelined, **cfg)
    bank.set_stream_meta(FREQS, rates(L))
    twins = make_twins(ctx, FREQS, rates(L), pipelined=pipelined, **cfg)
    total = 0
    for k in range(ncalls):
        x = torch.from_numpy(rand_iq(rs, S, n)).cuda()
        sec, usec = 77 + 3 * k, 999999 - k
        g = bank.process(x, sec, usec)
        if want_path:
            plan = bank.last_plan()
            assert plan["path"] == want_path and (want_path != "mfma" or plan["wps"] > 0), plan
        ctx.synchronize()
        g = as_np(g)
        for s in range(S):
            e = as_np(twins[s].process(x[s], sec, usec))
            assert g.shape[1] == e.shape[0], (k, s, g.shape, e.shape)
            assert np.array_equal(g[s], e), (k, s)
            for f in range(e.shape[0]):
                assert meta_of(g[s, f])[:2] == (FREQS[s], rates(L)[s]), (k, s, f)
        total += g.shape[1]
    if pipelined:
        g = bank.flush()
        for s in range(S):
            e = twins[s].flush()
            assert g.shape[1] == e.shape[1] >= 2 and np.array_equal(g[s], e[0]), ("flush", s)
        total += g.shape[1]
    assert total >= 2 * ncalls
    return bank


def test_site_valu_frame_epilogue(ctx):
    """decim_path = valu: the cascade kernel stores straight into the frame layout, its epilogue writes the meta blocks"""
    ctx.set_option("decim_path", "valu")
    for R in (0, 8, 40):
        run_twins(ctx, dict(log2decim=4, fcpos=sd.FC_CEN, nb_fec=R), call_len(4), 2, seed=R, want_path="valu")


def test_site_mfma_pieces_epilogue(ctx):
    """decim_path = mfma, rx_direct = 1: the matrix-core waves store into the frame layout, the VALU pieces write the meta blocks"""
    ctx.set_option("decim_path", "mfma")
    ctx.set_option("rx_direct", 1)
    L = 3
    n = smallest_mfma_call(ctx, L, nb_fec=8)
    for R in (0, 8, 40):
        run_twins(ctx, dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R), n, 2, seed=20 + R, want_path="mfma")


@pytest.mark.parametrize("enc_path,enc_form,R", [("fft", "bitslice", 0), ("fft", "bitslice", 8), ("fft", "table", 8),
                                                 ("karatsuba", "table", 40), ("fft", "bitslice", 40), ("karatsuba", "table", 8)])
def test_site_k2_and_the_encoders(ctx, enc_path, enc_form, R):
    """decim_path = mfma, rx_direct = 0: stream order, then K2 -- a launch of its own (nb_fec = 0, and 8 without the FFT: the generic
    matrix kernel), or riding in the structured encoder's launch, where the encoder derives block 0 itself: the bit-sliced FFT form,
    the table FFT form, the Karatsuba walk (40 rows: always; any count with enc_path = karatsuba from 13 rows on)"""
    ctx.set_option("decim_path", "mfma")
    ctx.set_option("rx_direct", 0)
    ctx.set_option("enc_path", enc_path)
    ctx.set_option("enc_form", enc_form)
    L = 3
    n = smallest_mfma_call(ctx, L, nb_fec=R)
    run_twins(ctx, dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R), n, 2, seed=40 + R, want_path="mfma")
    assert (ctx.option("rx_direct"), ctx.option("enc_path"), ctx.option("enc_form")) == ("0", enc_path, enc_form)


@pytest.mark.parametrize("rx_fused", [0, 1, 2])
def test_pipelined_and_flush(ctx, rx_fused):
    """pipelined: a call delivers the previous call's frames, encoded inside this call's launch (1), next to it (2) or behind it (0);
    flush delivers the last call's"""
    ctx.set_option("decim_path", "mfma")
    ctx.set_option("rx_fused", rx_fused)
    L = 3
    n = smallest_mfma_call(ctx, L, nb_fec=32)
    run_twins(ctx, dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=32), n, 3, pipelined=True, seed=60 + rx_fused, want_path="mfma")
    assert ctx.option("rx_fused") == str(rx_fused)


def test_pipelined_valu_and_filterless(ctx):
    """pipelined on the VALU cascade, and the filter-less decimate1 (stream order + K2) immediate"""
    run_twins(ctx, dict(log2decim=4, fcpos=sd.FC_CEN, nb_fec=8), call_len(4), 3, pipelined=True, seed=70)
    run_twins(ctx, dict(log2decim=0, fcpos=sd.FC_CEN, nb_fec=8), call_len(0), 2, seed=71)
    run_twins(ctx, dict(log2decim=2, fcpos=sd.FC_SUP, nb_fec=40), call_len(2), 2, seed=72)


@pytest.mark.parametrize("rx_direct", [1, 0])
def test_ragged_on_the_matrix_cores(ctx, rx_direct):
    """ragged calls with decim_path = mfma: K1mr stores straight into the windows and writes the shared record, K2r rewrites the
    meta blocks behind it with each stream's values (rx_direct = 1); stream order + K2r (0)"""
    ctx.set_option("decim_path", "mfma")
    ctx.set_option("rx_direct", rx_direct)
    L = 3
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    rs = np.random.RandomState(80 + rx_direct)
    bank = sd.RxPipe(ctx, S, **cfg)
    bank.set_stream_meta(FREQS, rates(L))
    twins = make_twins(ctx, FREQS, rates(L), **cfg)
    n = smallest_mfma_call(ctx, L, nb_fec=8)
    for k in range(2):
        counts = [n - s * (5 << L) - s for s in range(S - 1)] + [(F << L) // 3]  # (the last stream opens one frame and completes none)
        x = rand_iq(rs, S, n)
        secs, usecs = [30 + 5 * k + s for s in range(S)], [999999 - s for s in range(S)]
        g, nf = bank.process_ragged(x, counts, secs, usecs)
        plan = bank.last_plan()
        assert plan["path"] == "mfma" and plan["wps"] > 0, plan
        for s in range(S):
            e = twins[s].process(np.ascontiguousarray(x[s, :counts[s]]), secs[s], usecs[s])
            assert nf[s] == e.shape[0] and np.array_equal(g[s, :nf[s]], e), (k, s)
            assert all(meta_of(f)[:2] == (FREQS[s], rates(L)[s]) for f in e), (k, s)
        assert min(nf[:S - 1]) >= 2


# ------------------------------------------------------------------------------------------------ 3. change between calls
def test_change_between_calls(ctx):
    L = 3
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    rs = np.random.RandomState(3)
    bank = sd.RxPipe(ctx, S, center_frequency_khz=111, sample_rate=48000, **cfg)
    twins = make_twins(ctx, FREQS, rates(L), **cfg)
    for s in range(S):
        assert bank.stream_meta(s) == {"center_frequency_khz": 111, "sample_rate": 48000}
    bank.set_stream_meta(FREQS, rates(L))

    def call(k):
        x = rand_iq(rs, S, call_len(L))
        g = bank.process(x, 500 + k, 999000)
        assert g.shape[1] >= 2
        for s in range(S):
            assert np.array_equal(g[s], twins[s].process(x[s], 500 + k, 999000)), (k, s)
        return g

    g = call(0)
    assert all(meta_of(g[s, f])[:2] == (FREQS[s], rates(L)[s]) for s in range(S) for f in range(g.shape[1]))
    # both arrays change while a frame is open: it keeps its meta block, frames opened later carry the new values
    bank.set_stream_meta(FREQS_B, rates_b(L))
    for s in range(S):
        assert bank.stream_meta(s) == {"center_frequency_khz": FREQS_B[s], "sample_rate": rates_b(L)[s]}
        twins[s].reconfigure(center_frequency_khz=FREQS_B[s], sample_rate=rates_b(L)[s])
    g = call(1)
    for s in range(S):
        assert meta_of(g[s, 0])[:2] == (FREQS[s], rates(L)[s]), s
        assert all(meta_of(g[s, f])[:2] == (FREQS_B[s], rates_b(L)[s]) for f in range(1, g.shape[1])), s
    # back to the config's values
    bank.set_stream_meta(None, None)
    for s in range(S):
        assert bank.stream_meta(s) == {"center_frequency_khz": 111, "sample_rate": 48000}
        twins[s].reconfigure(center_frequency_khz=111, sample_rate=48000)
    g = call(2)
    for s in range(S):
        assert meta_of(g[s, 0])[:2] == (FREQS_B[s], rates_b(L)[s]), s
        assert all(meta_of(g[s, f])[:2] == (111, 48000) for f in range(1, g.shape[1])), s
    # one array alone; reconfigure() of the field it covers has no effect until it is cleared
    bank.set_stream_meta(center_frequency_khz=FREQS)
    bank.reconfigure(center_frequency_khz=222)
    for s in range(S):
        assert bank.stream_meta(s) == {"center_frequency_khz": FREQS[s], "sample_rate": 48000}
        twins[s].reconfigure(center_frequency_khz=FREQS[s])
    g = call(3)
    assert all(meta_of(g[s, f])[:2] == (FREQS[s], 48000) for s in range(S) for f in range(1, g.shape[1]))
    bank.set_stream_meta(None, None)
    for s in range(S):
        twins[s].reconfigure(center_frequency_khz=222)
    g = call(4)
    assert all(meta_of(g[s, f])[:2] == (222, 48000) for s in range(S) for f in range(1, g.shape[1]))
    # refusals
    lib = sd._lib.lib()
    assert lib.sdrhip_rx_set_stream_meta(None, None, None) == -1
    assert lib.sdrhip_rx_get_stream_meta(None, 0, None, None) == -1
    assert lib.sdrhip_rx_get_stream_meta(bank.h, S, None, None) == -1
    assert lib.sdrhip_rx_get_stream_meta(bank.h, -1, None, None) == -1
    with pytest.raises(ValueError):
        bank.set_stream_meta([1, 2, 3])


# ------------------------------------------------------------------------------------------------ 4. asynchronous entries
VERSIONS = [(FREQS, rates), (FREQS_B, rates_b), (FREQS[::-1], lambda L: rates(L)[::-1])]


def counters(ctx):
    return ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")


def test_async_uniform_batches(ctx):
    """blocks = 3, depth = 3: the setter is called between submits with batches in flight; a batch carries the values in force when
    it was launched (its third block)"""
    L = 3
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    rs = np.random.RandomState(4)
    blk = call_len(L) // 3 + 8
    data = [[rand_iq(rs, S, blk) for _ in range(3)] for _ in range(3)]
    traffic = []
    for use in (True, False):
        bank = sd.RxPipe(ctx, S, **cfg)
        bank.set_async(depth=3, blocks=3)
        c0 = counters(ctx)
        for v in range(3):
            for j in range(3):
                if use and j == 1:  # (while the batch is being filled and earlier ones are in flight)
                    bank.set_stream_meta(VERSIONS[v][0], VERSIONS[v][1](L))
                bank.submit(data[v][j], 900 + v, 999999 if j == 0 else 5)
        out = [bank.collect(wait=True) for _ in range(3)]
        c1 = counters(ctx)
        traffic.append((c1[0] - c0[0], c1[1] - c0[1]))
        if not use:
            continue
        twins = make_twins(ctx, FREQS, rates(L), **cfg)
        for v in range(3):
            assert out[v].shape[1] >= 2
            for s in range(S):
                if v:
                    twins[s].reconfigure(center_frequency_khz=VERSIONS[v][0][s], sample_rate=VERSIONS[v][1](L)[s])
                e = twins[s].process(np.concatenate([b[s] for b in data[v]]), 900 + v, 999999)
                assert np.array_equal(out[v][s], e), (v, s)
                assert meta_of(out[v][s, -1])[:2] == (VERSIONS[v][0][s], VERSIONS[v][1](L)[s]), (v, s)
    assert traffic[0] == traffic[1], traffic  # (the table is not sample traffic)
    assert ctx.counter("fecbuf_shadow_mismatch") == 0


@pytest.mark.parametrize("packed", [True, False])
def test_async_ragged_batches(ctx, packed):
    L = 3
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    rs = np.random.RandomState(5)
    n = call_len(L)
    counts = [[n - s * (5 << L) - 3 * v for s in range(S)] for v in range(3)]
    data = [rand_iq(rs, S, n) for _ in range(3)]
    secs, usecs = [[40 + 7 * v + s for s in range(S)] for v in range(3)], [[999999 - s for s in range(S)] for _ in range(3)]
    traffic = []
    for use in (True, False):
        bank = sd.RxPipe(ctx, S, **cfg)
        bank.set_async(depth=3, blocks=1)
        c0 = counters(ctx)
        for v in range(3):
            if use:
                bank.set_stream_meta(VERSIONS[v][0], VERSIONS[v][1](L))
            x = np.concatenate([data[v][s, :counts[v][s]] for s in range(S)]) if packed else data[v]
            bank.submit_ragged(x, counts[v], secs[v], usecs[v])
        if use:
            bank.set_stream_meta(None, None)  # (every batch is in flight: they keep their values)
        out = [bank.collect_ragged(wait=True) for _ in range(3)]
        c1 = counters(ctx)
        traffic.append((c1[0] - c0[0], c1[1] - c0[1]))
        if not use:
            continue
        twins = make_twins(ctx, FREQS, rates(L), **cfg)
        for v in range(3):
            for s in range(S):
                if v:
                    twins[s].reconfigure(center_frequency_khz=VERSIONS[v][0][s], sample_rate=VERSIONS[v][1](L)[s])
                e = twins[s].process(np.ascontiguousarray(data[v][s, :counts[v][s]]), secs[v][s], usecs[v][s])
                assert out[v][s].shape[0] == e.shape[0] >= 2 and np.array_equal(out[v][s], e), (v, s)
    assert traffic[0] == traffic[1], traffic
    assert ctx.counter("fecbuf_shadow_mismatch") == 0


def hub_datagrams(oracle, seed, ncalls):
    """per call, per stream an (n, 512) array of raw datagrams made with the oracle encoder (losses, incoming fecblk 8 and 32)"""
    import test_gpu_tx_datagrams as tt

    rs = np.random.RandomState(seed)
    per = [tt.split(rs, tt.stream_dgrams(oracle, rs, 3 * ncalls + s % 2, (8, 32)[s % 2]), ncalls) for s in range(S)]
    return [[per[s][i] for s in range(S)] for i in range(ncalls)]


def test_async_datagram_batches(ctx, oracle):
    """depth = 3: three datagram batches in flight, the setter between the submits; a batch takes the values at its submit"""
    torch.zeros(1).cuda()
    L = 0
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    calls = hub_datagrams(oracle, 6, 3)
    traffic = []
    for use in (True, False):
        bank = sd.RxPipe(ctx, S, **cfg)
        bank.set_async(depth=3, blocks=1)
        c0 = counters(ctx)
        for v in range(3):
            if use:
                bank.set_stream_meta(VERSIONS[v][0], VERSIONS[v][1](L))
            bank.submit_datagrams(calls[v], 60 + v, 999999)
        if use:
            bank.set_stream_meta(None, None)
        out = [bank.collect_datagrams(wait=True) for _ in range(3)]
        c1 = counters(ctx)
        traffic.append((c1[0] - c0[0], c1[1] - c0[1]))
        if not use:
            continue
        twins = make_twins(ctx, FREQS, rates(L), **cfg)
        total = 0
        for v in range(3):
            for s in range(S):
                if v:
                    twins[s].reconfigure(center_frequency_khz=VERSIONS[v][0][s], sample_rate=VERSIONS[v][1](L)[s])
                e = as_np(twins[s].process_datagrams([calls[v][s]], 60 + v, 999999)[0][0])
                assert np.array_equal(as_np(out[v][s][0]), e), (v, s)
                total += e.shape[0]
        assert total >= 3 * S
    assert traffic[0] == traffic[1], traffic
    assert ctx.counter("fecbuf_shadow_mismatch") == 0


# ------------------------------------------------------------------------------------------------ 5. the hub
@pytest.mark.parametrize("L,R", [(0, 8), (2, 32)])
def test_hub_process_datagrams(ctx, oracle, L, R):
    """stream s's re-framed frames equal the one-stream hub's with that stream's values; device and host datagrams"""
    torch.zeros(1).cuda()
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    calls = hub_datagrams(oracle, 7 + L, 2)
    bank = sd.RxPipe(ctx, S, **cfg)
    bank.set_stream_meta(FREQS, rates(L))
    twins = make_twins(ctx, FREQS, rates(L), **cfg)
    total = 0
    for k, chunk in enumerate(calls):
        arg = [torch.from_numpy(c).cuda() for c in chunk] if k % 2 == 0 else chunk
        got = bank.process_datagrams(arg, [70 + s for s in range(S)], 999999)
        for s in range(S):
            e = as_np(twins[s].process_datagrams([arg[s]], 70 + s, 999999)[0][0])
            g = as_np(got[s][0])
            assert g.shape == e.shape and np.array_equal(g, e), (k, s)
            assert all(meta_of(f)[:2] == (FREQS[s], rates(L)[s]) for f in g), (k, s)
            total += g.shape[0]
    assert total >= S


# ------------------------------------------------------------------------------------------------ 6. follow_testsource
def test_follow_testsource(ctx):
    """what sdrdaemonrx's loop does with its source: frequency // 1000 and srate >> decim, per stream of a TestSource bank"""
    L, n = 3, call_len(3)
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
    ts = sd.TestSource(ctx, 3)
    want = [(2000000, 435000999), (1000000, 2147000999), (64000, 1296500500)]
    for s, (srate, freq) in enumerate(want):
        assert ts.configure("srate=%d,freq=%d" % (srate, freq), stream=s), ts.error()
    bank = sd.RxPipe(ctx, 3, **cfg)
    bank.follow_testsource(ts)
    for s, (srate, freq) in enumerate(want):
        assert bank.stream_meta(s) == {"center_frequency_khz": freq // 1000, "sample_rate": srate >> L}
    twins = make_twins(ctx, [f // 1000 for _, f in want], [r >> L for r, _ in want], nstreams=3, **cfg)
    for k in range(2):
        x = ts.read(n)
        g = bank.process(x, 10 + k, 999999)
        ctx.synchronize()
        assert g.shape[1] >= 2
        for s in range(3):
            assert torch.equal(g[s], twins[s].process(x[s].contiguous(), 10 + k, 999999)), (k, s)
    with pytest.raises(ValueError):
        sd.RxPipe(ctx, 2, **cfg).follow_testsource(ts)


# ------------------------------------------------------------------------------------------------ 7. the untouched default
@pytest.mark.parametrize("cleared", [False, True])
def test_untouched_default(ctx, cleared):
    """never set, or set and cleared: the bank launches what it launched before the entry existed -- the same plan as a bank of the
    same shape, frames equal to one-stream pipes with the same config, every stream the config's two values"""
    L = 4
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=32, center_frequency_khz=435000, sample_rate=625000)
    rs = np.random.RandomState(8)
    bank, plain = sd.RxPipe(ctx, S, **cfg), sd.RxPipe(ctx, S, **cfg)
    if cleared:
        bank.set_stream_meta(FREQS, rates(L))
        bank.set_stream_meta(None, None)
    twins = [sd.RxPipe(ctx, 1, **cfg) for _ in range(S)]
    for k in range(2):
        x = rand_iq(rs, S, call_len(L))
        g, p = bank.process(x, 5 + k, 6), plain.process(x, 5 + k, 6)
        assert bank.last_plan() == plain.last_plan()
        assert g.shape[1] >= 2 and np.array_equal(g, p)
        for s in range(S):
            assert np.array_equal(g[s], twins[s].process(x[s], 5 + k, 6)), (k, s)
            assert all(meta_of(f)[:2] == (435000, 625000) for f in g[s])
    for k in range(2):  # (ragged calls leave the streams at different frame positions: behind the uniform ones)
        x = rand_iq(rs, S, call_len(L))
        counts = [call_len(L) - s * (3 << L) for s in range(S)]
        gr, nf = bank.process_ragged(x, counts, 8 + k, 9)
        pr, nfp = plain.process_ragged(x, counts, 8 + k, 9)
        assert list(nf) == list(nfp) and np.array_equal(gr, pr) and bank.last_plan() == plain.last_plan()
        for s in range(S):
            assert np.array_equal(gr[s, :nf[s]], twins[s].process(np.ascontiguousarray(x[s, :counts[s]]), 8 + k, 9)), (k, s)
