"""8-bit IQ at the edges of the pipes (sdrhip_rx_set_input_format, sdrhip_tx_set_output_format).

Rx: RTL-SDR (u8, offset binary) and HackRF (s8) bytes through an 8-bit pipe must give the frames of an int16 pipe fed the samples
widened on the host by the reference's formulas (RtlSdrSource.cpp:542-553, HackRFSource.cpp:661-674); one case goes straight
against the compiled reference decimators + the oracle framer / encoder.  Tx: the 8-bit outputs must equal the int16 outputs >> 8
(HackRFSink.cpp:671-672), and the oracle's interpolators >> 8.  Byte counters, refusals and the untouched int16 default too."""
import ctypes as C

import numpy as np
import pytest
import torch

import sdrdaemon_amd as sd
import signals
import test_gpu_tx_datagrams as tdg

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    assert sd.device_count() > 0
    return sd.Context(0)


def widen(x8, fmt):
    """the reference sources' host-side widening"""
    return (x8.astype(np.int16) - 128).astype(np.int16) if fmt == "u8" else x8.astype(np.int16)


def rand8(rs, shape, fmt):
    return rs.randint(0, 256, size=shape).astype(np.uint8) if fmt == "u8" else rs.randint(-128, 128, size=shape).astype(np.int8)


def cw8(n, fmt, S=1):
    """a TestSource-like carrier quantised to 8 bits (the RTL-SDR's resolution)"""
    t = np.arange(n)
    out = []
    for s in range(S):
        ph = 2 * np.pi * (0.0123 + 0.01 * s) * t
        i, q = np.round(100 * np.cos(ph)), np.round(100 * np.sin(ph))
        v = np.stack([i, q], -1).astype(np.int16)
        out.append((v + 128).astype(np.uint8) if fmt == "u8" else v.astype(np.int8))
    return np.stack(out)


def run_rx(ctx, x, fmt, cfg, cuts, device=False, pipelined=False, stride_pad=0):
    """feed x (S, n, 2) in the cut calls through a pipe of input format `fmt`; -> all delivered frames (S, F, 128 + R, 512)"""
    S = x.shape[0]
    rx = sd.RxPipe(ctx, S, pipelined=pipelined, input_format=fmt, **cfg)
    got = []
    for i in range(len(cuts) - 1):
        seg = x[:, cuts[i]:cuts[i + 1]]
        if stride_pad or device:  # rows of a bigger buffer: a stride that is not the row length
            n = seg.shape[1]
            w = ((n + stride_pad + 7) & ~7) if device else n + stride_pad  # (device rows: 16-byte aligned, a multiple of 8 samples)
            big = np.zeros((S, w, 2), seg.dtype)
            big[:, :n] = seg
            seg = big[:, :n]
        if device:
            t = torch.from_numpy(np.ascontiguousarray(big)).cuda()[:, :seg.shape[1]]
            f = rx.process(t, tv_sec=10 + i, tv_usec=3 * i)
            ctx.synchronize()
            f = f.cpu().numpy()
        elif stride_pad:  # (host rows with their own stride: the C entry, bypassing the Python copy)
            cap = max(rx.max_frames(seg.shape[1]), 1)
            fb = (128 + cfg["nb_fec"]) * 512
            out = np.zeros((S, cap, 128 + cfg["nb_fec"], 512), np.uint8)
            nf = C.c_size_t(0)
            sd._lib.check(ctx.lib.sdrhip_rx_process(rx.h, C.c_void_p(seg.ctypes.data), seg.shape[1], big.strides[0] // (2 * big.itemsize), 10 + i, 3 * i,
                                                    C.c_void_p(out.ctypes.data), cap * fb, C.byref(nf), sd.MEM_HOST))
            f = out[:, :nf.value]
        else:
            f = rx.process(seg, tv_sec=10 + i, tv_usec=3 * i)
        got.append(f if f.ndim == 4 else f[None])
    if pipelined:
        got.append(rx.flush())
    rx.close()
    return np.concatenate(got, axis=1)


RX_CASES = [
    # (fmt, log2decim, fcpos, sample_bits, hb, nb_fec, S, device, pipelined, rx_direct, stride_pad)
    ("u8", 4, sd.FC_CEN, 8, sd.HB_EO1, 32, 8, False, False, 1, 8),
    ("s8", 4, sd.FC_CEN, 8, sd.HB_DB, 32, 8, True, False, 1, 8),
    ("u8", 4, sd.FC_CEN, 16, sd.HB_EO1, 0, 2, True, False, 0, 0),
    ("s8", 4, sd.FC_CEN, 8, sd.HB_EO1, 32, 2, False, True, 1, 0),
    ("u8", 4, sd.FC_CEN, 8, sd.HB_DB, 32, 2, True, True, 1, 0),
    ("u8", 0, sd.FC_INF, 8, sd.HB_EO1, 32, 8, False, False, 1, 24),
    ("s8", 0, sd.FC_CEN, 16, sd.HB_DB, 0, 2, True, False, 1, 0),
    ("u8", 1, sd.FC_INF, 8, sd.HB_EO1, 32, 2, True, False, 1, 0),
    ("s8", 1, sd.FC_SUP, 16, sd.HB_DB, 32, 2, False, False, 1, 0),
    ("u8", 1, sd.FC_CEN, 8, sd.HB_EO1, 0, 2, False, True, 1, 0),
    ("s8", 4, sd.FC_INF, 8, sd.HB_EO1, 32, 2, True, False, 1, 0),
    ("u8", 4, sd.FC_SUP, 16, sd.HB_DB, 32, 2, False, False, 0, 0),
    ("u8", 6, sd.FC_CEN, 8, sd.HB_EO1, 32, 1, True, False, 1, 0),
    ("s8", 6, sd.FC_INF, 8, sd.HB_DB, 0, 1, False, False, 1, 0),
    ("u8", 6, sd.FC_SUP, 16, sd.HB_EO1, 32, 1, True, True, 1, 0),
]


@pytest.mark.parametrize("case", RX_CASES, ids=lambda c: "%s-d%d-fc%d-b%d-hb%d-R%d-S%d-%s-%s-direct%d-pad%d" % (
    c[0], c[1], c[2], c[3], c[4], c[5], c[6], "dev" if c[7] else "host", "pipe" if c[8] else "imm", c[9], c[10]))
def test_rx_parity(ctx, case):
    fmt, L, fc, bits, hb, R, S, device, pipelined, direct, pad = case
    ctx.set_option("rx_direct", direct)
    rs = np.random.RandomState(L * 131 + fc * 7 + S + R)
    n = int(1.6 * 16129) << L
    if L == 6:
        x8 = cw8(n, fmt, S)
    else:
        x8 = rand8(rs, (S, n, 2), fmt)
    cuts = [0, n // 3 + 7, n // 3 + 7 + (5 << L) * 97, n]
    cfg = dict(log2decim=L, fcpos=fc, hb_variant=hb, sample_bits=bits, nb_fec=R)
    got = run_rx(ctx, x8, fmt, cfg, cuts, device, pipelined, pad)
    exp = run_rx(ctx, widen(x8, fmt), "s16", cfg, cuts, device, pipelined, pad)
    assert got.shape == exp.shape and got.shape[1] >= 1, (got.shape, exp.shape)
    assert np.array_equal(got, exp), case


@pytest.mark.skipif(not __import__("oracle_lib").Reference.available("eo1"), reason="compiled reference not built")
def test_rx_against_reference_chain(ctx, oracle):
    """u8 bytes through the 8-bit pipe against the reference's own Decimators at sample_bits = 8 + the oracle framer / encoder"""
    from oracle_lib import Reference

    L, R = 4, 32
    x8 = cw8((2 * 16129 + 3000) << L, "u8")[0]
    x8[::7] ^= 0x5A  # (not only the carrier)
    rx = sd.RxPipe(ctx, 1, log2decim=L, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=R, input_format="u8")
    got = rx.process(x8, tv_sec=5, tv_usec=6)
    y, ss = Reference("eo1").decimators().decimate(L, sd.FC_CEN, 8, widen(x8, "u8"))
    fr = oracle.framer(nb_fec_blocks=R, sample_bytes=(ss - 1) // 8 + 1, sample_bits=ss, tv_sec=5, tv_usec=6)
    exp = fr.write(y)
    assert got.shape[0] == exp.shape[0] == 2
    for f in range(2):
        assert np.array_equal(got[f, :128], exp[f]), f
        assert np.array_equal(got[f, 128:], oracle.frame_encode(exp[f], R)), f


@pytest.mark.parametrize("blocks", [1, 16])
def test_rx_async(ctx, blocks):
    S, n, L = 4, 65536, 4
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=32)
    rs = np.random.RandomState(blocks)
    nb = 2 * blocks + (3 if blocks > 1 else 5)
    data = rand8(rs, (nb, S, n, 2), "u8")
    a = sd.RxPipe(ctx, S, input_format="u8", **cfg)
    a.set_async(depth=4, blocks=blocks)
    pinned = ctx.host_alloc((nb, S, n, 2), np.uint8)
    pinned[:] = data
    got = []
    for i in range(nb):
        a.submit(pinned[i] if i % 2 else data[i].copy(), tv_sec=i, tv_usec=0)  # pinned (in place) and pageable, mixed in a batch
        while True:
            r = a.collect(wait=False)
            if r is None:
                break
            got.append(r)
    for _ in range(8):
        r = a.collect(wait=True)
        if r is None:
            break
        got.append(r)
    # the synchronous 8-bit pipe, one call per batch (a batch is stamped with its first block's time)
    b = sd.RxPipe(ctx, S, input_format="u8", **cfg)
    exp = [b.process(np.concatenate(list(data[i:i + blocks]), axis=1), tv_sec=i, tv_usec=0) for i in range(0, nb, blocks)]
    got, exp = np.concatenate(got, axis=1), np.concatenate(exp, axis=1)
    assert got.shape == exp.shape and got.shape[1] > 0
    assert np.array_equal(got, exp)
    # refused while a batch is filling; the handle stays usable
    if blocks > 1:
        a.submit(data[0])
        with pytest.raises(sd.SdrHipError) as e:
            a.set_input_format("s16")
        assert e.value.code == -1 and a.input_format == "u8"
        a.collect(wait=True)
    a.set_input_format("s8")
    ctx.host_free(pinned)


def tx_batch(oracle, rs, S, F, R=32, lose=24):
    """S streams x F frames of received super blocks (128 of 128 + R, `lose` originals lost) and their payload samples"""
    rx = np.zeros((S, F, 128, 512), np.uint8)
    ys = []
    for s in range(S):
        y = signals.mixed(F * 16129 + 1, 7 + s)
        frames = oracle.framer(nb_fec_blocks=R).write(y)
        for f in range(F):
            full = np.concatenate([frames[f], oracle.frame_encode(frames[f], R)])
            lost = set(rs.choice(np.arange(1, 128), lose, replace=False).tolist())
            keep = [i for i in range(128 + R) if i not in lost][:128]
            rx[s, f] = full[keep]
        ys.append(y[:F * 16129])
    return rx, np.stack(ys)


def narrow(iq16):
    return (np.asarray(iq16).astype(np.int16) >> 8).astype(np.int8)


@pytest.mark.parametrize("L,path,F", [(0, "wave", 3), (1, "wave", 1), (2, "wave", 3), (3, "wave", 1), (4, "wave", 3), (5, "wave", 1),
                                      (6, "wave", 1), (3, "valu", 3), (6, "valu", 1), (4, "valu", 1)])
def test_tx_parity(ctx, oracle, L, path, F):
    ctx.set_option("interp_path", path)
    rs = np.random.RandomState(L * 10 + F)
    S = 2
    rx, ys = tx_batch(oracle, rs, S, F)
    a = sd.TxPipe(ctx, S, L, output_format="s8")
    b = sd.TxPipe(ctx, S, L)
    got, ref = [], []
    for mem in ("host", "device"):
        x = rx if mem == "host" else torch.from_numpy(rx).cuda()
        g, r = a.process(x), b.process(x)
        ctx.synchronize()
        g, r = (g, r) if mem == "host" else (g.cpu().numpy(), r.cpu().numpy())
        assert g.dtype == np.int8 and g.shape == r.shape
        got.append(g)
        ref.append(r)
    assert np.array_equal(np.concatenate(got, 1), narrow(np.concatenate(ref, 1)))
    # against the oracle's interpolators on the same payload (both calls: the histories carry over)
    oi = oracle.interpolators()
    exp = np.concatenate([oi.interpolate(L, ys[0]), oi.interpolate(L, ys[0])]) if L else np.concatenate([ys[0], ys[0]])
    assert np.array_equal(np.concatenate(got, 1)[0], narrow(exp))


def test_tx_pipelined_async_reconfigure(ctx, oracle):
    rs = np.random.RandomState(5)
    S = 2
    rx1, _ = tx_batch(oracle, rs, S, 1)
    rx2, _ = tx_batch(oracle, rs, S, 2)
    for pipelined in (False, True):
        a = sd.TxPipe(ctx, S, 4, pipelined=pipelined, output_format="s8")
        b = sd.TxPipe(ctx, S, 4, pipelined=pipelined)
        got, ref = [], []
        for i, x in enumerate([rx1, rx2, rx1]):
            if i == 2:
                for p in (a, b):
                    assert p.configure({"interp": 3})
            got.append(a.process(x))
            ref.append(b.process(x))
        if pipelined:
            got.append(a.flush())
            ref.append(b.flush())
        assert np.array_equal(np.concatenate(got, 1), narrow(np.concatenate(ref, 1)))
    # submit / collect with the meta blocks
    a = sd.TxPipe(ctx, S, 5, output_format="s8")
    b = sd.TxPipe(ctx, S, 5)
    for p in (a, b):
        p.set_async(depth=2)
        p.submit(rx2)
        p.submit(rx1)
    for _ in range(2):
        (g, g0), (r, r0) = a.collect(block0=True), b.collect(block0=True)
        assert g.dtype == np.int8 and np.array_equal(g, narrow(r)) and np.array_equal(g0, r0) and g0.shape[1] > 0


@pytest.mark.parametrize("L,path,device", [(0, "wave", False), (1, "wave", True), (4, "wave", False), (6, "wave", True), (3, "valu", False)])
def test_tx_datagrams_ragged(ctx, oracle, L, path, device):
    ctx.set_option("interp_path", path)
    rs = np.random.RandomState(L + 100)
    S = 4
    per = [tdg.stream_dgrams(oracle, rs, k, 16) for k in (3, 1, 0, 2)]  # ragged counts, one stream without a frame
    outs = []
    for fmt in ("s8", "s16"):
        p = sd.TxPipe(ctx, S, L, output_format=fmt)
        dg = [torch.from_numpy(np.stack(d) if len(d) else np.zeros((0, 512), np.uint8)).cuda() for d in per] if device else \
             [np.stack(d) if len(d) else np.zeros((0, 512), np.uint8) for d in per]
        res = p.process_datagrams(dg)
        ctx.synchronize()
        outs.append([(r[0].cpu().numpy() if device else r[0], r[2]) for r in res])
    for (g, gi), (r, ri) in zip(*outs):
        assert g.dtype == np.int8 and g.shape == r.shape and gi == ri
        assert np.array_equal(g, narrow(r))
    assert sum(o[0].shape[0] for o in outs[0]) > 0


def test_byte_counters(ctx, oracle):
    S, n = 4, 400000
    x8 = rand8(np.random.RandomState(1), (S, n, 2), "s8")
    deltas = []
    for fmt, x in (("s8", x8), ("s16", widen(x8, "s8"))):
        rx = sd.RxPipe(ctx, S, log2decim=4, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=32, input_format=fmt)
        h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        rx.process(x)
        deltas.append((ctx.counter("h2d_bytes") - h0, ctx.counter("d2h_bytes") - d0))
    assert deltas[1][0] - deltas[0][0] == 2 * S * n, deltas
    assert deltas[0][1] == deltas[1][1] > 0, deltas  # (the same frames come back)
    rx1, _ = tx_batch(oracle, np.random.RandomState(2), 2, 1)
    td = []
    for fmt in ("s8", "s16"):
        tx = sd.TxPipe(ctx, 2, 3, output_format=fmt)
        h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        tx.process(rx1)
        td.append((ctx.counter("h2d_bytes") - h0, ctx.counter("d2h_bytes") - d0))
    assert td[0][0] == td[1][0] > 0, td
    assert td[1][1] - td[0][1] == 2 * 2 * (16129 << 3), td


def test_refusals(ctx, oracle):
    rx = sd.RxPipe(ctx, 2, log2decim=2, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=0)
    assert ctx.lib.sdrhip_rx_set_input_format(rx.h, 3) == -1
    assert ctx.lib.sdrhip_rx_set_input_format(rx.h, -1) == -1
    tx = sd.TxPipe(ctx, 2, 2)
    assert ctx.lib.sdrhip_tx_set_output_format(tx.h, 1) == -1  # U8 is no Tx format
    assert ctx.lib.sdrhip_tx_set_output_format(tx.h, 7) == -1
    with pytest.raises(ValueError):
        sd.TxPipe(ctx, 1, 2, output_format="u8")
    # 8-bit device input with a stride that is not a multiple of 8 samples: EALIGN, nothing consumed
    rx.set_input_format("u8")
    n = 16129 * 5
    x8 = rand8(np.random.RandomState(3), (2, n, 2), "u8")
    t = torch.zeros((2, n + 4, 2), dtype=torch.uint8, device="cuda")
    t[:, :n] = torch.from_numpy(x8).cuda()
    out = torch.zeros((2, 8, 128, 512), dtype=torch.uint8, device="cuda")
    nf = C.c_size_t(0)
    rc = ctx.lib.sdrhip_rx_process(rx.h, C.c_void_p(t.data_ptr()), n, n + 4, 0, 0, C.c_void_p(out.data_ptr()), 8 * 128 * 512, C.byref(nf), sd.MEM_DEVICE)
    assert rc == -4
    got = rx.process(torch.from_numpy(x8).cuda())
    fresh = sd.RxPipe(ctx, 2, log2decim=2, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=0, input_format="u8").process(x8)
    assert np.array_equal(got.cpu().numpy(), fresh)
    # 8-bit device output with a stride that is not a multiple of 8 samples: EALIGN, the interpolator did not move
    tx.set_output_format("s8")
    rx1, _ = tx_batch(oracle, np.random.RandomState(4), 2, 1)
    nres = 16129 << 2  # (= 4 mod 8: a valid int16 stride, not an 8-bit one)
    o = torch.zeros((2, nres, 2), dtype=torch.int8, device="cuda")
    d = torch.from_numpy(rx1).cuda()
    no = C.c_size_t(0)
    rc = ctx.lib.sdrhip_tx_process(tx.h, C.c_void_p(d.data_ptr()), None, 1, 128 * 512, C.c_void_p(o.data_ptr()), nres, C.byref(no), sd.MEM_DEVICE)
    assert rc == -4
    g = tx.process(rx1)
    assert np.array_equal(g, sd.TxPipe(ctx, 2, 2, output_format="s8").process(rx1))
    # a pipelined Tx batch waiting / pipelined Rx frames waiting: refused until flushed
    p = sd.TxPipe(ctx, 2, 2, pipelined=True)
    p.process(rx1)
    with pytest.raises(sd.SdrHipError):
        p.set_output_format("s8")
    p.flush()
    p.set_output_format("s8")
    q = sd.RxPipe(ctx, 1, log2decim=0, fcpos=sd.FC_CEN, nb_fec=0, pipelined=True)
    q.process(np.zeros((2 * 16129, 2), np.int16))
    with pytest.raises(sd.SdrHipError):
        q.set_input_format("s8")
    q.flush()
    q.set_input_format("s8")


def _counts(ctx):
    return [ctx.kernel_timing_read(k)[1] for k in range(5)]


def test_explicit_s16_changes_nothing(ctx, oracle):
    x = signals.noise(3 * 16129 << 4, 9, 12)
    res = []
    for explicit in (False, True):
        rx = sd.RxPipe(ctx, 1, log2decim=4, fcpos=sd.FC_CEN, nb_fec=32)
        tx = sd.TxPipe(ctx, 1, 4)
        if explicit:
            rx.set_input_format("s16")
            tx.set_output_format("s16")
        ctx.kernel_timing(True)
        _counts(ctx)
        f = rx.process(x, tv_sec=1, tv_usec=2)
        iq = tx.process(f[:1, :128])
        ctx.synchronize()
        res.append((f, iq, rx.last_plan(), _counts(ctx)))
        ctx.kernel_timing(False)
    (f0, i0, p0, c0), (f1, i1, p1, c1) = res
    assert np.array_equal(f0, f1) and np.array_equal(i0, i1) and i0.dtype == np.int16
    assert p0 == p1 and c0 == c1 and c0[4] == 0, (c0, c1)
