"""Ragged Rx bank (sdrhip_rx_process_ragged, sdrhip_decimate_ragged, sdrhip_rx_frames_view_ragged).

Every stream of a bank takes its own number of samples per call, with its own stamp.  Per stream the bank must produce byte for
byte what a one-stream pipe with the same config produces when it is fed that stream's samples and stamps, call after call: frame
contents, recovery blocks, meta blocks, frameIndex.  Also against the compiled reference decimators + the oracle framer / encoder,
equal-count calls against sdrhip_rx_process, mixed uniform / ragged sequences with reconfiguration, 8-bit input, device memory with
a last row exactly as long as its count, the zero-copy view, and the refusals (nothing consumed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sdrdaemon_amd as sd

pytestmark = pytest.mark.gpu

F = 16129  # decimated samples per frame


@pytest.fixture
def ctx():
    assert sd.device_count() > 0
    return sd.Context(0)


def rand_iq(rs, S, n, bits=16):
    hi = 1 << (bits - 1)
    return rs.randint(-hi, hi, size=(S, max(n, 1), 2)).astype(np.int16)


def counts_for(L, S, k):
    """count sequences with zeros, counts below 2^L, counts that are not multiples of 2^L and frames that straddle calls"""
    u, f = 1 << L, F << L
    base = [[0, u - 1, f + 3 * u + 1, f // 3], [f // 2 + 7, 0, f + 5, 2 * f + u], [f, f // 2, 0, 3]][k % 3]
    return [base[s % 4] + (s // 4) * (u + 1) for s in range(S)]


class Twins:
    """S one-stream pipes: the expected result of a ragged bank"""

    def __init__(self, ctx, S, **cfg):
        self.p = [sd.RxPipe(ctx, 1, **cfg) for _ in range(S)]

    def process(self, x, counts, secs, usecs):
        return [p.process(np.ascontiguousarray(x[s, :counts[s]]), int(secs[s]), int(usecs[s])) for s, p in enumerate(self.p)]

    def reconfigure(self, **kw):
        for p in self.p:
            p.reconfigure(**kw)

    def set_input_format(self, fmt):
        for p in self.p:
            p.set_input_format(fmt)


def check_call(got, nf, exp, where):
    assert len(nf) == len(exp)
    for s, e in enumerate(exp):
        assert nf[s] == e.shape[0], (where, s, nf[s], e.shape[0])
        assert np.array_equal(got[s, :nf[s]], e), (where, s)


def run_parity(ctx, S, cfg, calls, seed=1, bits=16, device=False):
    rs = np.random.RandomState(seed)
    bank = sd.RxPipe(ctx, S, **cfg)
    twins = Twins(ctx, S, **cfg)
    total = 0
    for k, counts in enumerate(calls):
        x = rand_iq(rs, S, max(counts), bits)
        secs = rs.randint(0, 1 << 31, size=S)
        usecs = rs.randint(0, 1000000, size=S)
        xin = torch.from_numpy(x).cuda() if device else x
        got, nf = bank.process_ragged(xin, counts, secs, usecs)
        if device:
            ctx.synchronize()
            got = got.cpu().numpy()
        check_call(got, nf, twins.process(x, counts, secs, usecs), (cfg, k))
        total += int(nf.sum())
    return bank, total


@pytest.mark.parametrize("hb", [sd.HB_EO1, sd.HB_DB])
@pytest.mark.parametrize("fcpos", [sd.FC_INF, sd.FC_SUP, sd.FC_CEN])
@pytest.mark.parametrize("L", range(7))
def test_parity_decim_fcpos_variant(ctx, L, fcpos, hb):
    cfg = dict(log2decim=L, fcpos=fcpos, hb_variant=hb, sample_bits=16, nb_fec=8)
    _, total = run_parity(ctx, 4, cfg, [counts_for(L, 4, k) for k in range(3)], seed=L * 10 + fcpos * 2 + hb)
    assert total >= 4


@pytest.mark.parametrize("R", [0, 1, 8, 32, 128])
def test_parity_nb_fec(ctx, R):
    cfg = dict(log2decim=3, fcpos=sd.FC_CEN, sample_bits=16, nb_fec=R)
    run_parity(ctx, 5, cfg, [counts_for(3, 5, k) for k in range(4)], seed=100 + R)


@pytest.mark.parametrize("bits", [8, 12, 16])
def test_parity_sample_bits(ctx, bits):
    cfg = dict(log2decim=4, fcpos=sd.FC_CEN, sample_bits=bits, nb_fec=32)
    run_parity(ctx, 4, cfg, [counts_for(4, 4, k) for k in range(3)], seed=200 + bits, bits=bits)


def test_one_long_stream_beside_many_short(ctx):
    """a long stream on the matrix cores (K1mr wave groups) while VALU pieces serve the short ones, in one launch"""
    L = 4
    S = 24
    long_n, short = (40 * F + 1234) << L, [17, 0, 65536, (F << L) // 7, 3]
    calls = [[long_n] + [short[(s + k) % 5] for s in range(1, S)] for k in range(3)]
    bank, total = run_parity(ctx, S, dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=32), calls, seed=7, device=True)
    plan = bank.last_plan()
    assert plan["path"] == "mfma" and plan["wps"] > 0, plan
    assert plan["npieces"] > S, plan  # (every short stream has a piece of its own)
    assert total >= 120


@pytest.mark.parametrize("opt", [("decim_path", "valu"), ("decim_path", "mfma"), ("rx_direct", "0"), ("rx_direct", "1"), None])
def test_parity_under_context_options(ctx, opt):
    """forced valu runs K1r; forced mfma, and the default for a call this big, run K1mr: frame-direct stores with rx_direct = 1 (the
    default), stream order + K2r with 0"""
    if opt:
        ctx.set_option(*opt)
    L = 4
    calls = [[(33 * F + 11) << L, 100, 0, (F << L) + 9], [5, (34 * F) << L, (F << L) // 2, 0]]
    bank, _ = run_parity(ctx, 4, dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=16), calls, seed=9)
    plan = bank.last_plan()
    if opt == ("decim_path", "valu"):
        assert plan["path"] == "valu" and plan["nseg"] >= 4, plan
    else:
        assert plan["path"] == "mfma" and plan["wps"] > 0, plan


def test_forced_mfma_on_short_calls(ctx):
    """decim_path = mfma on calls below the automatic threshold: K1mr with streams too short for a span on pieces alone"""
    ctx.set_option("decim_path", "mfma")
    L = 3
    calls = [counts_for(L, 4, k) for k in range(3)]
    bank, _ = run_parity(ctx, 4, dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=8), calls, seed=19)
    assert bank.last_plan()["path"] == "mfma"


@pytest.mark.skipif(not __import__("oracle_lib").Reference.available("eo1"), reason="compiled reference not built")
@pytest.mark.parametrize("L,fcpos,R", [(4, sd.FC_CEN, 32), (3, sd.FC_INF, 8), (5, sd.FC_SUP, 0)])
def test_against_reference_chain(ctx, oracle, L, fcpos, R):
    """per stream: the compiled reference decimators, the oracle framer with that stream's stamps, frame_encode"""
    from oracle_lib import Reference

    S = 3
    rs = np.random.RandomState(L)
    bank = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, sample_bits=16, nb_fec=R, center_frequency_khz=435000, sample_rate=625000)
    refs = [Reference("eo1").decimators() for _ in range(S)]
    framers = [None] * S
    got = [[] for _ in range(S)]
    exp = [[] for _ in range(S)]
    calls = [[(F << L) + 77, 0, (2 * F + 5) << L], [(F << L) // 2, (F + 3) << L, 1], [(F << L), (F << L) // 3 + 1, (F << L)]]
    for k, counts in enumerate(calls):
        x = rand_iq(rs, S, max(counts))
        secs, usecs = [1000 + 10 * k + s for s in range(S)], [37 * k + s for s in range(S)]
        g, nf = bank.process_ragged(x, counts, secs, usecs)
        for s in range(S):
            got[s].extend(list(g[s, :nf[s]]))
            if counts[s] >> L == 0:  # (the reference's unsigned loop bound wraps on a call without a whole output sample)
                continue
            y, ss = refs[s].decimate(L, fcpos, 16, np.ascontiguousarray(x[s, :counts[s]]))
            if framers[s] is None:
                framers[s] = oracle.framer(nb_fec_blocks=R, sample_bytes=(ss - 1) // 8 + 1, sample_bits=ss)
            framers[s].s.tv_sec, framers[s].s.tv_usec = secs[s], usecs[s]
            exp[s].extend(list(framers[s].write(y)))
    for s in range(S):
        assert len(got[s]) == len(exp[s]) >= 1, s
        for f in range(len(exp[s])):
            assert np.array_equal(got[s][f][:128], exp[s][f]), (s, f)
            if R:
                assert np.array_equal(got[s][f][128:], oracle.frame_encode(exp[s][f], R)), (s, f)


def test_equal_counts_match_uniform_call(ctx):
    """equal counts and stamps take the ragged kernels (there is no short cut to sdrhip_rx_process) and give its bytes"""
    rs = np.random.RandomState(3)
    S, L = 6, 4
    a = sd.RxPipe(ctx, S, log2decim=L, nb_fec=32)
    b = sd.RxPipe(ctx, S, log2decim=L, nb_fec=32)
    for k, n in enumerate([(F << L) + 333, 65536, (3 * F) << L]):
        x = rand_iq(rs, S, n)
        g, nf = a.process_ragged(x, [n] * S, 5 + k, 6)
        e = b.process(x, 5 + k, 6)
        assert list(nf) == [e.shape[1]] * S
        assert np.array_equal(g, e)


def test_equal_counts_headline_shape(ctx):
    """8 x 2^25, device memory: the ragged call with equal counts (the ragged kernels: K1mr frame-direct, the frame-list encoder) gives
    the bytes and counts of sdrhip_rx_process"""
    S, n = 8, 1 << 25
    x = torch.randint(-32768, 32768, (S, n, 2), dtype=torch.int16, device="cuda")
    a = sd.RxPipe(ctx, S, log2decim=4, nb_fec=32)
    b = sd.RxPipe(ctx, S, log2decim=4, nb_fec=32)
    for k in range(2):
        g, nf = a.process_ragged(x, [n] * S, 10 + k, 0)
        e = b.process(x, 10 + k, 0)
        ctx.synchronize()
        assert list(nf) == [e.shape[1]] * S
        assert torch.equal(g, e)
        pa, pb = a.last_plan(), b.last_plan()  # K1mr with the uniform launch's geometry
        assert pa["path"] == pb["path"] == "mfma" and (pa["span"], pa["head"]) == (pb["span"], pb["head"]), (pa, pb)
        assert pa["wps"] == S * pb["wps"] and pa["npieces"] == S * pb["npieces"], (pa, pb)


def test_mixed_uniform_ragged_and_reconfigure(ctx):
    """uniform, ragged, uniform on diverged streams, reconfigure (fecblk, decim) between ragged calls; against twin pipes"""
    rs = np.random.RandomState(11)
    S = 4
    cfg = dict(log2decim=3, fcpos=sd.FC_CEN, nb_fec=16)
    bank, twins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, S, **cfg)

    def uniform(n, sec):
        x = rand_iq(rs, S, n)
        g = bank.process(x, sec, 1)
        exp = twins.process(x, [n] * S, [sec] * S, [1] * S)
        assert g.shape[1] == max(e.shape[0] for e in exp)
        for s in range(S):
            assert np.array_equal(g[s, :exp[s].shape[0]], exp[s]), s
        assert bank.max_frames(0) == 0

    def ragged(counts, sec):
        x = rand_iq(rs, S, max(counts))
        secs, usecs = [sec + s for s in range(S)], [3 * s for s in range(S)]
        g, nf = bank.process_ragged(x, counts, secs, usecs)
        check_call(g, nf, twins.process(x, counts, secs, usecs), counts)

    L = 3
    uniform((F << L) + 100, 1)
    ragged([(F << L) // 2, 0, (2 * F << L) + 5, 7], 2)
    # diverged now: a uniform call is a ragged call with equal counts; the view of differing windows is refused
    uniform((F << L) + 4000, 3)
    with pytest.raises(sd.SdrHipError):
        bank._view("cuda")
    ragged([5, (F << L), 0, (F << L) // 3], 4)
    bank.reconfigure(nb_fec=40)
    twins.reconfigure(nb_fec=40)
    ragged([(2 * F << L), 3, (F << L) + 1, 0], 5)
    bank.reconfigure(log2decim=5, sample_rate=156250)
    twins.reconfigure(log2decim=5, sample_rate=156250)
    L = 5
    ragged([(F << L) + 9, (F << L) // 2, 0, 40], 6)
    uniform((F << L) // 2 + 1, 7)
    ragged([0, 0, 0, 0], 8)
    uniform((2 * F) << L, 9)


def test_ragged_wrap_of_some_streams_only(ctx):
    """A window of one call (rx_window = 1): stream 0's window passes the end of the area on calls where the other two stay, and its
    open frame moves to slot 0 in place, alone; then a uniform call on the unaligned bank (the ragged route).  Against twin pipes."""
    rs = np.random.RandomState(21)
    S, L = 3, 1
    cfg = dict(log2decim=L, nb_fec=8)
    ctx.set_option("rx_window", 1)
    try:
        bank, twins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, S, **cfg)
        n = (F // 2) << L  # half a frame everywhere: one slot per stream, every stream keeps an open frame
        x = rand_iq(rs, S, n)
        g = bank.process(x, 1, 2)
        assert g.shape[1] == 0 and all(e.shape[0] == 0 for e in twins.process(x, [n] * S, [1] * S, [2] * S))
        counts = [(9 * F // 4) << L, (F // 4) << L, 0]
        total = np.zeros(S, np.int64)
        for k in range(8):
            x = rand_iq(rs, S, max(counts))
            secs, usecs = [10 + k + s for s in range(S)], [5 * s for s in range(S)]
            g, nf = bank.process_ragged(x, counts, secs, usecs)
            check_call(g, nf, twins.process(x, counts, secs, usecs), k)
            total += nf
        assert list(total) == [(F // 2 + 8 * (9 * F // 4)) // F, (F // 2 + 8 * (F // 4)) // F, 0]
        n = (F << L) + 300
        x = rand_iq(rs, S, n)
        g = bank.process(x, 30, 4)
        exp = twins.process(x, [n] * S, [30] * S, [4] * S)
        assert g.shape[1] == max(e.shape[0] for e in exp)
        for s in range(S):
            assert np.array_equal(g[s, :exp[s].shape[0]], exp[s]), s
    finally:
        ctx.set_option("rx_window", 0)


def test_fecblk_change_on_unaligned_bank_with_open_frames(ctx):
    """ragged calls leave three streams at three positions, each with an open frame; the frame size changes (every open frame moves
    to slot 0 of a new area, 128 original blocks each); two more ragged calls.  Against twin pipes reconfigured at the same points."""
    rs = np.random.RandomState(22)
    S, L = 3, 1
    cfg = dict(log2decim=L, nb_fec=8)
    bank, twins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, S, **cfg)

    def ragged(counts, sec):
        x = rand_iq(rs, S, max(counts))
        secs, usecs = [sec + s for s in range(S)], [7 * s for s in range(S)]
        g, nf = bank.process_ragged(x, counts, secs, usecs)
        check_call(g, nf, twins.process(x, counts, secs, usecs), counts)
        return nf

    assert list(ragged([(2 * F + F // 3) << L, (F + F // 2) << L, (F // 4) << L], 1)) == [2, 1, 0]
    assert list(ragged([(F // 3) << L, (F + 100) << L, 6], 2)) == [0, 1, 0]  # (windows at slots 2, 2 and 0 -- samples 2 F / 3, F / 2 + 100, F / 4 + 3)
    bank.reconfigure(nb_fec=40)
    twins.reconfigure(nb_fec=40)
    assert list(ragged([(F // 2) << L, (F // 2) << L, F << L], 3)) == [1, 1, 1]
    assert list(ragged([(2 * F) << L, 0, (3 * F) << L], 4)) == [2, 0, 3]


def test_frames_view_ragged_after_uniform_and_pipelined_calls(ctx):
    """sdrhip_rx_frames_view_ragged describes what a uniform call delivered too: after a uniform call, after pipelined calls -- the one
    whose frames lie in the old area included (a wrapped window that would reach the waiting frames gets a new area) -- and after
    flush_view.  The tensors formed from (base, stride, first, count) are the frames process() copied out."""
    rs = np.random.RandomState(23)
    S, L, R = 2, 1, 8

    def same(views, frames, where):
        ctx.synchronize()
        for s in range(S):
            assert views[s].shape[0] == frames.shape[1], (where, s)
            assert np.array_equal(views[s].cpu().numpy(), np.asarray(frames[s].cpu() if torch.is_tensor(frames) else frames[s])), (where, s)

    a = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    p = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R, pipelined=True)
    # (decimated counts of test_pipelined_many_calls_wrap_the_frame_window up to its first call that keeps the old area: the last one)
    sizes = [64516, 16129, 64516, 5000, 5000, 16129, 700, 0, 5000, 64516, 48387, 64516, 48387, 48387, 64516, 150000]
    prev = np.zeros((S, 0, 128 + R, 512), np.uint8)
    for i, c in enumerate(sizes):
        x = rand_iq(rs, S, c << L)[:, :c << L]
        e = a.process(x, 100 + i, 3 * i) if c else np.zeros((S, 0, 128 + R, 512), np.uint8)
        if c:
            same(a.frames_view_ragged(), e, ("uniform", i))
        g = p.process(x, 100 + i, 3 * i)
        assert np.array_equal(g, prev), i
        same(p.frames_view_ragged(), g, ("pipelined", i))
        prev = e
    assert prev.shape[1] == 10 and g.shape[1] == 4
    last = p.flush_view()
    same(p.frames_view_ragged(), last.torch(), "flush_view")
    assert np.array_equal(last.torch().cpu().numpy(), prev)


@pytest.mark.parametrize("fmt", ["u8", "s8"])
@pytest.mark.parametrize("device", [False, True])
def test_iq8_input(ctx, fmt, device):
    rs = np.random.RandomState(5)
    S, L = 3, 4
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=32)
    bank = sd.RxPipe(ctx, S, input_format=fmt, **cfg)
    twins = Twins(ctx, S, **cfg)
    twins.set_input_format(fmt)
    for k in range(3):
        counts = counts_for(L, 3, k)
        x8 = (rs.randint(0, 256, size=(S, max(counts), 2)).astype(np.uint8) if fmt == "u8"
              else rs.randint(-128, 128, size=(S, max(counts), 2)).astype(np.int8))
        g, nf = bank.process_ragged(torch.from_numpy(x8).cuda() if device else x8, counts, 50 + k, 60)
        if device:
            ctx.synchronize()
            g = g.cpu().numpy()
        check_call(g, nf, twins.process(x8, counts, [50 + k] * S, [60] * S), (fmt, k))


def test_device_last_row_exactly_its_count(ctx):
    """device input whose last stream's row ends at n_in[S-1]: the kernels read nothing past any stream's count"""
    rs = np.random.RandomState(6)
    S, L, R = 4, 4, 32
    stride = (2 * F << L) + 64
    counts = [stride - 3, 1000, (F << L) + 17, (F << L) // 2 + 5]
    x = rand_iq(rs, S, stride)
    flat = np.concatenate([x[s].reshape(-1) for s in range(S - 1)] + [x[S - 1, :counts[-1]].reshape(-1)])
    buf = torch.from_numpy(flat).cuda()  # (S - 1) * stride + counts[-1] samples, nothing behind
    bank = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    cap = max(bank.max_frames(max(counts)), 1)
    fb = (128 + R) * 512
    out = torch.empty((S, cap, 128 + R, 512), dtype=torch.uint8, device="cuda")
    nf = (C.c_size_t * S)()
    lib = sd._lib.lib()
    sd._lib.check(lib.sdrhip_rx_process_ragged(bank.h, C.c_void_p(buf.data_ptr()), (C.c_size_t * S)(*counts), stride,
                                               (C.c_uint32 * S)(*[1] * S), (C.c_uint32 * S)(*[2] * S), C.c_void_p(out.data_ptr()),
                                               cap * fb, nf, sd.MEM_DEVICE))
    ctx.synchronize()
    exp = Twins(ctx, S, log2decim=L, nb_fec=R).process(x, counts, [1] * S, [2] * S)
    check_call(out.cpu().numpy(), list(nf), exp, "last row")


def test_frames_view_ragged_equals_copy(ctx):
    rs = np.random.RandomState(8)
    S, L = 4, 3
    a = sd.RxPipe(ctx, S, log2decim=L, nb_fec=8)
    b = sd.RxPipe(ctx, S, log2decim=L, nb_fec=8)
    for k in range(4):
        counts = counts_for(L, S, k)
        x = rand_iq(rs, S, max(counts))
        g, nf = a.process_ragged(x, counts, k, k)
        views, nv = b.process_view_ragged(torch.from_numpy(x).cuda(), counts, k, k)
        ctx.synchronize()
        assert list(nf) == list(nv)
        for s in range(S):
            assert views[s].shape[0] == nf[s]
            assert np.array_equal(views[s].cpu().numpy(), g[s, :nf[s]]), (k, s)


def test_refusals_consume_nothing(ctx):
    """each refusal returns SDRHIP_EINVAL and leaves no trace: the next call continues as if it never happened"""
    rs = np.random.RandomState(12)
    S, L, R = 3, 3, 16
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    bank, twins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, S, **cfg)
    lib = sd._lib.lib()
    fb = (128 + R) * 512

    def ragged(x, counts, sec):
        g, nf = bank.process_ragged(x, counts, sec, 0)
        check_call(g, nf, twins.process(x, counts, [sec] * S, [0] * S), counts)

    c0 = [(F << L) + 5, 100, (F << L) // 2]
    ragged(rand_iq(rs, S, max(c0)), c0, 1)
    counts = [(2 * F << L), 7, (F << L)]
    x = rand_iq(rs, S, max(counts))
    cnt, sec, nf = (C.c_size_t * S)(*counts), (C.c_uint32 * S)(*[2] * S), (C.c_size_t * S)()
    out = np.zeros((S, 4, 128 + R, 512), np.uint8)
    p, po, n = C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), x.shape[1]
    assert lib.sdrhip_rx_process_ragged(bank.h, p, None, n, sec, sec, po, 4 * fb, nf, sd.MEM_HOST) == -1
    assert lib.sdrhip_rx_process_ragged(bank.h, p, cnt, n, None, sec, po, 4 * fb, nf, sd.MEM_HOST) == -1
    assert lib.sdrhip_rx_process_ragged(bank.h, p, cnt, n, sec, None, po, 4 * fb, nf, sd.MEM_HOST) == -1
    assert lib.sdrhip_rx_process_ragged(bank.h, p, cnt, n, sec, sec, po, 4 * fb, None, sd.MEM_HOST) == -1
    assert lib.sdrhip_rx_process_ragged(bank.h, p, cnt, n - 1, sec, sec, po, 4 * fb, nf, sd.MEM_HOST) == -1  # stride < largest
    assert bank.max_frames(max(counts)) == 2
    assert lib.sdrhip_rx_process_ragged(bank.h, p, cnt, n, sec, sec, po, 2 * fb - 1, nf, sd.MEM_HOST) == -1  # room for the 2-frame stream
    # streams at different positions: no pipelined mode, no async batches
    assert lib.sdrhip_rx_set_pipelined(bank.h, 1) == -1
    with pytest.raises(sd.SdrHipError):
        bank.submit(rand_iq(rs, S, 64), 0, 0)
    ragged(x, counts, 2)  # continues seamlessly
    # pipelined mode and a batch being filled, on handles of their own; each goes on as if the refused call never happened
    piped, ptwins = sd.RxPipe(ctx, S, pipelined=True, **cfg), Twins(ctx, S, **cfg)
    assert lib.sdrhip_rx_process_ragged(piped.h, p, cnt, n, sec, sec, po, 4 * fb, nf, sd.MEM_HOST) == -1
    piped.ctx.lib.sdrhip_rx_set_pipelined(piped.h, 0)
    g, nfp = piped.process_ragged(x, counts, 2, 0)
    check_call(g, nfp, ptwins.process(x, counts, [2] * S, [0] * S), "after the pipelined refusal")
    filling, ftwins = sd.RxPipe(ctx, S, **cfg), Twins(ctx, S, **cfg)
    filling.set_async(depth=2, blocks=2)
    block = rand_iq(rs, S, 64 << L)
    filling.submit(block, 4, 0)
    assert lib.sdrhip_rx_process_ragged(filling.h, p, cnt, n, sec, sec, po, 4 * fb, nf, sd.MEM_HOST) == -1
    assert filling.collect(wait=True).shape[1] == 0  # (the partly filled batch goes out as it is)
    ftwins.process(block, [block.shape[1]] * S, [4] * S, [0] * S)
    g, nfp = filling.process_ragged(x, counts, 2, 0)
    check_call(g, nfp, ftwins.process(x, counts, [2] * S, [0] * S), "after the batch refusal")


@pytest.mark.parametrize("path", ["auto", "mfma"])
def test_decimate_ragged_against_reference_and_twins(ctx, oracle, path):
    """auto: these calls are below the matrix-core threshold (K1r); mfma: forced, the centred cascades run K1mr"""
    from oracle_lib import Reference

    ctx.set_option("decim_path", path)

    have_ref = Reference.available("eo1")
    rs = np.random.RandomState(21)
    S = 5
    for L, fcpos in [(4, sd.FC_CEN), (3, sd.FC_INF), (2, sd.FC_SUP), (6, sd.FC_CEN), (1, sd.FC_INF), (0, sd.FC_CEN)]:
        bank = sd.Decimators(ctx, S)
        singles = [sd.Decimators(ctx, 1) for _ in range(S)]
        refs = [Reference("eo1").decimators() for _ in range(S)] if have_ref else None
        ss_bank = 16
        for k in range(3):
            u = 1 << L
            counts = [[0, u - 1, 300000 + 3, 70001, 5 * u][(s + k) % 5] for s in range(S)]
            x = rand_iq(rs, S, (max(counts) + 3) & ~3)  # (device rows: a multiple of 4 samples)
            dev = k == 1
            xin = torch.from_numpy(x).cuda() if dev else x
            y, n_out, ss_new = bank.decimate_ragged(L, fcpos, ss_bank, xin, counts)
            if dev:
                ctx.synchronize()
                y = y.cpu().numpy()
            for s in range(S):
                assert n_out[s] == counts[s] >> L
                e, ss_e = singles[s].decimate(L, fcpos, ss_bank, np.ascontiguousarray(x[s, :counts[s]]))
                assert np.array_equal(y[s, :n_out[s]], e.reshape(-1, 2)), (L, fcpos, k, s)
                assert ss_e == ss_new
                if refs and n_out[s]:  # (the reference's unsigned loop bound wraps on a call without a whole output sample)
                    r, ss_r = refs[s].decimate(L, fcpos, ss_bank, np.ascontiguousarray(x[s, :counts[s]]))
                    assert np.array_equal(y[s, :n_out[s]], np.asarray(r).reshape(-1, 2)), (L, fcpos, k, s, "ref")
            if L > 0 and (fcpos == sd.FC_CEN or L >= 3):
                assert bank.last_plan()["path"] == ("mfma" if path == "mfma" and fcpos == sd.FC_CEN and L >= 2 else "valu")
