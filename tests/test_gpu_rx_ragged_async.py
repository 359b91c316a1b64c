"""Asynchronous ragged Rx entry (sdrhip_rx_submit_ragged / sdrhip_rx_collect_ragged).

Every submit appends one block per stream, each stream with its own count.  Per stream a batch must be exactly one
sdrhip_rx_process_ragged call of the stream's summed counts, stamped with its first block's stamps: frames, recovery blocks, meta
blocks and frameIndex byte for byte, and so also what one one-stream pipe per stream gives.  Also against the compiled reference
chain, the input forms (packed pinned in place, packed pageable, strided pageable, mixed), 8-bit input, the link bytes a batch
moves, the submit / collect contract and its refusals (nothing consumed), two threads, and equal counts against sdrhip_rx_submit."""
import ctypes as C

import numpy as np
import pytest

import sdrdaemon_amd as sd
from test_gpu_rx_ragged import F, Twins

pytestmark = pytest.mark.gpu

EBUSY, EINVAL = -6, -1


@pytest.fixture
def ctx():
    assert sd.device_count() > 0
    return sd.Context(0)


def block_counts(L, S, k):
    """per-block counts with zeros, counts below 2^L, counts that are not multiples of 2^L; their sums leave frames straddling
    batches"""
    u, f = 1 << L, F << L
    base = [[0, u - 1, f // 3 + 1, f // 5], [f // 2 + 7, 0, 5, f // 4 + u], [f // 3, f // 2 + 3, 0, 3], [u, f // 7, f // 3, 0]][k % 4]
    return [base[(s + k) % 4] + (s // 4) * (u + 1) for s in range(S)]


def rand_block(rs, counts, fmt="s16"):
    if fmt == "s16":
        return [rs.randint(-32768, 32768, size=(c, 2)).astype(np.int16) for c in counts]
    dt = np.uint8 if fmt == "u8" else np.int8
    return [rs.randint(0, 256, size=(c, 2)).astype(np.uint8).view(dt) for c in counts]


class Feed:
    """the blocks of a test, the input form of each submit, and the pinned buffers that must outlive their batch"""

    def __init__(self, ctx, S, L, nblocks, seed, fmt="s16", counts=None):
        rs = np.random.RandomState(seed)
        self.ctx, self.S, self.fmt = ctx, S, fmt
        self.counts = [list(counts[b]) if counts else block_counts(L, S, b) for b in range(nblocks)]
        self.x = [rand_block(rs, c, fmt) for c in self.counts]
        self.sec = [rs.randint(0, 1 << 31, size=S).astype(np.uint32) for _ in range(nblocks)]
        self.usec = [rs.randint(0, 1000000, size=S).astype(np.uint32) for _ in range(nblocks)]
        self.pinned = []

    def arg(self, b, form):
        xs = self.x[b]
        dt = xs[0].dtype
        if form == "mixed":
            form = ("pinned", "packed", "strided")[b % 3]
        if form == "strided":
            rows = np.zeros((self.S, max(max(self.counts[b]), 1) + 3, 2), dt)  # (padding between a short row and the stride)
            for s in range(self.S):
                rows[s, :self.counts[b][s]] = xs[s]
            return rows
        packed = np.concatenate(xs).reshape(-1)
        if form == "pinned" and packed.size:
            a = self.ctx.host_alloc((packed.size,), dt)
            a[:] = packed
            self.pinned.append(a)
            return a
        return packed

    def free(self):
        for a in self.pinned:
            self.ctx.host_free(a)
        self.pinned = []

    def batch(self, blocks):
        """-> (rows, per-stream sums, first-block stamps) of the blocks of one batch"""
        S = self.S
        tot = [sum(self.counts[b][s] for b in blocks) for s in range(S)]
        rows = np.zeros((S, max(max(tot), 1), 2), self.x[0][0].dtype)
        for s in range(S):
            rows[s, :tot[s]] = np.concatenate([self.x[b][s] for b in blocks]) if tot[s] else rows[s, :0]
        return rows, tot, self.sec[blocks[0]], self.usec[blocks[0]]


def run_async(rx, feed, form="packed"):
    """submit every block (collecting whenever the ring is full), then collect the rest; -> list of batches, each a list of S
    frame arrays"""
    got = []
    for b in range(len(feed.counts)):
        while True:
            try:
                rx.submit_ragged(feed.arg(b, form), feed.counts[b], feed.sec[b], feed.usec[b])
                break
            except sd.SdrHipError as e:
                assert e.code == EBUSY
                fr = rx.collect_ragged(wait=True)
                assert fr is not None
                got.append(fr)
    while True:
        fr = rx.collect_ragged(wait=True)
        if fr is None:
            break
        got.append(fr)
    return got


def expected(ctx, feed, blocks, cfg, twins=None):
    """the synchronous ragged calls (and optionally one-stream twins) fed the per-batch sums and first-block stamps"""
    S, nb = feed.S, len(feed.counts)
    sync = sd.RxPipe(ctx, S, input_format=feed.fmt, **cfg)
    out = []
    for b0 in range(0, nb, blocks):
        rows, tot, sec, usec = feed.batch(list(range(b0, min(b0 + blocks, nb))))
        g, nf = sync.process_ragged(rows, tot, sec, usec)
        exp = [g[s, :nf[s]] for s in range(S)]
        if twins is not None:
            tw = twins.process(rows, tot, sec, usec)
            for s in range(S):
                assert np.array_equal(exp[s], tw[s]), ("twin", b0, s)
        out.append(exp)
    return out


def check_batches(got, exp, where=""):
    assert len(got) == len(exp), (where, len(got), len(exp))
    n = 0
    for k, (g, e) in enumerate(zip(got, exp)):
        for s in range(len(e)):
            assert g[s].shape == e[s].shape, (where, k, s, g[s].shape, e[s].shape)
            assert np.array_equal(g[s], e[s]), (where, k, s)
            n += e[s].shape[0]
    return n


def parity(ctx, S, cfg, nblocks, blocks, depth, seed, form="packed", fmt="s16", with_twins=True):
    feed = Feed(ctx, S, cfg["log2decim"], nblocks, seed, fmt)
    rx = sd.RxPipe(ctx, S, input_format=fmt, **cfg)
    rx.set_async(depth=depth, blocks=blocks)
    got = run_async(rx, feed, form)
    feed.free()
    twins = None
    if with_twins:
        twins = Twins(ctx, S, **cfg)
        if fmt != "s16":
            twins.set_input_format(fmt)
    return check_batches(got, expected(ctx, feed, blocks, cfg, twins), (cfg, blocks, depth, form))


@pytest.mark.parametrize("blocks,depth", [(1, 1), (1, 4), (3, 1), (3, 4), (8, 1), (8, 4)])
def test_parity_blocks_and_depth(ctx, blocks, depth):
    cfg = dict(log2decim=4, fcpos=sd.FC_CEN, nb_fec=32)
    assert parity(ctx, 5, cfg, 10, blocks, depth, seed=blocks * 10 + depth) >= 4


@pytest.mark.parametrize("L,fcpos,hb", [(0, sd.FC_CEN, sd.HB_EO1), (2, sd.FC_CEN, sd.HB_DB), (4, sd.FC_INF, sd.HB_EO1),
                                        (4, sd.FC_SUP, sd.HB_DB), (4, sd.FC_CEN, sd.HB_DB), (6, sd.FC_CEN, sd.HB_EO1),
                                        (6, sd.FC_INF, sd.HB_DB)])
def test_parity_decim_fcpos_variant(ctx, L, fcpos, hb):
    cfg = dict(log2decim=L, fcpos=fcpos, hb_variant=hb, nb_fec=8)
    assert parity(ctx, 4, cfg, 7, 3, 4, seed=100 + L * 10 + fcpos * 2 + hb) >= 2


@pytest.mark.parametrize("R", [0, 8, 32, 64])
def test_parity_nb_fec(ctx, R):
    cfg = dict(log2decim=3, fcpos=sd.FC_CEN, nb_fec=R)
    parity(ctx, 4, cfg, 8, 3, 4, seed=200 + R)


@pytest.mark.skipif(not __import__("oracle_lib").Reference.available("eo1"), reason="compiled reference not built")
def test_against_reference_chain(ctx, oracle):
    """per stream and batch: the compiled reference decimators over the batch's samples, the oracle framer stamped with the
    batch's first block, frame_encode"""
    from oracle_lib import Reference

    S, L, R, blocks = 3, 4, 32, 3
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, sample_bits=16, nb_fec=R, center_frequency_khz=435000, sample_rate=625000)
    f = F << L
    feed = Feed(ctx, S, L, 9, 31, counts=[[f // 2 + 77 + 13 * b, (f // 3) * (b % 2), f // 4 + b] for b in range(9)])
    rx = sd.RxPipe(ctx, S, **cfg)
    rx.set_async(depth=4, blocks=blocks)
    got_b = run_async(rx, feed, "packed")
    refs = [Reference("eo1").decimators() for _ in range(S)]
    framers = [None] * S
    got = [[f for batch in got_b for f in batch[s]] for s in range(S)]
    exp = [[] for _ in range(S)]
    for b0 in range(0, 9, blocks):
        rows, tot, sec, usec = feed.batch(list(range(b0, b0 + blocks)))
        for s in range(S):
            if tot[s] >> L == 0:  # (the reference's unsigned loop bound wraps on a call without a whole output sample)
                continue
            y, ss = refs[s].decimate(L, sd.FC_CEN, 16, np.ascontiguousarray(rows[s, :tot[s]]))
            if framers[s] is None:
                framers[s] = oracle.framer(nb_fec_blocks=R, sample_bytes=(ss - 1) // 8 + 1, sample_bits=ss)
            framers[s].s.tv_sec, framers[s].s.tv_usec = int(sec[s]), int(usec[s])
            exp[s].extend(list(framers[s].write(y)))
    for s in range(S):
        assert len(got[s]) == len(exp[s]) >= 1, s
        for f in range(len(exp[s])):
            assert np.array_equal(got[s][f][:128], exp[s][f]), (s, f)
            assert np.array_equal(got[s][f][128:], oracle.frame_encode(exp[s][f], R)), (s, f)


def test_input_forms_give_identical_frames(ctx):
    cfg = dict(log2decim=3, fcpos=sd.FC_CEN, nb_fec=16)
    res = {}
    for form in ("pinned", "packed", "strided", "mixed"):
        feed = Feed(ctx, 6, 3, 9, 77)
        rx = sd.RxPipe(ctx, 6, **cfg)
        rx.set_async(depth=2, blocks=3)
        res[form] = run_async(rx, feed, form)
        feed.free()
    n = check_batches(res["packed"], expected(ctx, Feed(ctx, 6, 3, 9, 77), 3, cfg), "packed")
    assert n >= 4
    for form in ("pinned", "strided", "mixed"):
        check_batches(res[form], res["packed"], form)


@pytest.mark.parametrize("fmt", ["u8", "s8"])
@pytest.mark.parametrize("form", ["packed", "pinned", "strided"])
def test_iq8_input(ctx, fmt, form):
    """odd and even packed offsets (K0p's realigned loads) and the widening in one pass"""
    cfg = dict(log2decim=4, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=8)
    assert parity(ctx, 5, cfg, 8, 3, 4, seed=300 + len(form), form=form, fmt=fmt, with_twins=False) >= 2


def test_link_bytes(ctx):
    """h2d: the packed sample bytes (tables are not counted), less than S x largest x 4; d2h: exactly the frames"""
    S, L, R = 4, 2, 8
    counts = [[70000, 200001, 0, 130003]]
    feed = Feed(ctx, S, L, 1, 5, counts=counts)
    rx = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R)
    rx.set_async(depth=4, blocks=1)
    h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
    rx.submit_ragged(feed.arg(0, "packed"), counts[0], feed.sec[0], feed.usec[0])
    fr = rx.collect_ragged()
    h1, d1 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
    assert h1 - h0 == sum(counts[0]) * 4 < S * max(counts[0]) * 4
    nf = [f.shape[0] for f in fr]
    assert sum(nf) >= 3 and len(set(nf)) > 1, nf
    assert d1 - d0 == sum(nf) * (128 + R) * 512
    check_batches([fr], expected(ctx, feed, 1, dict(log2decim=L, nb_fec=R)))


def _lib_collect(rx, max_frames, wait=1):
    S = rx.nstreams
    fb = (128 + rx.nb_fec) * 512
    out = np.empty((S, max(max_frames, 1), 128 + rx.nb_fec, 512), np.uint8)
    nf = (C.c_size_t * S)()
    rc = rx.ctx.lib.sdrhip_rx_collect_ragged(rx.h, out.ctypes.data_as(C.c_void_p), max(max_frames, 1) * fb, max_frames, nf, wait)
    return rc, list(nf[:]), out


def test_contract_ebusy_max_frames_and_wait(ctx):
    S, L = 3, 2
    cfg = dict(log2decim=L, nb_fec=8)
    f = F << L
    counts = [[f + 3, 2 * f, 7], [f // 2, 5, f + 11], [f, 0, f], [3, f // 3, 2 * f], [f, f, 0], [1, 2, 3]]
    feed = Feed(ctx, S, L, 6, 9, counts=counts)
    rx = sd.RxPipe(ctx, S, **cfg)
    assert rx.collect_ragged(wait=False) is None and rx.collect_ragged(wait=True) is None  # nothing submitted
    rx.set_async(depth=1, blocks=2)
    got = []
    rx.submit_ragged(feed.arg(0, "packed"), feed.counts[0], feed.sec[0], feed.usec[0])
    assert rx.collect_ragged(wait=False) is None  # still being filled
    rx.submit_ragged(feed.arg(1, "strided"), feed.counts[1], feed.sec[1], feed.usec[1])  # launched
    with pytest.raises(sd.SdrHipError) as e:  # ring full
        rx.submit_ragged(feed.arg(2, "packed"), feed.counts[2], feed.sec[2], feed.usec[2])
    assert e.value.code == EBUSY
    rc, nf, _ = _lib_collect(rx, 0)  # too small: the batch stays, n_frames[] says how many
    assert rc == EINVAL and max(nf) > 0, (rc, nf)
    fr = rx.collect_ragged()
    assert [f.shape[0] for f in fr] == nf
    got.append(fr)
    for b in (2, 3, 4):
        rx.submit_ragged(feed.arg(b, "packed"), feed.counts[b], feed.sec[b], feed.usec[b])
        if b == 3:
            got.append(rx.collect_ragged())
    got.append(rx.collect_ragged(wait=True))  # block 4 alone: a partly filled batch goes out as it is
    assert rx.collect_ragged(wait=True) is None
    # expected: batches {0, 1}, {2, 3}, {4}
    sync = sd.RxPipe(ctx, S, **cfg)
    exp = []
    for blocks in ([0, 1], [2, 3], [4]):
        rows, tot, sec, usec = feed.batch(blocks)
        g, n = sync.process_ragged(rows, tot, sec, usec)
        exp.append([g[s, :n[s]] for s in range(S)])
    assert check_batches(got, exp) >= 2


def test_refusals_consume_nothing(ctx):
    """every refusal leaves the pipe as if the call never happened: the frames equal those of the same sequence without it"""
    S, L = 4, 3
    cfg = dict(log2decim=L, nb_fec=8)
    feed = Feed(ctx, S, L, 6, 11)
    lib = ctx.lib
    rx = sd.RxPipe(ctx, S, **cfg)
    rx.set_async(depth=4, blocks=2)
    x0 = feed.arg(0, "packed")
    n0 = (C.c_size_t * S)(*feed.counts[0])
    t = (C.c_uint32 * S)(*[0] * S)
    ptr = x0.ctypes.data_as(C.c_void_p)
    assert lib.sdrhip_rx_submit_ragged(rx.h, ptr, None, 0, t, t) == EINVAL
    assert lib.sdrhip_rx_submit_ragged(rx.h, ptr, n0, 0, None, t) == EINVAL
    assert lib.sdrhip_rx_submit_ragged(rx.h, ptr, n0, 0, t, None) == EINVAL
    assert lib.sdrhip_rx_submit_ragged(rx.h, ptr, n0, max(feed.counts[0]) - 1, t, t) == EINVAL  # stride below the largest count
    # uniform batch being filled: a ragged submit is refused
    u = np.zeros((S, 64, 2), np.int16)
    rx.submit(u, 0, 0)
    with pytest.raises(sd.SdrHipError):
        rx.submit_ragged(x0, feed.counts[0], feed.sec[0], feed.usec[0])
    # (the uniform batch is collected and its 64 samples per stream go into the reference sequence as a uniform call)
    assert rx.collect(wait=True).shape[1] == 0
    got = []
    rx.submit_ragged(x0, feed.counts[0], feed.sec[0], feed.usec[0])
    # ragged batch being filled: uniform submit / collect and synchronous calls are refused
    for call in (lambda: rx.submit(u, 0, 0), lambda: rx.collect(wait=True), lambda: rx.process(u, 0, 0),
                 lambda: rx.process_ragged(u, [64] * S, 0, 0), lambda: rx.set_input_format("u8")):
        with pytest.raises(sd.SdrHipError) as e:
            call()
        assert e.value.code == EINVAL
    rx.submit_ragged(feed.arg(1, "strided"), feed.counts[1], feed.sec[1], feed.usec[1])  # launched: in flight now
    for call in (lambda: rx.submit(u, 0, 0), lambda: rx.process(u, 0, 0), lambda: rx.process_ragged(u, [64] * S, 0, 0)):
        with pytest.raises(sd.SdrHipError) as e:
            call()
        assert e.value.code == EINVAL
    got.append(rx.collect_ragged())
    for b in (2, 3):
        rx.submit_ragged(feed.arg(b, "packed"), feed.counts[b], feed.sec[b], feed.usec[b])
    got.append(rx.collect_ragged())
    sync = sd.RxPipe(ctx, S, **cfg)
    sync.process(u, 0, 0)
    exp = []
    for blocks in ([0, 1], [2, 3]):
        rows, tot, sec, usec = feed.batch(blocks)
        g, n = sync.process_ragged(rows, tot, sec, usec)
        exp.append([g[s, :n[s]] for s in range(S)])
    assert check_batches(got, exp) >= 2
    # pipelined mode refuses the ragged async path
    p = sd.RxPipe(ctx, S, pipelined=True, **cfg)
    with pytest.raises(sd.SdrHipError) as e:
        p.submit_ragged(x0, feed.counts[0], 0, 0)
    assert e.value.code == EINVAL


def test_sync_ragged_calls_before_and_after_continue_the_streams(ctx):
    S, L = 4, 4
    cfg = dict(log2decim=L, nb_fec=32)
    feed = Feed(ctx, S, L, 8, 13)
    rx = sd.RxPipe(ctx, S, **cfg)
    sync = sd.RxPipe(ctx, S, **cfg)

    def both_sync(blocks):
        rows, tot, sec, usec = feed.batch(blocks)
        g, n = rx.process_ragged(rows, tot, sec, usec)
        e, m = sync.process_ragged(rows, tot, sec, usec)
        assert list(n) == list(m)
        for s in range(S):
            assert np.array_equal(g[s, :n[s]], e[s, :m[s]]), (blocks, s)

    both_sync([0])
    both_sync([1])  # (the streams now sit at different frame positions)
    rx.set_async(depth=4, blocks=3)
    got = []
    for b in (2, 3, 4, 5, 6):
        rx.submit_ragged(feed.arg(b, "mixed"), feed.counts[b], feed.sec[b], feed.usec[b])
    got.append(rx.collect_ragged())
    got.append(rx.collect_ragged(wait=True))
    feed.free()
    exp = []
    for blocks in ([2, 3, 4], [5, 6]):
        rows, tot, sec, usec = feed.batch(blocks)
        g, n = sync.process_ragged(rows, tot, sec, usec)
        exp.append([g[s, :n[s]] for s in range(S)])
    check_batches(got, exp)
    both_sync([7])


def test_submit_and_collect_from_two_threads(ctx):
    import threading

    S, L, blocks, nb = 4, 4, 3, 24
    cfg = dict(log2decim=L, nb_fec=32)
    feed = Feed(ctx, S, L, nb, 17)
    rx = sd.RxPipe(ctx, S, **cfg)
    rx.set_async(depth=4, blocks=blocks)
    got, errors = [], []
    done = threading.Event()

    def collector():
        try:
            while len(got) < nb // blocks:
                fr = rx.collect_ragged(wait=done.is_set(), max_frames=64)
                if fr is not None:
                    got.append(fr)
        except Exception as e:  # pragma: no cover
            errors.append(e)

    t = threading.Thread(target=collector)
    t.start()
    for b in range(nb):
        while True:
            try:
                rx.submit_ragged(feed.arg(b, "pinned"), feed.counts[b], feed.sec[b], feed.usec[b])
                break
            except sd.SdrHipError as e:
                assert e.code == EBUSY  # ring full: the collector will make room
    done.set()
    t.join(timeout=120)
    assert not t.is_alive() and not errors, errors
    feed.free()
    assert check_batches(got, expected(ctx, feed, blocks, cfg)) >= 8


def test_equal_counts_match_uniform_submit(ctx):
    S, L, n, blocks = 4, 4, 65536, 2
    cfg = dict(log2decim=L, nb_fec=32)
    feed = Feed(ctx, S, L, 6, 19, counts=[[n] * S] * 6)
    for b in range(6):
        feed.sec[b][:] = 1000 + b
        feed.usec[b][:] = 7 * b
    uni = sd.RxPipe(ctx, S, **cfg)
    uni.set_async(depth=4, blocks=blocks)
    rg = sd.RxPipe(ctx, S, **cfg)
    rg.set_async(depth=4, blocks=blocks)
    got_u, got_r = [], []
    for b in range(6):
        uni.submit(np.stack(feed.x[b]), int(feed.sec[b][0]), int(feed.usec[b][0]))
        rg.submit_ragged(feed.arg(b, "packed"), feed.counts[b], feed.sec[b], feed.usec[b])
        if b % blocks == blocks - 1:
            got_u.append(uni.collect())
            got_r.append(rg.collect_ragged())
    total = 0
    for u, r in zip(got_u, got_r):
        for s in range(S):
            assert np.array_equal(u[s], r[s]), s
            total += r[s].shape[0]
    assert total >= 4
