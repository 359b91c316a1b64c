"""Per-stream input format (sdrhip_rx_set_stream_format / RxPipe.set_stream_formats): 8- and 16-bit IQ rows in one call, unpacked by
K0x (rx_unpack_mixed_kernels.hip).  Every comparison is byte equality.  The yardsticks: frames formed in numpy alone (`b - 128` for
u8, `b` for s8) through the oracle framer and encoder -- at log2decim = 0 and sample_bits = 16 a frame carries the widened input
verbatim --, S one-stream pipes with set_input_format(fmt[s]), and the oracle chain on the numpy-widened samples.
W = K0x's row samples per workgroup (4096); a lane's chunk is 4 (int16) or 8 (8-bit) samples."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_rx_egress import ctx, dgram_calls, mismatches, ragged_blocks, rounds, stamps, torch_first  # noqa: F401  (fixtures)
from test_gpu_rx_ragged_async import rand_block
from test_gpu_rx_stream_bits import per_stream, same, yardstick
from test_gpu_rx_stream_fec import code

pytestmark = pytest.mark.gpu

F = 16129
W = 4096
EBUSY, EINVAL = -6, -1
FMT6 = ["s16", "u8", "s8", "u8", "s16", "s8"]
BYTES = {"s16": 4, "u8": 2, "s8": 2}
R_OPEN = 2  # recovery blocks of the cases that show K0x in the open


def widen(x, fmt):
    """what the reference's sources make of their buffers (RtlSdrSource.cpp:542-553, HackRFSource.cpp:661-674), in numpy alone"""
    a = np.asarray(x)
    if fmt == "s16":
        return a
    return (a.astype(np.int16) - 128).astype(np.int16) if fmt == "u8" else a.astype(np.int16)


def raw(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


class Verbatim:
    """per stream: the oracle framer and encoder over the widened samples (decimate1 at sample size 16 is the identity)"""

    def __init__(self, oracle, fmts, R):
        self.o, self.fmts, self.R = oracle, fmts, R
        self.fr = [oracle.framer(nb_fec_blocks=R, sample_bytes=2, sample_bits=16) for _ in fmts]

    def step(self, xs, secs, usecs):
        out = []
        for s, x in enumerate(xs):
            if len(x) == 0:
                out.append(np.zeros((0, 128 + self.R, 512), np.uint8))
                continue
            self.fr[s].s.tv_sec, self.fr[s].s.tv_usec = int(secs[s]), int(usecs[s])
            fr = self.fr[s].write(widen(x, self.fmts[s]))
            out.append(np.stack([np.concatenate([f, self.o.frame_encode(f, self.R)]) for f in fr]) if len(fr)
                       else np.zeros((0, 128 + self.R, 512), np.uint8))
        return out


def joined(per_call):
    """per stream, the frames of a sequence of calls one after the other"""
    S = len(per_call[0])
    return [np.concatenate([np.asarray(c[s]).reshape(-1, np.asarray(c[s]).shape[-2], 512) for c in per_call]) for s in range(S)]


# ------------------------------------------------------------------------------------------------ 1. K0x in the open
_OPEN = {}


def open_calls(oracle):
    """synchronous calls whose per-stream counts walk through 0, 1, 7, 8, 9, W - 1, W, W + 1 (stream s starts s steps into the walk),
    then one that tops every stream past its first frame boundary: every sample of the walk reaches a delivered frame.  Made once,
    with the frames numpy and the oracle expect"""
    if not _OPEN:
        walk = [0, 1, 7, 8, 9, W - 1, W, W + 1]
        rs = np.random.RandomState(5)
        S = len(FMT6)
        plans = [[walk[(k + s) % len(walk)] for s in range(S)] for k in range(len(walk))]
        plans.append([F - sum(walk) + 3 + s for s in range(S)])
        chain = Verbatim(oracle, FMT6, R_OPEN)
        calls, exp = [], []
        for k, counts in enumerate(plans):
            xs = [rand_block(rs, [counts[s]], FMT6[s])[0] for s in range(S)]
            secs, usecs = stamps(k, S)
            calls.append((xs, counts, secs, usecs))
            exp.append(chain.step(xs, secs, usecs))
        _OPEN["calls"], _OPEN["exp"] = calls, joined(exp)
        assert [e.shape[0] for e in _OPEN["exp"]] == [1] * S
    return _OPEN["calls"], _OPEN["exp"]


def open_pipe(ctx, fmts=FMT6):
    import sdrdaemon_amd as sd

    rx = sd.RxPipe(ctx, len(fmts), log2decim=0, fcpos=sd.FC_CEN, sample_bits=16, nb_fec=R_OPEN)
    rx.set_stream_formats(fmts)
    assert [rx.stream_format(s) for s in range(len(fmts))] == list(fmts)
    return rx


def test_open_host_memory(ctx, oracle):
    calls, exp = open_calls(oracle)
    rx = open_pipe(ctx)
    got = []
    for xs, counts, secs, usecs in calls:
        fr, nf = rx.process_ragged(xs, None, secs, usecs)
        got.append(per_stream(fr, nf))
    same(joined(got), exp, "host rows")


def device_rows(xs, counts, fill):
    """uint8 device rows (S, 4 * in_stride): row s holds its samples at its start, `fill` everywhere behind them"""
    import torch

    stride = max((max(counts) + 3) & ~3, 4)
    buf = np.full((len(xs), 4 * stride), fill, np.uint8)
    for s, x in enumerate(xs):
        b = raw(x)
        buf[s, :b.size] = b
    return torch.from_numpy(buf).cuda()


def test_open_device_memory(ctx, oracle):
    """the caller's device rows read in place; the bytes behind each row's count hold 0x00 in one run and 0xa5 in the other: the
    frames are the same, and the expected ones"""
    calls, exp = open_calls(oracle)
    runs = []
    for fill in (0x00, 0xA5):
        rx = open_pipe(ctx)
        got = []
        for xs, counts, secs, usecs in calls:
            fr, nf = rx.process_ragged(device_rows(xs, counts, fill), counts, secs, usecs)
            got.append(per_stream(fr.cpu().numpy(), nf))
        runs.append(joined(got))
    same(runs[0], runs[1], "two fills")
    same(runs[0], exp, "device rows")


# ------------------------------------------------------------------------------------------------ 2. packed asynchronous batches
FMT_B = ["u8", "s16", "u8", "s8", "s16", "s8"]
# the format sets of this section: the mixed array (K0x), and six streams of one bank-wide format set with set_input_format and no
# array (K0p: the same chunk walk as its own kernel)
SETS = {"mixed": FMT_B, "s16": ["s16"] * 6, "u8": ["u8"] * 6, "s8": ["s8"] * 6}
_BATCH = {}


def batch_blocks(oracle, fmts=FMT_B):
    """three batches of three blocks.  Batch 0: segments of 1..9 samples (every chunk straddles a boundary), an odd 8-bit row in
    front of an int16 row (block 0: rows 0 -> 1; 5 + 3 + 7 odd in front of row 4), two odd 8-bit rows in front of one (block 1,
    rows 0 and 2 of 3 and 5 in front of row 4: aligned again), zero-count rows between them.  Batch 1: totals that cross W with a
    segment boundary inside the chunk that holds sample W (W + 2, W + 1), inside the last chunk of the first workgroup (W - 3, W - 1),
    a row whose first segment is empty.  Batch 2: long int16 segments behind 4097 and 2049 8-bit samples (whole chunks 2 bytes off a
    dword), then the block that tops every stream past its frame boundary.  (The rows named are FMT_B's; a bank-wide set runs the same
    counts: an all-8-bit one has odd rows in front of every other row, an all-int16 one none.)  Made once per format set"""
    key = tuple(fmts)
    if key not in _BATCH:
        S = len(fmts)
        plans = [[[5, 9, 3, 7, 6, 1], [3, 2, 5, 0, 8, 4], [1, 0, 9, 5, 0, 2]],
                 [[W + 2, W + 1, W - 3, W + 2, W - 1, 0], [7, 6, 5, 0, 3, W + 3], [1, 9, W + 1, 3, 8, 5]],
                 [[4097, 5000, 0, 0, 3000, 77], [0, 0, 2049, 1, 4100, 0], None]]
        tot = [sum(blk[s] for b in plans for blk in b if blk) for s in range(S)]
        plans[2][2] = [F - tot[s] + 3 + s for s in range(S)]
        assert min(plans[2][2]) > 0
        rs = np.random.RandomState(6)
        chain = Verbatim(oracle, fmts, R_OPEN)
        batches, exp = [], []
        for i, plan in enumerate(plans):
            blocks = []
            for j, counts in enumerate(plan):
                secs, usecs = stamps(3 * i + j, S)
                blocks.append(([rand_block(rs, [counts[s]], fmts[s])[0] for s in range(S)], counts, secs, usecs))
            batches.append(blocks)
            both = [np.concatenate([b[0][s] for b in blocks]) for s in range(S)]
            exp.append(chain.step(both, blocks[0][2], blocks[0][3]))  # (a batch is one step with its first block's stamps)
        assert [e.shape[0] for e in joined(exp)] == [1] * S
        _BATCH[key] = (batches, exp)
    return _BATCH[key]


def bank_rows(xs, counts):
    """a bank-wide block as strided rows of the format's dtype (test_gpu_rx_ragged_async's Feed.arg(b, "strided")): padding behind a
    short row, and 3 samples of it behind the longest"""
    rows = np.full((len(xs), max(max(counts), 1) + 3, 2), 0x5A, xs[0].dtype)
    for s, x in enumerate(xs):
        rows[s, :counts[s]] = x
    return rows


FORMS = ["staged_packed", "pinned_in_place", "strided"]


@pytest.mark.parametrize("form,fset", [(form, fset) for fset in ("mixed", "s16", "u8", "s8") for form in FORMS],
                         ids=[form if fset == "mixed" else form + "-" + fset for fset in ("mixed", "s16", "u8", "s8") for form in FORMS])
def test_packed_batches(ctx, oracle, form, fset):
    """blocks = 3 in three input forms: per-stream arrays packed for the caller and staged; one packed buffer of pinned memory used in
    place (its upload is exactly sum n * bytes(fmt)); strided rows of 4-byte units (a bank-wide set: of samples).  Each form's frames
    equal numpy's, so each other's.  fset "mixed": the array is set and K0x unpacks; "s16" / "u8" / "s8": set_input_format alone, K0p"""
    import sdrdaemon_amd as sd

    fmts = SETS[fset]
    batches, exp = batch_blocks(oracle, fmts)
    if fset == "mixed":
        rx = open_pipe(ctx, fmts)
    else:
        rx = sd.RxPipe(ctx, len(fmts), log2decim=0, fcpos=sd.FC_CEN, sample_bits=16, nb_fec=R_OPEN)
        rx.set_input_format(fset)
        assert [rx.stream_format(s) for s in range(len(fmts))] == fmts
    rx.set_async(depth=2, blocks=3)
    pinned = []
    try:
        for i, blocks in enumerate(batches):
            up0 = ctx.counter("h2d_bytes")
            for xs, counts, secs, usecs in blocks:
                # (the array set: bytes, or a list that the engine packs; bank-wide: samples of the format's dtype)
                flat = np.concatenate([raw(x) for x in xs]) if fset == "mixed" else np.concatenate(xs).reshape(-1)
                if form == "staged_packed":
                    rx.submit_ragged(xs if fset == "mixed" else flat, counts, secs, usecs)
                elif form == "pinned_in_place":
                    buf = ctx.host_alloc((max(flat.size, 1),), flat.dtype)
                    pinned.append(buf)
                    buf[:flat.size] = flat
                    rx.submit_ragged(buf[:flat.size], counts, secs, usecs)
                elif fset == "mixed":
                    rx.submit_ragged(device_rows(xs, counts, 0x5A).cpu().numpy(), counts, secs, usecs)
                else:
                    rx.submit_ragged(bank_rows(xs, counts), counts, secs, usecs)
            up = ctx.counter("h2d_bytes") - up0
            want = sum(c * BYTES[f] for _, counts, _, _ in blocks for c, f in zip(counts, fmts))
            print(fset, form, "batch", i, "h2d_bytes", up, "sum n * bytes(fmt)", want)
            assert up == want, (fset, form, i, up, want)
            same(rx.collect_ragged(), exp[i], (fset, form, i))
        assert rx.collect_ragged(wait=False) is None
    finally:
        for b in pinned:
            ctx.host_free(b)


# ------------------------------------------------------------------------------------------------ 3. one-stream pipes and the oracle
class FormatTwins:
    """S one-stream pipes, stream s with set_input_format(fmt[s]) and its own sample_bits, fecblk, centre frequency and rate"""

    def __init__(self, ctx, fmts, bits, fec, fc, rate, **cfg):
        import sdrdaemon_amd as sd

        self.p = [sd.RxPipe(ctx, 1, input_format=fmts[s], sample_bits=bits[s], nb_fec=fec[s], center_frequency_khz=fc[s], sample_rate=rate[s],
                            **cfg) for s in range(len(fmts))]

    def ragged(self, xs, secs, usecs):
        return [p.process(np.ascontiguousarray(xs[s]), int(secs[s]), int(usecs[s])) for s, p in enumerate(self.p)]


CASES = {"decimate16_cen": dict(L=4, fc=2, opts={"decim_path": "mfma", "mfma_span": 1024, "rx_direct": "1"}, path="mfma"),
         "decimate4_inf": dict(L=2, fc=0, opts={}, path=None)}
RESTORE = {"decim_path": "auto", "mfma_span": 0, "rx_direct": "1"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_stream_pipes_and_oracle(ctx, oracle, case):
    """formats mixed, set_stream_bits [8, 12, 8, 16], a stream meta array and two fecblk values: two synchronous calls (a stream idle
    in the second), then a departure-order batch of two blocks.  The bank's frames equal the one-stream pipes', and those equal the
    oracle chain (decimators at the stream's size over the numpy-widened samples, framer, encoder)"""
    import sdrdaemon_amd as sd

    c = CASES[case]
    L, fc = c["L"], c["fc"]
    fmts, bits, fec = ["u8", "s16", "s8", "s16"], [8, 12, 8, 16], [4, 8, 4, 8]
    fcs, rates = [100000 + 7 * s for s in range(4)], [250000, 625000, 1000000, 48000]
    S = len(fmts)
    for k, v in c["opts"].items():
        ctx.set_option(k, v)
    try:
        cfg = dict(log2decim=L, fcpos=fc)
        bank = sd.RxPipe(ctx, S, nb_fec=1, sample_bits=15, center_frequency_khz=1, sample_rate=2, **cfg)
        bank.set_stream_formats(fmts)
        bank.set_stream_bits(bits)
        bank.set_stream_meta(fcs, rates)
        bank.set_stream_fec(fec)
        twins = FormatTwins(ctx, fmts, bits, fec, fcs, rates, **cfg)
        decs, framers = [yardstick(oracle) for _ in range(S)], [None] * S
        rs = np.random.RandomState(40 + L)

        def block(frames, first):
            counts = [(f * F << L) + ((3 + 5 * s) << L if first else 0) for s, f in enumerate(frames)]
            xs = []
            for s, n in enumerate(counts):  # (8-bit radios: full-scale bytes; the 12-bit stream within its size)
                xs.append(rand_block(rs, [n], fmts[s])[0] if fmts[s] != "s16" else
                          rs.randint(-(1 << (bits[s] - 1)), 1 << (bits[s] - 1), size=(n, 2)).astype(np.int16))
            return xs, counts

        def chain(xs, secs, usecs):
            out = []
            for s in range(S):
                if len(xs[s]) == 0:
                    out.append(np.zeros((0, 128 + fec[s], 512), np.uint8))
                    continue
                y, ss = decs[s].decimate(L, fc, bits[s], np.ascontiguousarray(widen(xs[s], fmts[s])))
                if framers[s] is None:
                    framers[s] = oracle.framer(nb_fec_blocks=fec[s], sample_bytes=(ss - 1) // 8 + 1, sample_bits=ss,
                                               center_frequency_khz=fcs[s], sample_rate=rates[s])
                framers[s].s.tv_sec, framers[s].s.tv_usec = int(secs[s]), int(usecs[s])
                fr = framers[s].write(y)
                out.append(np.stack([np.concatenate([f, oracle.frame_encode(f, fec[s])]) for f in fr]) if len(fr)
                           else np.zeros((0, 128 + fec[s], 512), np.uint8))
            return out

        total = 0
        for k, frames in enumerate([[1, 1, 1, 1], [1, 0, 0, 1]]):
            xs, counts = block(frames, k == 0)
            secs, usecs = stamps(k, S)
            got, nf = bank.process_ragged(xs, counts, secs, usecs)
            exp = twins.ragged(xs, secs, usecs)
            same(per_stream(got, nf), exp, (case, k, "one-stream pipes"))
            same(exp, chain(xs, secs, usecs), (case, k, "oracle chain"))
            assert bank.last_plan()["path"] == c["path"], (case, k, bank.last_plan())
            if c["path"] == "mfma":
                assert bank.last_plan()["wps"] > 0, bank.last_plan()
            total += int(sum(nf))
        # ---- a departure-order batch of two blocks (the streams' fecblk differ: departure order only)
        bank.set_async(depth=2, blocks=2)
        bank.set_egress("round_robin")
        blocks = [block([0, 1, 0, 0], False), block([1, 0, 1, 0], False)]
        secs, usecs = stamps(7, S)
        for xs, counts in blocks:
            bank.submit_ragged(xs, counts, secs, usecs)
        both = [np.concatenate([blocks[0][0][s], blocks[1][0][s]]) for s in range(S)]
        exp = twins.ragged(both, secs, usecs)
        same(exp, chain(both, secs, usecs), (case, "batch", "oracle chain"))
        dg, tags, nf, records = bank.collect_egress()
        e_dg, e_tags = rounds([np.asarray(e) for e in exp])
        assert list(nf) == [np.asarray(e).shape[0] for e in exp] and records is None
        assert dg.shape == e_dg.shape and np.array_equal(tags, e_tags) and dg.tobytes() == e_dg.tobytes()
        assert total + int(sum(nf)) >= 8
    finally:
        for k in c["opts"]:
            ctx.set_option(k, RESTORE[k])


# ------------------------------------------------------------------------------------------------ 4. equal entries
def test_equal_entries(ctx):
    """an all-u8 array with packed input delivers the frames of bank-wide set_input_format("u8")"""
    import sdrdaemon_amd as sd

    S, L = 3, 1
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=3, sample_bits=8)
    a, b = sd.RxPipe(ctx, S, **cfg), sd.RxPipe(ctx, S, input_format="u8", **cfg)
    a.set_stream_formats(["u8"] * S)
    a.set_async(depth=2, blocks=2)
    b.set_async(depth=2, blocks=2)
    rs = np.random.RandomState(12)
    total = 0
    for i, plan in enumerate([[[1, 0, 1], [0, 1, 1]], [[0, 1, 0], [1, 0, 0]]]):
        for j, frames in enumerate(plan):
            # (a stream that is fed gets an odd count: the row behind it starts 2 bytes off a dword)
            counts = [(f * F << L) + 2 * s + 1 if f else 0 for s, f in enumerate(frames)]
            xs = [rand_block(rs, [n], "u8")[0] for n in counts]
            packed = np.concatenate([raw(x) for x in xs])
            a.submit_ragged(packed, counts, 20 + i, j)
            b.submit_ragged(packed, counts, 20 + i, j)
        ga, gb = a.collect_ragged(), b.collect_ragged()
        same(ga, gb, ("equal", i))
        total += sum(g.shape[0] for g in ga)
    assert total >= 4


# ------------------------------------------------------------------------------------------------ 5. contract
def test_setter_refusals(ctx):
    import sdrdaemon_amd as sd

    S = 3
    fm = ["u8", "s16", "s8"]
    a = sd.RxPipe(ctx, S, log2decim=0, nb_fec=R_OPEN)
    a.set_stream_formats(fm)
    names = lambda: [a.stream_format(s) for s in range(S)]  # noqa: E731
    assert ctx.lib.sdrhip_rx_set_stream_format(a.h, (C.c_int * S)(0, 3, 1)) == EINVAL and names() == fm
    assert ctx.lib.sdrhip_rx_set_stream_format(a.h, (C.c_int * S)(-1, 0, 1)) == EINVAL and names() == fm
    with pytest.raises(ValueError):
        a.set_stream_formats(["u8", "u16", "s8"])
    with pytest.raises(ValueError):
        a.set_stream_formats(["u8", "s16"])
    assert names() == fm
    f = C.c_int(9)
    assert ctx.lib.sdrhip_rx_get_stream_format(a.h, S, C.byref(f)) == EINVAL and f.value == 9
    # ---- a batch being filled, then in flight
    a.set_async(depth=2, blocks=2)
    rs = np.random.RandomState(3)
    xs = [rand_block(rs, [40 + s], fm[s])[0] for s in range(S)]
    a.submit_ragged(xs, None, 1, 2)
    assert code(a.set_stream_formats, ["s16"] * S) == EINVAL and code(a.set_stream_formats, None) == EINVAL and names() == fm
    a.submit_ragged(xs, None, 1, 3)
    assert code(a.set_stream_formats, ["s16"] * S) == EINVAL and names() == fm
    assert a.collect_ragged() is not None
    a.set_input_format("u8")  # (allowed, its value unused while the array is set)
    assert names() == fm
    a.set_stream_formats(["s8", "s8", "u8"])
    assert names() == ["s8", "s8", "u8"]
    a.set_stream_formats(None)
    assert names() == ["u8"] * S  # (bank-wide again: set_input_format's value)
    # ---- a pipelined pipe
    p = sd.RxPipe(ctx, 2, pipelined=True, log2decim=0, nb_fec=R_OPEN)
    assert code(p.set_stream_formats, ["u8", "s16"]) == EINVAL and p.stream_format(1) == "s16"


def test_set_input_format_is_refused_with_batches_about(ctx):
    """(the rule the new setter copies, on the same handle)"""
    import sdrdaemon_amd as sd

    a = sd.RxPipe(ctx, 2, log2decim=0, nb_fec=R_OPEN)
    a.set_stream_formats(["u8", "s16"])
    a.set_async(depth=2, blocks=2)
    a.submit_ragged([np.zeros((8, 2), np.uint8), np.zeros((8, 2), np.int16)], None)
    assert code(a.set_input_format, "s8") == EINVAL
    assert a.collect_ragged() is not None
    a.set_input_format("s8")
    assert [a.stream_format(s) for s in range(2)] == ["u8", "s16"]


def test_uniform_entries_are_refused_and_consume_nothing(ctx):
    """process(), submit() and pipelined mode are refused while the array is set; the refused calls leave frames and state as on
    one-stream pipes that never saw them; after set_stream_formats(None) process() continues the same streams"""
    import sdrdaemon_amd as sd

    S, L = 3, 1
    fm = ["u8", "s16", "s8"]
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN)
    a = sd.RxPipe(ctx, S, nb_fec=3, **cfg)
    twins = FormatTwins(ctx, fm, [16] * S, [3] * S, [435000] * S, [625000] * S, **cfg)
    a.set_stream_formats(fm)
    rs = np.random.RandomState(21)
    n = (F << L) // 2 + 11
    x16 = rs.randint(-32768, 32768, size=(S, 64, 2)).astype(np.int16)
    for k in range(3):
        xs = [rand_block(rs, [n], f)[0] for f in fm]
        secs, usecs = stamps(k, S)
        if k == 1:
            assert code(a.process, x16) == EINVAL and code(a.submit, x16) == EINVAL
            assert ctx.lib.sdrhip_rx_set_pipelined(a.h, 1) == EINVAL
        got, nf = a.process_ragged(xs, None, secs, usecs)
        same(per_stream(got, nf), twins.ragged(xs, secs, usecs), ("ragged", k))
    a.set_stream_formats(None)
    for p in twins.p:
        p.set_input_format("s16")
    x = rs.randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)
    got = a.process(x, 50, 60)
    exp = twins.ragged(list(x), [50] * S, [60] * S)
    assert got.shape[1] == 1
    same(list(got), exp, "uniform again")


def test_datagram_entries_ignore_the_array(oracle, ctx):
    import sdrdaemon_amd as sd

    calls = dgram_calls(oracle)
    S = len(calls[0])
    a, b = sd.RxPipe(ctx, S, log2decim=0, nb_fec=R_OPEN), sd.RxPipe(ctx, S, log2decim=0, nb_fec=R_OPEN)
    a.set_stream_formats(["u8", "s16", "s8", "u8", "s16"])
    total = 0
    for i in (0, 1, 2):
        ga, gb = a.process_datagrams(calls[i], 5, i), b.process_datagrams(calls[i], 5, i)
        same([f for f, _ in ga], [f for f, _ in gb], ("datagrams", i))
        assert [r for _, r in ga] == [r for _, r in gb]
        total += sum(np.asarray(f).shape[0] for f, _ in ga)
    assert total > 0 and mismatches(ctx) == 0


def test_launch_classes_of_a_handle_that_never_called_the_setter(ctx):
    """one stream-order ragged batch (int16, decimate2_cen, 8 recovery blocks): one unpack launch in the convert class, one decimator
    launch, one encoder launch, as before this setter existed; with the array set K0x stands where K0p stood: the same classes and
    counts"""
    import sdrdaemon_amd as sd

    S, L = 3, 1
    rs = np.random.RandomState(33)
    xs, counts = ragged_blocks(rs, S, L, [1, 2, 1], True)
    res = []
    for fm in (None, ["s16"] * S):
        rx = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=8)
        if fm:
            rx.set_stream_formats(fm)
        rx.set_async(depth=2, blocks=1)
        ctx.kernel_timing(True)
        try:
            [ctx.kernel_timing_read(k) for k in range(5)]
            rx.submit_ragged(xs if fm else np.concatenate(xs).reshape(-1), counts, 1, 2)
            frames = rx.collect_ragged()
            ctx.synchronize()
            res.append((frames, [ctx.kernel_timing_read(k)[1] for k in range(5)]))
        finally:
            ctx.kernel_timing(False)
    print("launches per class", res[0][1], res[1][1])
    assert res[0][1] == [1, 0, 1, 0, 1]  # K_DECIMATE, K_INTERPOLATE, K_FEC_ENCODE, K_FEC_DECODE, K_CONVERT
    assert res[1][1] == res[0][1]
    same(res[0][0], res[1][0], "K0x against K0p")
