"""sdrhip_decimate_taps (K1t): every rate of a centred cascade in one launch.  Every comparison is bit-exact against the oracle --
oracle.decimators(bias).decimate(k, 2, ss, x[:n_used]) with one object per (stream, tap), carried across calls: what a reference
Decimators object of its own gives for decimate<2^k>_cen.  The shapes are small: at 20 000 samples the planner settles on segments
of one or two passes, so a stream is already five to ten workgroups and every one but the first rebuilds its histories by a warm-up."""
import ctypes as C

import numpy as np
import pytest
import torch

import bank_bounds_cases as B
import sdrdaemon_amd as sd
import signals
from sdrdaemon_amd import _lib
from test_gpu_bank_bounds import Buf, check_output, host, once, second_input, to_mem

pytestmark = pytest.mark.gpu

CEN = sd.FC_CEN
N1 = 20000 + 77
EINVAL, EALIGN = -1, -4


@pytest.fixture(scope="module")
def ctx():
    assert sd.device_count() > 0, "GPU tests need a GPU and libsdrhip.so"
    return sd.Context(0)


def mask_shapes(L):
    """the single highest bit, all bits, alternating bits, {1, L} and {L - 1, L}"""
    shapes = [(L,), tuple(range(1, L + 1)), tuple(range(L, 0, -2))[::-1], (1, L), (L - 1, L)]
    return sorted(set(shapes), key=shapes.index)


def used(n, L):
    return (n >> L) << L


def signal_bits(name, n, ss):
    """signal `name` of signals.ALL ("noise": signals.noise) scaled to ss effective bits"""
    x = signals.noise(n, 4321, ss) if name == "noise" else (signals.ALL[name](n) >> (16 - ss)).astype(np.int16)
    return np.ascontiguousarray(x)


def expect_tap(oracle, bias, name, ss, k, n):
    """a fresh reference object's decimate<2^k>_cen on the first n samples of the signal: (samples, sample size)"""
    return once(("tap", bias, name, ss, k, n), lambda: oracle.decimators(bias).decimate(k, CEN, ss, signal_bits(name, N1, ss)[:n]))


# ------------------------------------------------------------------------------ 1. every mask shape
@pytest.mark.parametrize("bias", [sd.HB_EO1, sd.HB_DB], ids=["eo1", "db"])
@pytest.mark.parametrize("L", [2, 3, 4, 5, 6])
def test_every_mask_shape(ctx, oracle, L, bias):
    n_used = used(N1, L)
    for name in ("noise", "mixed"):
        for ss in (8, 12, 16):
            xd = torch.from_numpy(signal_bits(name, N1, ss)).cuda()
            for mask in mask_shapes(L):
                d = sd.Decimators(ctx, 1, bias)
                outs, sizes, nu = d.decimate_taps(mask, ss, xd)
                plan = d.last_plan()
                where = (L, bias, name, ss, mask, plan)
                assert list(nu) == [n_used] and sorted(outs) == sorted(mask), where
                # the stream had at least 3 workgroups: the warm-up path ran (and the launch is the VALU cascade on K1r's grid)
                assert plan["path"] == "valu" and plan["nseg"] == B.plan_decimate_ragged(L, CEN, [n_used], 1) >= 3, where
                for k in mask:
                    e, ess = expect_tap(oracle, bias, name, ss, k, n_used)
                    g = outs[k].cpu().numpy()
                    assert g.shape == (1, n_used >> k, 2) and np.array_equal(g[0], e), where + (k, np.argwhere(g[0] != e)[:4].tolist())
                    assert sizes[k] == ess, where + (k,)


# ------------------------------------------------------------------------------ 2. ragged bank
RAGGED_COUNTS = [0, 63, 64, 2048 * 2 + 1, N1]


@pytest.mark.parametrize("mem", ["device", "host"])
def test_ragged_bank(ctx, oracle, mem):
    S, L, mask, ss = 5, 6, (2, 4, 6), 12
    d = sd.Decimators(ctx, S, sd.HB_EO1)
    od = {(s, k): oracle.decimators(sd.HB_EO1) for s in range(S) for k in mask}
    for call, shift in enumerate((0, 2, 3)):  # (the counts permuted: every stream crosses a call boundary mid-history)
        cnt = RAGGED_COUNTS[shift:] + RAGGED_COUNTS[:shift]
        x = np.stack([signals.noise(N1 + 3, 100 + 10 * call + s, ss) for s in range(S)])  # (rows a multiple of 4 samples apart)
        outs, sizes, nu = d.decimate_taps(mask, ss, to_mem(x, mem), counts=cnt)
        plan = d.last_plan()
        assert list(nu) == [used(n, L) for n in cnt], (call, list(nu))
        assert plan["path"] == "valu" and plan["nseg"] == B.plan_decimate_ragged(L, CEN, list(nu), S), (call, plan)
        for k in mask:
            g = host(outs[k])
            assert g.shape == (S, max(nu) >> k, 2), (call, k, g.shape)
            for s in range(S):
                n = int(nu[s])
                if n:  # (a stream below 2^L produces nothing and keeps its histories: its reference objects see no call)
                    e, ess = od[s, k].decimate(k, CEN, ss, x[s, :n])
                    assert sizes[k] == ess, (call, s, k)
                else:
                    e = np.zeros((0, 2), np.int16)
                assert np.array_equal(g[s, :n >> k], e), (mem, call, s, k, np.argwhere(g[s, :n >> k] != e)[:4].tolist())
                assert not g[s, n >> k:].any(), (mem, call, s, k, "written past the stream's count")


# ------------------------------------------------------------------------------ 3. chunking
def test_chunking(ctx, oracle):
    L, mask, chunks = 4, (1, 4), [16, 0, 17, 31, 64, 1, 4096, 3]
    x = signals.noise(sum(chunks), 3)
    d = sd.Decimators(ctx, 1, sd.HB_EO1)
    got, consumed, pos = {k: [] for k in mask}, [], 0
    for n in chunks:
        seg = x[pos:pos + n]
        pos += n
        outs, _, nu = d.decimate_taps(mask, 16, seg)
        assert list(nu) == [used(n, L)], n
        assert d.last_plan()["path"] == ("valu" if used(n, L) else None), (n, d.last_plan())
        consumed.append(seg[:used(n, L)])
        for k in mask:
            assert outs[k].shape == (1, used(n, L) >> k, 2), (n, k)
            got[k].append(outs[k][0])
    for k in mask:
        e, _ = oracle.decimators(sd.HB_EO1).decimate(k, CEN, 16, np.concatenate(consumed))
        assert np.array_equal(np.concatenate(got[k]), e), k


# ------------------------------------------------------------------------------ 4. state
def replay(oracle, bias, history):
    """a reference object that has seen the bank's calls so far; a tap call acts on every history as decimate(L, CEN) does"""
    od = oracle.decimators(bias)
    for L, fc, seg in history:
        od.decimate(L, fc, 16, seg)
    return od


# tap calls between plain calls of every mode (the tap call {6} is the centred-after-inf case on the existing kernels), then every L
# with the first stage's history left as rotate-sums: no packed int16 first stage, the other five K1t kernels
SEQUENCE = [("taps", (2, 4)), ("dec", 6, CEN), ("taps", (1, 2, 3)), ("dec", 4, sd.FC_INF), ("taps", (6,)), ("dec", 2, CEN),
            ("dec", 3, sd.FC_SUP), ("taps", (2, 4, 5)), ("dec", 5, sd.FC_INF), ("short", (1, 3)), ("taps", (2, 6)),
            ("dec", 3, sd.FC_INF), ("taps", (1, 2, 3, 4)), ("dec", 4, sd.FC_SUP), ("taps", (1, 3)), ("dec", 3, sd.FC_INF), ("taps", (1, 2))]


@pytest.mark.parametrize("bias", [sd.HB_EO1, sd.HB_DB], ids=["eo1", "db"])
def test_state_across_entries(ctx, oracle, bias):
    x = signals.noise(len(SEQUENCE) * 8192, 99)
    d, history = sd.Decimators(ctx, 1, bias), []
    for i, step in enumerate(SEQUENCE):
        seg = x[i * 8192:(i + 1) * 8192]
        if step[0] == "short":  # (fewer samples than the first history holds: it keeps older rotate-sums)
            seg = seg[:40]
        if step[0] == "dec":
            _, L, fc = step
            a, _ = d.decimate(L, fc, 16, seg)
            b, _ = replay(oracle, bias, history).decimate(L, fc, 16, seg)
            assert np.array_equal(a, b), (bias, i, step)
        else:
            mask = step[1]
            L, fc = max(mask), CEN
            outs, sizes, nu = d.decimate_taps(mask, 16, seg)
            seg = seg[:int(nu[0])]
            for k in mask:
                e, ess = replay(oracle, bias, history).decimate(k, CEN, 16, seg)
                assert np.array_equal(outs[k][0], e) and sizes[k] == ess, (bias, i, step, k)
        history.append((L, fc, seg))


# ------------------------------------------------------------------------------ 5. bounds
BOUNDS_COUNTS = [N1, 4096 + 31, 3 * 2048 + 33]  # (remainders 13, 31 and 1 of 32; rows that end in full and in partial stores)
BOUNDS_MASK = (1, 3, 5)


def taps_struct(mask, bufs):
    t = _lib.DecimTaps()
    for k in mask:
        t.iq_out[k], t.out_stride[k] = bufs[k].ptr, bufs[k].stride
    return t


def bounds_run(ctx, mem, fill):
    S, L, cnt = 3, 5, BOUNDS_COUNTS
    xin0, _ = B.input_arena(S, cnt, fill)
    xin = Buf(xin0, mem)
    out = {k: Buf(B.arena(S, used(max(cnt), L) >> k, B.stride_for(used(max(cnt), L) >> k), B.GUARD, B.SENTINEL)[0], mem) for k in BOUNDS_MASK}
    bank = sd.Decimators(ctx, S, sd.HB_EO1)
    t, n_in, nu = taps_struct(BOUNDS_MASK, out), (C.c_size_t * S)(*cnt), (C.c_size_t * S)(*[77] * S)
    rc = ctx.lib.sdrhip_decimate_taps(bank.h, sum(1 << k for k in BOUNDS_MASK), 16, xin.ptr, n_in, xin.stride, C.byref(t), nu, xin.mem)
    assert rc == 0, (rc, ctx.lib.sdrhip_last_error())
    ctx.synchronize()
    plan = bank.last_plan()
    y2, _ = bank.decimate(L, CEN, 16, to_mem(second_input(S), mem))
    ctx.synchronize()
    return {"out": {k: out[k].read() for k in BOUNDS_MASK}, "xin": xin.read(), "xin0": xin0, "n_used": list(nu), "plan": plan, "y2": host(y2),
            "sizes": {k: t.sample_size[k] for k in BOUNDS_MASK}}


@pytest.mark.parametrize("mem", ["device", "host"])
def test_bounds(ctx, oracle, mem):
    S, L, cnt = 3, 5, BOUNDS_COUNTS

    def make():
        exp, exp2, x2 = {}, [], second_input(S)
        for s in range(S):
            x = B.stream_samples(s, cnt[s])[:used(cnt[s], L)]
            for k in BOUNDS_MASK:
                exp[s, k] = oracle.decimators(sd.HB_EO1).decimate(k, CEN, 16, x)
            od = oracle.decimators(sd.HB_EO1)
            od.decimate(L, CEN, 16, x)
            exp2.append(od.decimate(L, CEN, 16, x2[s])[0])
        return exp, exp2
    exp, exp2 = once(("taps-bounds",), make)
    res = [bounds_run(ctx, mem, fill) for fill in B.FILLS]
    for fill, r in zip(B.FILLS, res):
        where = ("taps", mem, fill)
        assert r["n_used"] == [used(n, L) for n in cnt], where
        assert r["plan"]["path"] == "valu" and r["plan"]["nseg"] == B.plan_decimate_ragged(L, CEN, r["n_used"], S), (where, r["plan"])
        for k in BOUNDS_MASK:
            check_output(r["out"][k], [n >> k for n in r["n_used"]], [exp[s, k][0] for s in range(S)], where + (k,))
            assert r["sizes"][k] == exp[0, k][1], where + (k,)
        assert np.array_equal(r["xin"], r["xin0"]), (where, "the input was written")
        for s in range(S):
            assert np.array_equal(r["y2"][s], exp2[s]), (where, "the following call", s)
    for k in BOUNDS_MASK:
        assert np.array_equal(res[0]["out"][k], res[1]["out"][k]), (mem, k, "the result depends on what lies behind the rows")


# ------------------------------------------------------------------------------ 6. refusals
def test_refusals_consume_nothing(ctx, oracle):
    S, L, mask, n = 2, 4, (2, 4), 8192
    bits = sum(1 << k for k in mask)
    x = np.stack([signals.noise(3 * n, 50 + s) for s in range(S)])
    d = sd.Decimators(ctx, S, sd.HB_EO1)
    od = {(s, k): oracle.decimators(sd.HB_EO1) for s in range(S) for k in mask}
    lib = ctx.lib

    def valid(piece):
        seg = np.ascontiguousarray(x[:, piece * n:(piece + 1) * n])
        outs, _, nu = d.decimate_taps(mask, 16, torch.from_numpy(seg).cuda())
        assert list(nu) == [n] * S and d.last_plan()["path"] == "valu"
        for s in range(S):
            for k in mask:
                assert np.array_equal(outs[k][s].cpu().numpy(), od[s, k].decimate(k, CEN, 16, seg[s])[0]), (piece, s, k)

    valid(0)
    xin = torch.from_numpy(np.ascontiguousarray(x[:, n:2 * n])).cuda()
    out = {k: torch.full((S, (n >> k) + 8, 2), 0x5a5a, dtype=torch.int16, device="cuda") for k in mask}

    def call(handle=None, m=bits, ss=16, inp=None, n_in=(n, n), in_stride=n, taps=True, n_used=True, mem=sd.MEM_DEVICE, out_ptr=None,
             out_stride=None):
        t = _lib.DecimTaps()
        for k in mask:
            t.iq_out[k] = (out_ptr or {}).get(k, out[k].data_ptr())
            t.out_stride[k] = (out_stride or {}).get(k, (n >> k) + 8)
        nu = (C.c_size_t * S)(*[77] * S)
        rc = lib.sdrhip_decimate_taps(d.h if handle is None else handle, m, ss, xin.data_ptr() if inp is None else inp,
                                      (C.c_size_t * S)(*n_in) if n_in is not None else None, in_stride, C.byref(t) if taps else None,
                                      nu if n_used else None, mem)
        assert list(nu) == [77] * S, "a refused call wrote n_used"
        return rc

    huge = 1 << 50  # (2^34 segments of the longest kind: more than a grid holds; refused by the planner, no byte is touched)
    einval = {
        "NULL handle": dict(handle=C.c_void_p(0)), "NULL taps": dict(taps=False), "NULL n_in": dict(n_in=None), "NULL n_used": dict(n_used=False),
        "empty mask": dict(m=0), "bit 0": dict(m=bits | 1), "bit 7": dict(m=bits | 0x80), "bit 31": dict(m=bits | (1 << 31)),
        "sampleSize 0": dict(ss=0), "sampleSize 17": dict(ss=17), "mem": dict(mem=7),
        "NULL tapped buffer": dict(out_ptr={2: 0}), "NULL input": dict(inp=0),
        "in_stride below the count": dict(in_stride=n - 4), "out_stride below the count": dict(out_stride={4: (n >> 4) - 4}),
        "too many segments": dict(n_in=(huge, huge), in_stride=huge, out_stride={k: huge >> k for k in mask}),
    }
    ealign = {
        "input pointer": dict(inp=xin.data_ptr() + 4), "output pointer": dict(out_ptr={4: out[4].data_ptr() + 8}),
        "in_stride": dict(in_stride=n + 2), "out_stride": dict(out_stride={2: (n >> 2) + 6}),
    }
    for name, kw in einval.items():
        assert call(**kw) == EINVAL, (name, lib.sdrhip_last_error())
    for name, kw in ealign.items():
        assert call(**kw) == EALIGN, (name, lib.sdrhip_last_error())
    ctx.synchronize()
    for k in mask:
        assert bool((out[k] == 0x5a5a).all()), (k, "a refused call wrote output")
    # nothing was consumed, enqueued or changed: the bank goes on from piece 0, and the plan on record is still that call's
    assert d.last_plan()["path"] == "valu"
    valid(1)
    valid(2)


# ------------------------------------------------------------------------------ 7. link bytes
@pytest.mark.parametrize("counts", [[4096 + 7, 0, 20000 + 77], [40000, 40000, 40000], [40000 + 5, 63, 33000 + 1]],
                         ids=["pinned-rows", "equal-rectangles", "unequal-rows"])
def test_host_call_moves_exactly_the_counts(ctx, oracle, counts):
    S, L, mask = 3, 6, (2, 4, 6)
    x = np.stack([signals.noise(max(counts), 70 + s) for s in range(S)])
    d = sd.Decimators(ctx, S, sd.HB_EO1)
    up0, down0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
    outs, _, nu = d.decimate_taps(mask, 16, x, counts=counts)
    up, down = ctx.counter("h2d_bytes") - up0, ctx.counter("d2h_bytes") - down0
    assert list(nu) == [used(n, L) for n in counts]
    assert up == 4 * sum(counts), (up, 4 * sum(counts))
    assert down == 4 * sum(int(u) >> k for k in mask for u in nu), (down, list(nu))
    for s in range(S):
        for k in mask:
            e = oracle.decimators(sd.HB_EO1).decimate(k, CEN, 16, x[s, :int(nu[s])])[0] if nu[s] else np.zeros((0, 2), np.int16)
            assert np.array_equal(outs[k][s, :int(nu[s]) >> k], e), (s, k)
            assert not outs[k][s, int(nu[s]) >> k:].any(), (s, k)


# ------------------------------------------------------------------------------ 8. fan-out composition
def test_fan_out_hub(ctx, oracle):
    """INTEGRATION.md "fan-out hub": the taps' rows are rows j * nstreams + s of one device arena, which ONE Rx bank of T * nstreams
    streams at log2decim = 0 frames and protects, each row at its own rate"""
    S, mask, rate = 2, (2, 4), 2400000
    L, T = max(mask), len(mask)
    counts = [17 * 16129 + 5, 16 * 16129 + 16 * 40]
    x = np.stack([signals.noise((max(counts) + 3) & ~3, 80 + s) for s in range(S)])  # (rows a multiple of 4 samples apart)
    nu = [used(n, L) for n in counts]
    stride = B.stride_for(max(nu) >> min(mask))
    arena = torch.full((T * S, stride, 2), 0x5a5a, dtype=torch.int16, device="cuda")
    d = sd.Decimators(ctx, S, sd.HB_EO1)
    outs, sizes, got_nu = d.decimate_taps(mask, 16, torch.from_numpy(x).cuda(), counts=counts,
                                          out={k: arena[j * S:(j + 1) * S, :max(nu) >> k] for j, k in enumerate(mask)})
    assert list(got_nu) == nu and all(sizes[k] == 16 for k in mask), (got_nu, sizes)
    row_counts = [nu[s] >> k for k in mask for s in range(S)]
    rates = [rate >> k for k in mask for s in range(S)]

    def pipe():
        rx = sd.RxPipe(ctx, T * S, log2decim=0, fcpos=CEN, sample_bits=16, nb_fec=8, sample_rate=rate)
        rx.set_stream_meta(sample_rate=rates)
        return rx
    frames, nf = pipe().process_ragged(arena, row_counts, tv_sec=1000, tv_usec=250)
    ctx.synchronize()
    ref = np.zeros((T * S, max(row_counts), 2), np.int16)
    for j, k in enumerate(mask):
        for s in range(S):
            e = oracle.decimators(sd.HB_EO1).decimate(k, CEN, 16, x[s, :nu[s]])[0]
            ref[j * S + s, :len(e)] = e
    exp, enf = pipe().process_ragged(ref, row_counts, tv_sec=1000, tv_usec=250)
    assert list(nf) == list(enf) == [c // 16129 for c in row_counts] and min(nf) >= 1, (list(nf), list(enf))
    frames = frames.cpu().numpy()
    for r in range(T * S):
        assert np.array_equal(frames[r, :nf[r]], np.asarray(exp)[r, :nf[r]]), r
