"""The DSP banks touch nothing outside a call's rows: sdrhip_decimate (K1, K1m and the filter-less kernel), sdrhip_decimate_ragged and
sdrhip_decimate_ragged_bits (K1r, K1mr), the uniform sdrhip_interpolate (the copy, K5, K5w in workgroups of one and of four waves) and
sdrhip_testsource_read, in device and in host memory, over the shapes of bank_bounds_cases.py -- every store form at a row's end, every
dropped remainder, every piece edge.  Every buffer is a view into an arena (guard rows in front and behind, a gap behind every row), the
entries are called through ctypes with the arena's pointers and strides.  Per case, all of it byte-exact:
 1. rows [0, n_out[s]) are the oracle's (decimators(bias) / interpolators(), pinned to the compiled reference; testsource_generate);
 2. every other sample of the output arena still holds the sentinel: gaps, guard rows, rows of streams without a result;
 3. a second, fresh bank given the same samples with the OTHER fill behind them (noise / rails: gaps, guard rows, whatever follows
    n_in[s]) returns the same bytes, and a following call of 4096 fresh samples per stream on either bank is the oracle's next call:
    neither the result nor the state left behind took anything from behind a row;
 4. the input arena is as it was;
 5. the launch was the one the case names (sdrhip_decimators_last_plan / sdrhip_interpolators_last_plan): no fall-back to another path.
A wrong bound shows as a failed assertion here, in memory the test owns."""
import ctypes as C

import numpy as np
import pytest
import torch

import bank_bounds_cases as B
import sdrdaemon_amd as sd

pytestmark = pytest.mark.gpu

MEMS = ["device", "host"]


@pytest.fixture(scope="module")
def ctx():
    assert sd.device_count() > 0, "GPU tests need a GPU and libsdrhip.so"
    c = sd.Context(0)
    yield c
    restore(c, B.DECIM_DEFAULTS)
    restore(c, B.INTERP_DEFAULTS)


def restore(ctx, defaults):
    for k, v in defaults.items():
        ctx.set_option(k, v)


_cache = {}


def once(key, make):
    """a reference computed once per module and shared (never written to)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class Buf:
    """an arena in the memory a call takes; ptr / stride: its rows 1..S as the library is given them"""

    def __init__(self, arena, mem):
        self.stride = arena.shape[1]
        if mem == "device":
            self.mem, self.t = sd.MEM_DEVICE, torch.from_numpy(arena).cuda()
            base = self.t.data_ptr()
        else:
            self.mem, self.a = sd.MEM_HOST, arena.copy()
            base = self.a.ctypes.data
        self.ptr = base + self.stride * 4

    def read(self):
        return self.t.cpu().numpy() if self.mem == sd.MEM_DEVICE else self.a


def to_mem(x, mem):
    return torch.from_numpy(x).cuda() if mem == "device" else x


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def second_input(S, signal_of=None):
    return np.stack([B.stream_samples(signal_of(s) if signal_of else s, B.SECOND, second=True) for s in range(S)])


def check_output(out, n_out, exp, where):
    """checks 1 and 2 on an output arena"""
    out = out.copy()
    for s, n in enumerate(n_out):
        assert np.array_equal(out[1 + s, :n], exp[s]), (where, "stream", s, np.argwhere(out[1 + s, :n] != exp[s])[:4])
        out[1 + s, :n] = B.SENTINEL
    bad = np.argwhere(out != B.SENTINEL)
    assert not len(bad), (where, "written outside the results: (row, sample, component)", bad[:8].tolist(), "n_out", list(n_out))


def check_pair(res, exp2, where):
    """checks 3 and 4 on the two banks' runs"""
    for fill, r in zip(B.FILLS, res):
        assert np.array_equal(r["xin"], r["xin0"]), (where, fill, "the input was written")
        for s, e in enumerate(exp2):
            assert np.array_equal(r["y2"][s], e), (where, fill, "the following call", s)
    assert np.array_equal(res[0]["out"], res[1]["out"]), (where, "the result depends on what lies behind the rows")


# ------------------------------------------------------------------------------ decimator bank
def decim_counts(c):
    return c["counts"] if "counts" in c else [c["n_in"]] * c["S"]


def decim_expected(oracle, c, entry):
    """-> (exp[s], size after the call [s] or None, exp2[s]): one-stream oracle objects given each stream's samples, then SECOND more"""
    def make():
        L, fc, cnt = c["L"], c["fcpos"], decim_counts(c)
        bits = B.ragged_bits(L) if entry == "ragged_bits" else [16] * c["S"]
        exp, sizes, exp2 = [], [], []
        x2 = second_input(c["S"])
        for s in range(c["S"]):
            od = oracle.decimators(c["bias"])
            if (cnt[s] if L == 0 else cnt[s] >> L):
                y, ss = od.decimate(L, fc, bits[s], B.stream_samples(s, cnt[s], bits[s]))
            else:  # (no whole output sample: nothing enters any history)
                y, ss = np.zeros((0, 2), np.int16), None
            exp.append(y)
            sizes.append(ss)
            exp2.append(od.decimate(L, fc, 16, x2[s])[0])
        return exp, sizes, exp2
    return once(("decim", c["id"], entry == "ragged_bits"), make)


def decim_run(ctx, c, entry, mem, fill):
    S, L, fc, cnt = c["S"], c["L"], c["fcpos"], decim_counts(c)
    bits = B.ragged_bits(L) if entry == "ragged_bits" else None
    xin0, _ = B.input_arena(S, cnt, fill, bits)
    n_res = max(cnt) >> L
    out0, _ = B.arena(S, n_res, B.stride_for(n_res), B.GUARD, B.SENTINEL)
    xin, out = Buf(xin0, mem), Buf(out0, mem)
    bank, lib = sd.Decimators(ctx, S, c["bias"]), ctx.lib
    if entry == "uniform":
        ss, n_out = C.c_uint(16), C.c_size_t(0)
        rc = lib.sdrhip_decimate(bank.h, L, fc, C.byref(ss), xin.ptr, c["n_in"], xin.stride, out.ptr, out.stride, C.byref(n_out), xin.mem)
        n_out, sizes = [n_out.value] * S, [ss.value] * S
    else:
        n_in, n_out = (C.c_size_t * S)(*cnt), (C.c_size_t * S)(*[77] * S)
        if entry == "ragged":
            ss = C.c_uint(16)
            rc = lib.sdrhip_decimate_ragged(bank.h, L, fc, C.byref(ss), xin.ptr, n_in, xin.stride, out.ptr, out.stride, n_out, xin.mem)
            sizes = [ss.value] * S
        else:
            ss = (C.c_uint * S)(*bits)
            rc = lib.sdrhip_decimate_ragged_bits(bank.h, L, fc, ss, xin.ptr, n_in, xin.stride, out.ptr, out.stride, n_out, xin.mem)
            sizes = list(ss)
        n_out = list(n_out)
    assert rc == 0, (rc, lib.sdrhip_last_error())
    ctx.synchronize()
    plan = bank.last_plan()
    y2, _ = bank.decimate(L, fc, 16, to_mem(second_input(S), mem))
    ctx.synchronize()
    return {"out": out.read(), "xin": xin.read(), "xin0": xin0, "n_out": n_out, "sizes": sizes, "plan": plan, "y2": host(y2)}


def decim_case(ctx, oracle, c, entry, mem):
    where = (c["id"], entry, mem)
    exp, sizes, exp2 = decim_expected(oracle, c, entry)
    try:
        restore(ctx, c["opts"])
        res = [decim_run(ctx, c, entry, mem, fill) for fill in B.FILLS]
    finally:
        restore(ctx, B.DECIM_DEFAULTS)
    for fill, r in zip(B.FILLS, res):
        print(where, fill, "last_plan", r["plan"])
        assert r["n_out"] == [n >> c["L"] for n in decim_counts(c)], (where, fill)
        assert all(e is None or e == g for e, g in zip(sizes, r["sizes"])), (where, fill, sizes, r["sizes"])
        check_output(r["out"], r["n_out"], exp, where + (fill,))
        for k, v in c["expect"].items():
            assert r["plan"][k] == v, (where, fill, k, r["plan"], c["expect"])
        if c["expect"]["path"] == "mfma":
            assert r["plan"]["wps"] >= 1, (where, r["plan"])
    check_pair(res, exp2, where)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("case", B.DECIM_UNIFORM, ids=[c["id"] for c in B.DECIM_UNIFORM])
def test_decimate(ctx, oracle, case, mem):
    decim_case(ctx, oracle, case, "uniform", mem)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("entry", ["ragged", "ragged_bits"])
@pytest.mark.parametrize("case", B.DECIM_RAGGED, ids=[c["id"] for c in B.DECIM_RAGGED])
def test_decimate_ragged(ctx, oracle, case, entry, mem):
    decim_case(ctx, oracle, case, entry, mem)


# ------------------------------------------------------------------------------ interpolator bank, the uniform entry
def interp_expected(oracle, L, n, signal):
    def make():
        oi = oracle.interpolators()
        return oi.interpolate(L, B.stream_samples(signal, n)), oi.interpolate(L, B.stream_samples(signal, B.SECOND, second=True))
    return once(("interp", L, n, signal), make)


def interp_run(ctx, c, mem, fill):
    S, L, n = c["S"], c["L"], c["n_in"]
    xin0, _ = B.input_arena(S, [n] * S, fill, signal_of=c["signal_of"])
    out0, _ = B.arena(S, n << L, B.stride_for(n << L), B.GUARD, B.SENTINEL)
    xin, out = Buf(xin0, mem), Buf(out0, mem)
    bank, n_out = sd.Interpolators(ctx, S), C.c_size_t(0)
    rc = ctx.lib.sdrhip_interpolate(bank.h, L, xin.ptr, n, xin.stride, out.ptr, out.stride, C.byref(n_out), xin.mem)
    assert rc == 0, (rc, ctx.lib.sdrhip_last_error())
    ctx.synchronize()
    plan = bank.last_plan()
    y2 = bank.interpolate(L, to_mem(second_input(S, c["signal_of"]), mem))
    ctx.synchronize()
    return {"out": out.read(), "xin": xin.read(), "xin0": xin0, "n_out": [n_out.value] * S, "plan": plan, "y2": host(y2)}


INTERP_CASES = B.INTERP_UNIFORM + [B.INTERP_FOUR]


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("case", INTERP_CASES, ids=[c["id"] for c in INTERP_CASES])
def test_interpolate(ctx, oracle, case, mem):
    c, where = case, (case["id"], mem)
    both = [interp_expected(oracle, c["L"], c["n_in"], c["signal_of"](s)) for s in range(c["S"])]
    exp, exp2 = [b[0] for b in both], [b[1] for b in both]
    try:
        restore(ctx, c["opts"])
        res = [interp_run(ctx, c, mem, fill) for fill in B.FILLS]
    finally:
        restore(ctx, B.INTERP_DEFAULTS)
    for fill, r in zip(B.FILLS, res):
        print(where, fill, "last_plan", r["plan"])
        assert r["n_out"] == [c["n_in"] << c["L"]] * c["S"], (where, fill)
        check_output(r["out"], r["n_out"], exp, where + (fill,))
        assert r["plan"] == c["expect"], (where, fill, r["plan"], c["expect"])
    check_pair(res, exp2, where)


# ------------------------------------------------------------------------------ TestSource bank
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("n", B.TS_N)
def test_testsource_read(ctx, oracle, n, mem):
    """three streams of three configurations: n samples each and nothing else, then the phase-continuous next 4096"""
    ts = sd.TestSource(ctx, B.TS_S)
    for s, kv in enumerate(B.TS_CONFIGS):
        assert ts.configure(kv, s), ts.error()
    par = [(oracle.lib.orc_nco_phase_inc(off, rate), oracle.lib.orc_nco_amp_q15(power)) for off, rate, power in B.TS_PARAMS]
    first = [oracle.testsource_generate(0, inc, amp, n) for inc, amp in par]
    out0, _ = B.arena(B.TS_S, n, B.stride_for(n), B.GUARD, B.SENTINEL)
    out = Buf(out0, mem)
    rc = ctx.lib.sdrhip_testsource_read(ts.h, out.ptr, n, out.stride, out.mem)
    assert rc == 0, (rc, ctx.lib.sdrhip_last_error())
    ctx.synchronize()
    check_output(out.read(), [n] * B.TS_S, [e for e, _ in first], (n, mem))
    y2 = ts.read(B.SECOND, host=mem == "host")
    ctx.synchronize()
    for s, (inc, amp) in enumerate(par):
        assert np.array_equal(host(y2)[s], oracle.testsource_generate(first[s][1], inc, amp, B.SECOND)[0]), (n, mem, s)
