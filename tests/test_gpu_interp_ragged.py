"""The sample-fed ragged interpolator entry (sdrhip_interpolate_ragged, K5c) on the GPU: per stream, the output and the state a call
leaves are those of a one-stream bank given the same chunks in the same order -- here the oracle's interpolators, which are pinned to
the compiled reference --, whatever the other streams of the call got: any count (0, 1, odd), every ratio, both kernels, device and
host memory, mixed with the uniform call on one bank, at every segment edge; nothing outside n_out[s] samples of a row is written;
the grid is the sum of the streams' segments (sdrhip_interpolators_last_plan), in workgroups of four waves from 4096 entries on; and a
refused call leaves the bank as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

import sdrdaemon_amd as sd
import signals

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a
PARITY = [[4001, 0, 1, 127, 2048], [0, 3, 129, 2049, 255], [513, 1025, 0, 0, 16129]]


@pytest.fixture(scope="module")
def ctx():
    assert sd.device_count() > 0, "GPU tests need a GPU and libsdrhip.so"
    c = sd.Context(0)
    yield c
    c.set_option("interp_path", "auto")
    c.set_option("interp_span", 0)


def route(ctx, path, span=0):
    ctx.set_option("interp_path", path)
    ctx.set_option("interp_span", span)


_cache = {}


def once(key, make):
    """a reference computed once per module and shared (never written to)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def stream_samples(s, n):
    """the first n samples of stream s's input: every stream its own signal"""
    x = once(("in", s), lambda: signals.mixed(70000, 100 + s))
    assert n <= x.shape[0]
    return x[:n]


def expected(oracle, L, calls, tag):
    """calls: a list of per-stream counts.  -> exp[call][stream] = what a one-stream reference object, given the stream's chunks of
    all calls in order, returns for this one (a stream's chunks are consecutive pieces of its signal)"""
    def make():
        S = len(calls[0])
        banks, pos, out = [oracle.interpolators() for _ in range(S)], [0] * S, []
        for cnt in calls:
            row = []
            for s in range(S):
                n = int(cnt[s])
                x = stream_samples(s, pos[s] + n)[pos[s]:]
                row.append(banks[s].interpolate(L, x) if n else np.zeros((0, 2), np.int16))
                pos[s] += n
            out.append(row)
        return out
    return once(("exp", L, tag), make)


def rows_for(calls, k, pad=0, seed=0):
    """the input of call k: (S, max + pad, 2) int16, row s = the stream's next counts[s] samples, whatever lies behind them noise"""
    S = len(calls[0])
    pos = [sum(int(c[s]) for c in calls[:k]) for s in range(S)]
    mx = max(int(c) for c in calls[k])
    x = np.random.RandomState(1000 + seed + k).randint(-32768, 32768, size=(S, mx + pad, 2)).astype(np.int16)
    for s in range(S):
        n = int(calls[k][s])
        x[s, :n] = stream_samples(s, pos[s] + n)[pos[s]:]
    return x


def device_rows(x):
    """(S, n, 2) numpy -> a CUDA tensor of rows a multiple of 4 samples apart"""
    S, n = x.shape[0], x.shape[1]
    buf = torch.zeros((S, max((n + 3) & ~3, 4), 2), dtype=torch.int16, device="cuda")
    buf[:, :n].copy_(torch.from_numpy(x))
    return buf[:, :n]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run_calls(ctx, bank, L, calls, exp, mem, where):
    for k, cnt in enumerate(calls):
        x = rows_for(calls, k)
        out, n_out = bank.interpolate_ragged(L, device_rows(x) if mem == "device" else x, cnt)
        ctx.synchronize()
        out = host(out)
        assert list(n_out) == [int(c) << L for c in cnt], (where, k)
        assert out.shape == (len(cnt), max(cnt) << L, 2), (where, k, out.shape)
        for s in range(len(cnt)):
            assert np.array_equal(out[s, :n_out[s]], exp[k][s]), (where, "call", k, "stream", s, "count", cnt[s])


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("path", ["wave", "valu"])
@pytest.mark.parametrize("L", range(7))
def test_parity_with_one_stream_twins(ctx, oracle, L, path, mem):
    """three consecutive calls with the counts moving between the streams: every stream's outputs are its twin's, so the state carries
    over, across a call in which the stream got nothing too"""
    route(ctx, path)
    bank = sd.Interpolators(ctx, 5)
    run_calls(ctx, bank, L, PARITY, expected(oracle, L, PARITY, "parity"), mem, (L, path, mem))
    plan = bank.last_plan()
    assert plan["compact"] and plan["path"] == ("copy" if L == 0 else "wave" if path == "wave" and L >= 2 else "valu")
    assert plan["entries"] == sum(max(1, -(-n // plan["seg_len"])) for n in PARITY[-1])


WAVE_EDGES = [127, 128, 129, 255, 256, 257, 383]
VALU_EDGES = [511, 512, 513, 1023, 1024, 1025, 1537]


@pytest.mark.parametrize("span", [128, 256])
@pytest.mark.parametrize("L", [2, 4, 6])
def test_wave_segment_edges(ctx, oracle, L, span):
    """K5w with segments of one block and of a pair: a stream that ends one sample short of a block, on it, one past it, and with an odd
    block left; twice, so that every stream starts its second call from the state its edge left"""
    route(ctx, "wave", span)
    calls = [WAVE_EDGES, WAVE_EDGES[::-1]]
    bank = sd.Interpolators(ctx, len(WAVE_EDGES))
    run_calls(ctx, bank, L, calls, expected(oracle, L, calls, "wave-edges"), "device", (L, span))
    plan = bank.last_plan()
    assert plan == {"path": "wave", "seg_len": span, "wpw": 1, "entries": sum(-(-n // span) for n in WAVE_EDGES), "compact": True}


@pytest.mark.parametrize("L", [1, 2, 5])
def test_valu_macro_cycle_edges(ctx, oracle, L):
    """K5 around its macro-cycles of 512 inputs (1024 at x2); small calls plan one macro-cycle per segment"""
    route(ctx, "valu")
    calls = [VALU_EDGES, VALU_EDGES[::-1]]
    bank = sd.Interpolators(ctx, len(VALU_EDGES))
    run_calls(ctx, bank, L, calls, expected(oracle, L, calls, "valu-edges"), "device", L)
    plan = bank.last_plan()
    mc = 1024 if L == 1 else 512
    assert plan == {"path": "valu", "seg_len": mc, "wpw": 1, "entries": sum(-(-n // mc) for n in VALU_EDGES), "compact": True}


@pytest.mark.parametrize("path", ["wave", "valu"])
@pytest.mark.parametrize("L", [0, 1, 4])
def test_mixes_with_the_uniform_call(ctx, oracle, L, path):
    """ragged, uniform, ragged on one bank against twins given the same chunks; and equal counts through the ragged entry are the
    uniform call byte for byte, output and following state"""
    route(ctx, path)
    calls = [[700, 0, 2049], [1300, 1300, 1300], [5, 4097, 0]]
    exp = expected(oracle, L, calls, "mix")
    bank = sd.Interpolators(ctx, 3)
    for k, cnt in enumerate(calls):
        x = device_rows(rows_for(calls, k))
        if k == 1:
            out = host(bank.interpolate(L, x))
            assert not bank.last_plan()["compact"]
        else:
            out = host(bank.interpolate_ragged(L, x, cnt)[0])
            assert bank.last_plan()["compact"]
        for s in range(3):
            assert np.array_equal(out[s, :cnt[s] << L], exp[k][s]), (L, path, k, s)
    # equal counts: the two entries on two banks, then one more uniform call on each
    equal = [[3000, 3000, 3000], [1111, 1111, 1111]]
    a, b = sd.Interpolators(ctx, 3), sd.Interpolators(ctx, 3)
    x = device_rows(rows_for(equal, 0))
    ya, n_out = a.interpolate_ragged(L, x, equal[0])
    yb = b.interpolate(L, x)
    pa, pb = a.last_plan(), b.last_plan()
    assert list(n_out) == [3000 << L] * 3 and torch.equal(ya, yb)
    if L:  # (the same segments; the uniform x1 is a strided copy without any)
        assert (pa["path"], pa["seg_len"], pa["wpw"], pa["entries"]) == (pb["path"], pb["seg_len"], pb["wpw"], pb["entries"])
    x = device_rows(rows_for(equal, 1))
    assert torch.equal(a.interpolate(L, x), b.interpolate(L, x))
    ctx.synchronize()


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("path", ["wave", "valu"])
@pytest.mark.parametrize("L", [0, 1, 3, 6])
def test_nothing_outside_the_streams_results_is_written(ctx, oracle, L, path, mem):
    """the output is a slice of a larger allocation prefilled with a sentinel: past n_out[s] samples of a row, between the rows, in
    front of the first and behind the last nothing changes; the input rows are slices too, with noise behind every stream's samples"""
    route(ctx, path)
    calls = [[130, 0, 1, 2049, 999]]
    exp = expected(oracle, L, calls, "bounds")
    cnt, S = calls[0], 5
    mx = max(cnt)
    x = rows_for(calls, 0, pad=27)  # (rows of 2076 samples: a multiple of 4)
    stride_out = ((mx << L) + 64 + 3) & ~3
    if mem == "device":
        xin = torch.from_numpy(x).cuda()[:, :mx]
        big = torch.full((S + 2, stride_out, 2), SENTINEL, dtype=torch.int16, device="cuda")
    else:
        xin = x[:, :mx]
        big = np.full((S + 2, stride_out, 2), SENTINEL, np.int16)
    out = big[1:S + 1, :mx << L]
    got, n_out = sd.Interpolators(ctx, S).interpolate_ragged(L, xin, cnt, out=out)
    ctx.synchronize()
    big = host(big)
    for s in range(S):
        assert np.array_equal(big[1 + s, :n_out[s]], exp[0][s]), (L, path, mem, s)
        assert (big[1 + s, n_out[s]:] == SENTINEL).all(), (L, path, mem, s, "written past n_out")
    assert (big[0] == SENTINEL).all() and (big[S + 1] == SENTINEL).all()


def test_the_grid_follows_the_samples(ctx, oracle):
    """counts [2048 * 16, 1, 0, 129] at the default span: 16 + 1 + 1 + 1 entries, not 4 x 16"""
    route(ctx, "wave")
    calls = [[2048 * 16, 1, 0, 129]]
    bank = sd.Interpolators(ctx, 4)
    run_calls(ctx, bank, 4, calls, expected(oracle, 4, calls, "grid"), "device", "grid")
    assert bank.last_plan() == {"path": "wave", "seg_len": 2048, "wpw": 1, "entries": 16 + 1 + 1 + 1, "compact": True}
    # the uniform call on the longest stream's count: the rectangle
    bank.interpolate(4, device_rows(rows_for([[2048 * 16] * 4], 0)))
    ctx.synchronize()
    assert bank.last_plan() == {"path": "wave", "seg_len": 2048, "wpw": 1, "entries": 4 * 16, "compact": False}


# 17 streams in one-block segments: one without input, the others 246 .. 336 blocks with odd ends -- 4650 entries.  (A top count of
# 253 x 128, the shape of test_gpu_interp_variants.py, cannot pass 4096 with a stream of 0 among 17: 16 x 253 + 1 = 4049.)
FOUR = [0] + [(240 + 6 * s) * 128 - 7 * s for s in range(1, 17)]


def test_workgroups_of_four(ctx, oracle):
    """from 4096 entries on K5w runs in workgroups of four waves, whose waves belong to different streams where a stream ends; the
    same streams, three of them only, stay at one wave per workgroup"""
    route(ctx, "wave", 128)
    entries = sum(max(1, -(-n // 128)) for n in FOUR)
    assert entries >= 4096 and any(-(-n // 128) % 4 for n in FOUR)
    exp = expected(oracle, 2, [FOUR], "four")
    bank = sd.Interpolators(ctx, 17)
    run_calls(ctx, bank, 2, [FOUR], exp, "device", "four")
    assert bank.last_plan() == {"path": "wave", "seg_len": 128, "wpw": 4, "entries": entries, "compact": True}
    three = [FOUR[:3]]
    bank = sd.Interpolators(ctx, 3)
    run_calls(ctx, bank, 2, three, [exp[0][:3]], "device", "three")
    assert bank.last_plan() == {"path": "wave", "seg_len": 128, "wpw": 1, "entries": sum(max(1, -(-n // 128)) for n in three[0]), "compact": True}


def test_host_calls_move_exactly_the_samples(ctx, oracle):
    """one packed upload of 4 * sum n_in bytes, one packed download of 4 * sum n_out (x2: every stream's share rounded up to 16 bytes)"""
    route(ctx, "wave")
    calls = [[130, 0, 1, 2049, 999]]
    for L in (0, 1, 4):
        bank = sd.Interpolators(ctx, 5)
        up, down = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        run_calls(ctx, bank, L, calls, expected(oracle, L, calls, "bounds"), "host", ("bytes", L))
        n_out = [n << L for n in calls[0]]
        assert ctx.counter("h2d_bytes") - up == 4 * sum(calls[0])
        assert ctx.counter("d2h_bytes") - down == 4 * sum((n + 3) & ~3 if L == 1 else n for n in n_out), L


def test_all_zero_counts_launch_nothing(ctx, oracle):
    route(ctx, "wave")
    calls = [[100, 300], [0, 0], [77, 1]]
    exp = expected(oracle, 3, calls, "zeros")
    bank = sd.Interpolators(ctx, 2)
    run_calls(ctx, bank, 3, calls[:1], exp[:1], "device", "zeros")
    out, n_out = bank.interpolate_ragged(3, torch.zeros((2, 4, 2), dtype=torch.int16, device="cuda"), [0, 0])
    assert list(n_out) == [0, 0] and bank.last_plan()["path"] is None and bank.last_plan()["entries"] == 0
    x = rows_for(calls, 2)
    out, n_out = bank.interpolate_ragged(3, device_rows(x), calls[2])
    ctx.synchronize()
    for s in range(2):
        assert np.array_equal(host(out)[s, :n_out[s]], exp[2][s]), s


def test_refusals_leave_the_bank_as_it_was(ctx, oracle):
    """every refused call is refused on the host, in front of any launch: the call behind it gives what a bank that never saw the
    refused one gives"""
    route(ctx, "wave")
    L, S = 4, 3
    calls = [[300, 0, 1025], [64, 129, 2]]
    exp = expected(oracle, L, calls, "refusals")
    bank = sd.Interpolators(ctx, S)
    run_calls(ctx, bank, L, calls[:1], exp[:1], "device", "refusals")
    lib, sz = ctx.lib, C.c_size_t
    x = device_rows(rows_for(calls, 1))
    y = torch.full((S, 129 << L, 2), SENTINEL, dtype=torch.int16, device="cuda")
    xin, yout, xs, ys = x.data_ptr(), y.data_ptr(), x.stride(0) // 2, y.stride(0) // 2
    n_in, n_out = (sz * S)(*calls[1]), (sz * S)(7, 7, 7)
    refused = [
        ("NULL n_in", -1, (L, xin, None, xs, yout, ys, n_out, 1)),
        ("NULL n_out", -1, (L, xin, n_in, xs, yout, ys, None, 1)),
        ("NULL input", -1, (L, None, n_in, xs, yout, ys, n_out, 1)),
        ("NULL output", -1, (L, xin, n_in, xs, None, ys, n_out, 1)),
        ("in_stride below the largest count", -1, (L, xin, n_in, 128, yout, ys, n_out, 1)),
        ("out_stride below the largest result", -1, (L, xin, n_in, xs, yout, (129 << L) - 4, n_out, 1)),
        ("a count of 2^31", -1, (L, xin, (sz * S)(64, 1 << 31, 2), 1 << 32, yout, 1 << 40, n_out, 1)),
        ("a ratio of 128", -1, (7, xin, n_in, xs, yout, ys, n_out, 1)),
        ("a negative ratio", -1, (-1, xin, n_in, xs, yout, ys, n_out, 1)),
        ("an unknown memory kind", -1, (L, xin, n_in, xs, yout, ys, n_out, 5)),
    ]
    for what, code, args in refused:
        assert lib.sdrhip_interpolate_ragged(bank.h, *args) == code, what
        assert lib.sdrhip_last_error(), what
    for what, args in [("a misaligned input", (L, xin + 4, n_in, xs, yout, ys, n_out, 1)), ("a misaligned output", (L, xin, n_in, xs, yout + 8, ys, n_out, 1)),
                       ("an input stride of 4 k + 2", (L, xin, n_in, xs + 2, yout, ys, n_out, 1)), ("an output stride of 4 k + 1", (L, xin, n_in, xs, yout, ys + 1, n_out, 1))]:
        rc = lib.sdrhip_interpolate_ragged(bank.h, *args)
        assert rc == -4 and b"aligned" in lib.sdrhip_last_error(), (what, rc)
    ctx.synchronize()
    assert list(n_out) == [7, 7, 7] and (y == SENTINEL).all()
    out, got_n = bank.interpolate_ragged(L, x, calls[1])
    ctx.synchronize()
    for s in range(S):
        assert np.array_equal(host(out)[s, :got_n[s]], exp[1][s]), s
