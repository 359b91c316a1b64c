"""The case tables of the bank bounds tests (bank_bounds_cases.py) claim what they claim -- every store form and remainder per path
and ratio, gaps and guards around every row, the launches they name, host calls on both sides of the zero-copy limit -- so that a
later edit cannot hollow them out; and the oracle, given rows of an arena, does not look behind them: the property the GPU tests
demand of the library is one the reference has.  No GPU, no library."""
import numpy as np

import bank_bounds_cases as B


def _groups(cases, key):
    g = {}
    for c in cases:
        g.setdefault(key(c), []).append(c)
    return g


def _residues(L, counts):
    return {(n >> L) % 8 for n in counts}, {n % (1 << L) for n in counts}


def _wanted(L):
    return {1, 2, 3, 7}, {B.remainder(L, r) for r in (0, 1, "max")}


def test_every_store_form_and_remainder_per_path_and_ratio():
    uniform = [c for c in B.DECIM_UNIFORM if c["family"] != "k1m-ring" and not c["bias"]]
    groups = _groups(uniform, lambda c: (c["family"], c["L"], c["fcpos"]))
    assert {k[:2] for k in groups} >= ({("k1", L) for L in range(1, 7)} | {("simple", L) for L in range(3)} | {("k1m", L) for L in range(2, 7)}
                                       | {("k1m-tail", 4)})
    assert {k for k in groups if k[0] == "k1" and k[2] != B.FC_CEN} == {("k1", L, fc) for L in range(3, 7) for fc in (B.FC_INF, B.FC_SUP)}
    assert {k for k in groups if k[0] == "simple"} == {("simple", 0, B.FC_CEN)} | {("simple", L, fc) for L in (1, 2) for fc in (B.FC_INF, B.FC_SUP)}
    for (family, L, fc), cs in groups.items():
        assert _residues(L, [c["n_in"] for c in cs]) == _wanted(L), (family, L, fc)
    ragged = _groups(B.DECIM_RAGGED, lambda c: (c["family"], c["L"], c["fcpos"]))
    assert len(ragged) == len(groups) - 1  # (every path, ratio and position of the uniform table but the long-tail shape)
    for (family, L, fc), cs in ragged.items():
        assert _residues(L, [n for c in cs for n in (c["counts"][0], c["counts"][3])]) == _wanted(L), (family, L, fc)
    assert [(c["family"], c["L"]) for c in B.DECIM_UNIFORM if c["bias"]] == [("k1", 4), ("k1m", 4)]  # (the one K1 and the one K1m case at bias 1)
    assert not any(c["bias"] for c in B.DECIM_RAGGED)
    rings = [c for c in B.DECIM_UNIFORM if c["family"] == "k1m-ring"]
    assert [(c["opts"]["mfma_ring"], c["L"], c["n_in"]) for c in rings] == [(r, 4, B.shape(B.mf_base(4, 1024), 4, 3, 1)) for r in (3, 2)]
    ids = [c["id"] for c in B.DECIM_UNIFORM + B.DECIM_RAGGED + B.INTERP_UNIFORM]
    assert len(set(ids)) == len(ids)


def test_rows_have_gaps_and_guards():
    counts = [c["n_in"] for c in B.DECIM_UNIFORM] + [c["n_in"] >> c["L"] for c in B.DECIM_UNIFORM]
    counts += [max(c["counts"]) for c in B.DECIM_RAGGED] + [max(c["counts"]) >> c["L"] for c in B.DECIM_RAGGED]
    counts += [c["n_in"] << k for c in B.INTERP_UNIFORM + [B.INTERP_FOUR] for k in (0, c["L"])] + B.TS_N + [B.SECOND]
    for n in counts:
        stride = B.stride_for(n)
        assert stride % 4 == 0 and stride - n >= 8 and stride >= 1024, n
        a, v = B.arena(2, n, stride, B.GUARD, B.SENTINEL)
        assert a.shape == (4, stride, 2) and v.shape == (2, n, 2) and v.base is a and (a == B.SENTINEL).all()
    # inputs of at most about 140 k samples a stream; the one large output is the four-wave case's, about 9 MB
    assert max([c["n_in"] for c in B.DECIM_UNIFORM + B.INTERP_UNIFORM + [B.INTERP_FOUR]] + [max(c["counts"]) for c in B.DECIM_RAGGED]) <= 140000
    assert max(c["S"] * (c["n_in"] << c["L"]) * 4 for c in B.INTERP_UNIFORM) < B.FOUR_S * (B.FOUR_N << 2) * 4 < 9 << 20
    noise, _ = B.arena(3, 100, 1024, 1024, "noise")
    rails, _ = B.arena(3, 100, 1024, 1024, "rails")
    assert noise.min() < -32000 and noise.max() > 32000 and (rails[:, 0::2] == 32767).all() and (rails[:, 1::2] == -32768).all()


def test_the_cases_name_the_launches_they_are_meant_for():
    for c in B.DECIM_UNIFORM:
        L, used, e = c["L"], c["n_in"] >> c["L"] << c["L"], c["expect"]
        if c["family"] == "k1":
            assert e["path"] == "valu" and e["nseg"] >= 3, c["id"]  # (warm-up and state hand-over are in play)
        elif c["family"] == "simple":
            assert e == {"path": None}, c["id"]
        else:
            tail = c["family"] == "k1m-tail"
            assert e["path"] == "mfma" and used > e["head"] + 8 * e["span"] + 256, c["id"]
            assert (e["wps"], e["npieces"]) == ((1, 3) if tail else (2, 2)), c["id"]  # (two wave groups and a one-piece tail, or a tail across MF_TAIL_SEG)
            assert e["span"] == (4096 if tail else max(1024, 64 << L)) and e["head"] == max(64 << L, 2048), c["id"]
            assert used - e["tail_start"] >= (16384 + 256 if tail else 3072), c["id"]
    for c in B.DECIM_RAGGED:
        L, cnt, e = c["L"], c["counts"], c["expect"]
        assert 0 in cnt and (1 << L) in cnt and any(n < (1 << L) for n in cnt) and cnt[0] != cnt[3], c["id"]
        assert cnt[2] == (1 << L) - 1 and len(cnt) == 5 and len(B.ragged_bits(L)) == 5 and B.ragged_bits(L)[3] == 16 - L
        if c["family"] == "k1mr":
            assert e["path"] == "mfma" and e["wps"] >= 2 and all(n > e["head"] + 8 * e["span"] + 256 for n in (cnt[0], cnt[3])), c["id"]
        elif c["family"] == "k1r":
            assert e["path"] == "valu" and e["nseg"] >= 3 + 3 + 3, c["id"]  # (A and B in segments, one each for the streams without a pass)
        else:
            assert e == {"path": None}, c["id"]


def test_host_cases_lie_on_both_sides_of_the_zero_copy_limit():
    """sdrhip_decimate, sdrhip_decimate_ragged and _ragged_bits (the same counts) stage host rows through pinned zero-copy memory up to
    384 KiB and through copies above; sdrhip_interpolate and sdrhip_testsource_read have one route (a 2-D copy) at every size --
    the interpolator's cases lie on both sides all the same, the TestSource's sizes are set, at most 4099 samples"""
    sizes = {"decimate": [B.staged_bytes(c["S"], c["n_in"]) for c in B.DECIM_UNIFORM],
             "decimate_ragged": [B.staged_bytes(c["S"], max(c["counts"])) for c in B.DECIM_RAGGED],
             "interpolate": [B.staged_bytes(c["S"], c["n_in"]) for c in B.INTERP_UNIFORM + [B.INTERP_FOUR]]}
    for entry, b in sizes.items():
        assert min(b) <= B.ZEROCOPY_MAX < max(b), entry
    for path in ("valu", "mfma"):  # (and either kernel family of the uniform decimator on either side)
        b = [B.staged_bytes(c["S"], c["n_in"]) for c in B.DECIM_UNIFORM if c["opts"]["decim_path"] == path and c["expect"]["path"]]
        assert (min(b) <= B.ZEROCOPY_MAX < max(b)) == (path == "mfma"), path


def test_the_interpolator_shapes():
    want = {(n, L, path, span) for n in (1, 127, 129, 513, 2049, 4001) for L in (0, 1, 2, 4, 6) for path in ("valu", "wave") for span in (0, 128)}
    assert {(c["n_in"], c["L"], c["opts"]["interp_path"], c["opts"]["interp_span"]) for c in B.INTERP_UNIFORM} == want
    assert all(c["S"] == 3 for c in B.INTERP_UNIFORM)
    # x2 with an odd count: the one ratio whose per-stream byte count is no multiple of 16
    assert any(c["L"] == 1 and c["n_in"] % 2 and (c["n_in"] << 1) * 4 % 16 for c in B.INTERP_UNIFORM)
    for c in B.INTERP_UNIFORM:
        e, L, path, span = c["expect"], c["L"], c["opts"]["interp_path"], c["opts"]["interp_span"]
        assert e["path"] == ("copy" if L == 0 else "wave" if path == "wave" and L >= 2 else "valu") and e["wpw"] == 1, c["id"]
        if e["path"] == "wave":
            assert e["seg_len"] == (128 if span else 2048), c["id"]
    assert {c["expect"]["path"] for c in B.INTERP_UNIFORM} == {"copy", "valu", "wave"}
    f = B.INTERP_FOUR
    nseg = -(-f["n_in"] // 128)
    assert f["S"] == 17 and f["L"] == 2 and nseg == 253 and nseg % 4 != 0 and nseg * 17 == 4301 >= 4096
    assert f["expect"] == {"path": "wave", "seg_len": 128, "wpw": 4, "entries": 4301, "compact": False}
    assert [f["signal_of"](s) for s in range(17)] == [s % 3 for s in range(17)]


def test_the_testsource_shapes():
    assert B.TS_S == 3 and B.TS_N == [1, 3, 4099] and len(set(B.TS_CONFIGS)) == 3 and len(set(B.TS_PARAMS)) == 3


def _decimate_rows(oracle, c, counts, fill, bits=None):
    _, v = B.input_arena(c["S"], counts, fill, bits)
    return [oracle.decimators(c["bias"]).decimate(c["L"], c["fcpos"], bits[s] if bits else 16, v[s, :counts[s]])[0] for s in range(c["S"])]


def test_the_oracle_does_not_look_behind_a_row(oracle):
    """one case of each family with both fills behind the rows: the oracle reads the arena's own memory (a row's samples are
    contiguous there) and returns the same bytes"""
    first = {}
    for c in B.DECIM_UNIFORM:
        first.setdefault(c["family"], c)
    assert set(first) == {"k1", "simple", "k1m", "k1m-tail", "k1m-ring"}
    for c in first.values():
        a, b = (_decimate_rows(oracle, c, [c["n_in"]] * c["S"], fill) for fill in B.FILLS)
        assert all(x.shape == (c["n_in"] >> c["L"], 2) and np.array_equal(x, y) for x, y in zip(a, b)), c["id"]
    first = {}
    for c in B.DECIM_RAGGED:
        first.setdefault(c["family"], c)
    assert set(first) == {"k1r", "simple", "k1mr"}
    for c in first.values():
        for bits in (None, B.ragged_bits(c["L"])):
            a, b = (_decimate_rows(oracle, c, c["counts"], fill, bits) for fill in B.FILLS)
            assert all(x.shape == (n >> c["L"], 2) and np.array_equal(x, y) for x, y, n in zip(a, b, c["counts"])), c["id"]
    for c in (B.INTERP_UNIFORM[-1], B.INTERP_FOUR):
        res = []
        for fill in B.FILLS:
            _, v = B.input_arena(3, [c["n_in"]] * 3, fill)  # (three signals serve the seventeen streams)
            res.append([oracle.interpolators().interpolate(c["L"], v[s]) for s in range(3)])
        assert all(x.shape == (c["n_in"] << c["L"], 2) and np.array_equal(x, y) for x, y in zip(*res)), c["id"]
