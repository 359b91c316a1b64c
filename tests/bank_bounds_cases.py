"""Case tables and the buffer builder of the bank bounds tests (test_gpu_bank_bounds.py on the GPU, test_bank_bounds_cases.py for the
tables themselves).  Plain Python and numpy: no GPU, no library.

Every buffer those tests hand to the library is a view into an `arena`: rows 1..S of an (S + 2, stride, 2) array whose first and
last row are guards and whose rows are longer than the call's.  What a kernel or a staging copy reads or writes past a row's count
therefore lands in memory the test owns and looks at, never at the end of an allocation.

The shapes are the smallest at which each store form and each piece edge occurs.  A decimator shape is base + k * 2^L + r: k extra
output samples and a dropped remainder r, with (k, r) in KR, so that n_out mod 8 is 1, 2, 3 and 7 and the remainder 0, 1 and the
largest (taken modulo 2^L: decimate1 drops nothing, decimate2 at most one sample).  The planners' rules (decim_plan.h,
interp_ragged_plan.h) are restated here so that every case NAMES the launch it is meant to get: sdrhip_*_last_plan has to agree, a
case cannot pass on another path."""
import numpy as np

SENTINEL = 0x5a5a
GUARD = 1024                    # fewest samples of a guard row (K1m's ring reads 256 samples ahead, a uint4 store spans 4)
GAP = 8                         # fewest samples between a row's count and its stride
ZEROCOPY_MAX = 384 * 1024       # SDRHIP_ZEROCOPY_MAX: staged bytes up to which a host call of the decimators goes pinned zero-copy
FC_INF, FC_SUP, FC_CEN = 0, 1, 2
FILLS = ("noise", "rails")
KR = [(1, 0), (2, "max"), (3, 1), (7, 0)]
SECOND = 4096                   # fresh samples per stream of the call that follows on each bank

DECIM_DEFAULTS = {"decim_path": "auto", "mfma_span": 0, "mfma_ring": 4}
INTERP_DEFAULTS = {"interp_path": "auto", "interp_span": 0}


def stride_for(n):
    """the row stride of a call of n samples: a multiple of 4, at least GAP behind the samples, and a guard row's length"""
    return max((n + GAP + 3) & ~3, GUARD)


def arena(S, n, stride, guard, fill):
    """-> (the (S + 2, stride, 2) int16 arena, its (S, n, 2) view of rows 1..S).  Guard rows (of `stride` >= `guard` samples) and
    gaps hold `fill`: an int (outputs: SENTINEL), "noise" (full-scale RandomState) or "rails" (+32767 / -32768 alternating); the
    view's samples hold it too until the caller writes the valid ones."""
    assert stride % 4 == 0 and stride - n >= GAP and stride >= guard >= GUARD and S >= 1 and n >= 0
    if fill == "noise":
        a = np.random.RandomState(0xB0B + S + n).randint(-32768, 32768, size=(S + 2, stride, 2)).astype(np.int16)
    elif fill == "rails":
        a = np.empty((S + 2, stride, 2), np.int16)
        a[:, 0::2] = 32767
        a[:, 1::2] = -32768
    else:
        a = np.full((S + 2, stride, 2), int(fill), np.int16)
    return a, a[1:S + 1, :n]


def stream_samples(s, n, bits=16, second=False):
    """the valid samples of stream s (and of its following call): full-scale noise of `bits` effective bits, every stream its own"""
    x = np.random.RandomState(4000 + 2 * s + (1 if second else 0)).randint(-32768, 32768, size=(n, 2)).astype(np.int16)
    return (x >> (16 - bits)).astype(np.int16)


def input_arena(S, counts, fill, bits=None, signal_of=None):
    """the input of a call: an arena of the largest count, row s = the first counts[s] samples of stream s (of signal signal_of(s),
    where streams share signals), `fill` everywhere else"""
    n = max(counts)
    a, v = arena(S, n, stride_for(n), GUARD, fill)
    for s in range(S):
        v[s, :counts[s]] = stream_samples(signal_of(s) if signal_of else s, counts[s], 16 if bits is None else bits[s])
    return a, v


def remainder(L, r):
    return ((1 << L) - 1 if r == "max" else r) % (1 << L)


def shape(base, L, k, r):
    return base + (k << L) + remainder(L, r)


# ------------------------------------------------------------------------------ the planners' rules, restated (decim_plan.h)
def plan_decimate(L, fcpos, n_used, S):
    """-> (passes per segment, segments per stream) of K1"""
    cen = fcpos == FC_CEN
    praw = 2048 if cen else 8192
    npass = max(1, -(-n_used // praw))
    ns = L if cen else L - 2
    period = 1 << max(ns - 2, 0)
    per = max(32, period)
    while per > period and -(-npass // per) * S < 2048:
        per >>= 1
    while per > 1 and -(-npass // per) * S < 256:
        per >>= 1
    while per * praw < (64 << L):
        per <<= 1
    return per, -(-npass // per)


def plan_decimate_ragged(L, fcpos, used, S):
    """-> workgroups of K1r: the segments of every stream (at least one each), sized for the mean stream"""
    per, _ = plan_decimate(L, fcpos, -(-sum(used) // S), S)
    seg_raw = per * (2048 if fcpos == FC_CEN else 8192)
    return sum(-(-n // seg_raw) if n else 1 for n in used)


MF_READ_AHEAD, MF_TAIL_SEG = 256, 16384


def mf_span(L, span_opt):
    W = 64 << L
    return -(-span_opt // W) * W


def mf_head(L):
    return max(64 << L, 2048)


def plan_mfma(L, n_used, span_opt):
    """K1m with a forced span -> dict(head, span, wps, tail_start, npieces), or None where the planner declines"""
    head, span = mf_head(L), mf_span(L, span_opt)
    if not 2 <= L <= 6 or n_used <= head:
        return None
    wps = (n_used - head) // (8 * span)
    if wps and n_used - (head + wps * 8 * span) < MF_READ_AHEAD:
        wps -= 1
    if wps == 0:
        return None
    tail_start = head + wps * 8 * span
    return {"head": head, "span": span, "wps": wps, "tail_start": tail_start, "npieces": 1 + max(1, -(-(n_used - tail_start) // MF_TAIL_SEG))}


def plan_mfma_ragged(L, used, span_opt):
    """K1mr -> dict(head, span, wps, npieces) with the launch's totals, or None"""
    S = len(used)
    u = plan_mfma(L, sum(used) // S >> L << L, span_opt)
    if u is None:
        return None
    head, span, waves, pieces = u["head"], u["span"], 0, 0
    for n in used:
        wps = (n - head) // (8 * span) if n > head else 0
        tail_start = head + wps * 8 * span
        if wps and n - tail_start < MF_READ_AHEAD:
            wps -= 1
            tail_start = head + wps * 8 * span
        if not wps:
            tail_start = min(n, MF_TAIL_SEG)
        waves += wps
        pieces += 1 + -(-(n - tail_start) // MF_TAIL_SEG)
    return {"head": head, "span": span, "wps": waves, "npieces": pieces, "tail_start": 0} if waves else None


def plan_interp(path, span, L, n, S):
    """the uniform interpolator launch -> dict(path, seg_len, wpw, entries, compact) as sdrhip_interpolators_last_plan reports it"""
    if L == 0:
        return {"path": "copy", "seg_len": n, "wpw": 1, "entries": S, "compact": False}
    if path == "wave" and L >= 2:
        nsub = max(1, -(-n // 128))
        per = min(-(-span // 128), 16) if span else 16
        if per > 1:
            per &= ~1
        nseg = -(-nsub // per)
        return {"path": "wave", "seg_len": per * 128, "wpw": 4 if nseg * S >= 4096 else 1, "entries": nseg * S, "compact": False}
    ci = 1024 if L == 1 else 512
    nsub, per = max(1, -(-n // ci)), 16
    while per > 1 and -(-nsub // per) * S < 2048:
        per >>= 1
    return {"path": "valu", "seg_len": per * ci, "wpw": 1, "entries": -(-nsub // per) * S, "compact": False}


# ------------------------------------------------------------------------------ decimator bank, uniform calls (3 streams)
DECIM_S = 3
FCN = {FC_INF: "inf", FC_SUP: "sup", FC_CEN: "cen"}


def _decim_case(family, L, fcpos, n_in, opts, bias=0, tag=""):
    used = n_in >> L << L
    if opts["decim_path"] == "mfma":
        expect = dict(plan_mfma(L, used, opts["mfma_span"]), path="mfma")
    elif L == 0 or (fcpos != FC_CEN and L <= 2):
        expect = {"path": None}
    else:
        expect = {"path": "valu", "nseg": plan_decimate(L, fcpos, used, DECIM_S)[1]}
    return {"id": "%s-L%d-%s-n%d%s%s" % (family, L, FCN[fcpos], n_in, "-db" if bias else "", tag), "family": family, "L": L, "fcpos": fcpos,
            "bias": bias, "n_in": n_in, "S": DECIM_S, "opts": dict(DECIM_DEFAULTS, **opts), "expect": expect}


K1_CEN_BASE, K1_ROT_BASE, SIMPLE_BASE = 5 * 2048, 3 * 8192, 4096
VALU = {"decim_path": "valu"}


def mf_base(L, span_opt, groups=16):
    """K1m: head + `groups` spans (two wave groups of 8 for a uniform stream) + a tail of 3072 samples"""
    return mf_head(L) + groups * mf_span(L, span_opt) + 3072


MF_TAIL_BASE = 2048 + 32768 + 20480  # L = 4, spans of 4096: one wave group, a tail across MF_TAIL_SEG


def _mf(span, ring=4):
    return {"decim_path": "mfma", "mfma_span": span, "mfma_ring": ring}


def _uniform_decim():
    c = []
    for L in range(1, 7):
        c += [_decim_case("k1", L, FC_CEN, shape(K1_CEN_BASE, L, k, r), VALU) for k, r in KR]
    c.append(_decim_case("k1", 4, FC_CEN, shape(K1_CEN_BASE, 4, 3, 1), VALU, bias=1))
    for L in range(3, 7):
        for fc in (FC_INF, FC_SUP):
            c += [_decim_case("k1", L, fc, shape(K1_ROT_BASE, L, k, r), VALU) for k, r in KR]
    for L, fc in [(0, FC_CEN), (1, FC_INF), (1, FC_SUP), (2, FC_INF), (2, FC_SUP)]:
        c += [_decim_case("simple", L, fc, shape(SIMPLE_BASE, L, k, r), VALU) for k, r in KR]
    for L in range(2, 7):
        c += [_decim_case("k1m", L, FC_CEN, shape(mf_base(L, 1024), L, k, r), _mf(1024)) for k, r in KR]
    c.append(_decim_case("k1m", 4, FC_CEN, shape(mf_base(4, 1024), 4, 3, 1), _mf(1024), bias=1))
    c += [_decim_case("k1m-tail", 4, FC_CEN, shape(MF_TAIL_BASE, 4, k, r), _mf(4096)) for k, r in KR]
    c += [_decim_case("k1m-ring", 4, FC_CEN, shape(mf_base(4, 1024), 4, 3, 1), _mf(1024, ring), tag="-ring%d" % ring) for ring in (3, 2)]
    return c


DECIM_UNIFORM = _uniform_decim()

# ------------------------------------------------------------------------------ decimator bank, ragged calls (5 streams)
RAGGED_S = 5


def ragged_bits(L):
    return [16, 8, 12, 16 - L, 13]


def _ragged_case(family, L, fcpos, a, b, opts):
    counts = [a, 0, (1 << L) - 1, b, 1 << L]
    used = [n >> L << L for n in counts]
    if opts["decim_path"] == "mfma":
        expect = dict(plan_mfma_ragged(L, used, opts["mfma_span"]), path="mfma")
    elif L == 0 or (fcpos != FC_CEN and L <= 2):
        expect = {"path": None}
    else:
        expect = {"path": "valu", "nseg": plan_decimate_ragged(L, fcpos, used, RAGGED_S)}
    return {"id": "%s-L%d-%s-%d-%d" % (family, L, FCN[fcpos], a, b), "family": family, "L": L, "fcpos": fcpos, "bias": 0, "counts": counts,
            "S": RAGGED_S, "opts": dict(DECIM_DEFAULTS, **opts), "expect": expect}


def _ragged_decim():
    """A and B: the four shapes of the uniform table for the path, two a case"""
    c = []
    pairs = [(KR[0], KR[1]), (KR[2], KR[3])]
    for L in range(1, 7):
        c += [_ragged_case("k1r", L, FC_CEN, shape(K1_CEN_BASE, L, *p), shape(K1_CEN_BASE, L, *q), VALU) for p, q in pairs]
    for L in range(3, 7):
        for fc in (FC_INF, FC_SUP):
            c += [_ragged_case("k1r", L, fc, shape(K1_ROT_BASE, L, *p), shape(K1_ROT_BASE, L, *q), VALU) for p, q in pairs]
    for L, fc in [(0, FC_CEN), (1, FC_INF), (1, FC_SUP), (2, FC_INF), (2, FC_SUP)]:
        c += [_ragged_case("simple", L, fc, shape(SIMPLE_BASE, L, *p), shape(SIMPLE_BASE, L, *q), VALU) for p, q in pairs]
    for L in range(2, 7):  # (4 x 8 spans: the mean of the five streams still holds a span, K1mr plans from the mean)
        c += [_ragged_case("k1mr", L, FC_CEN, shape(mf_base(L, 1024, 32), L, *p), shape(mf_base(L, 1024, 32), L, *q), _mf(1024)) for p, q in pairs]
    return c


DECIM_RAGGED = _ragged_decim()

# ------------------------------------------------------------------------------ interpolator bank, uniform calls
INTERP_S = 3
INTERP_N = [1, 127, 129, 513, 2049, 4001]
INTERP_L = [0, 1, 2, 4, 6]


def _interp_case(S, n, L, path, span, signal_of=None, tag=""):
    return {"id": "%sx%d-n%d-%s-span%d" % (tag, 1 << L, n, path, span), "S": S, "n_in": n, "L": L, "signal_of": signal_of or (lambda s: s),
            "opts": {"interp_path": path, "interp_span": span}, "expect": plan_interp(path, span, L, n, S)}


INTERP_UNIFORM = [_interp_case(INTERP_S, n, L, path, span) for L in INTERP_L for n in INTERP_N for path in ("valu", "wave") for span in (0, 128)]
# workgroups of four waves: 17 streams x 253 one-block segments = 4301 entries, 253 no multiple of 4; stream s carries signal s % 3
FOUR_S, FOUR_N = 17, 32257
INTERP_FOUR = _interp_case(FOUR_S, FOUR_N, 2, "wave", 128, signal_of=lambda s: s % 3, tag="four-")

# ------------------------------------------------------------------------------ TestSource bank
TS_S = 3
TS_CONFIGS = ["srate=10000000,dfp=100000,power=20", "srate=2400000,dfn=37000,power=0", "srate=8000,dfp=4000,power=3"]
TS_PARAMS = [(100000, 10000000, 20), (-37000, 2400000, 0), (4000, 8000, 3)]  # (offset, rate, power) as the oracle's NCO takes them
TS_N = [1, 3, 4099]


def staged_bytes(S, n_in):
    """what a host call of S rows of n_in samples stages, as the library evaluates it against ZEROCOPY_MAX"""
    return S * ((n_in + 3) & ~3) * 4
