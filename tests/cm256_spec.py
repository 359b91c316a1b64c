"""CM256 written from its SPECIFICATION only (shared by test_cm256_spec_independent.py and test_gpu_cm256_geometry.py); it shares no
line with the oracle (oracle/sdr_oracle.c) or the product (sdrdaemon_amd/csrc/gf256.cpp).  Two facts about upstream cm256 / gf256:
  (A) the field polynomial is entry 3 of gf256's table of generator polynomials, which lists the sixteen degree-8 polynomials for which
      x is primitive in ascending order (stored as p >> 1) -- derived below by enumeration, never typed in;
  (B) recovery row i, column j of the encoder is (y_j + x_0) / (x_i + y_j) with x_i = OriginalCount + i, y_j = j (a Cauchy matrix
      normalised so that row 0 is all ones), recovery block i = sum_j a_ij * original_j.
Arithmetic is bit-serial carry-less multiplication and brute-force inversion (no logarithm tables, no generator), decoding is plain
Gaussian elimination on [I; A] (no closed-form Cauchy inverse, no LDU)."""
import numpy as np


def _clmul_mod(a, b, poly):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= poly
        b >>= 1
    return r


def _x_is_primitive(poly):
    # x generates the multiplicative group iff its order is 255 (then the polynomial is irreducible as well)
    v, n = 2, 1
    while v != 1:
        v = _clmul_mod(v, 2, poly)
        n += 1
        if n > 255:
            return False
    return n == 255


def field():
    """-> (polynomial, 256 x 256 multiplication table, inverses): what every helper below takes as `spec`"""
    prim = [p for p in range(0x101, 0x200, 2) if _x_is_primitive(p)]
    assert len(prim) == 16  # phi(255) / 8
    poly = prim[3]          # fact (A)
    mul = np.zeros((256, 256), np.uint8)
    for a in range(256):
        for b in range(a, 256):
            mul[a, b] = mul[b, a] = _clmul_mod(a, b, poly)
    inv = np.zeros(256, np.uint8)
    for a in range(1, 256):
        inv[a] = int(np.nonzero(mul[a] == 1)[0][0])
    return poly, mul, inv


def _matrix(spec, k, m):
    _, mul, inv = spec
    a = np.zeros((m, k), np.uint8)
    for i in range(m):
        for j in range(k):
            a[i, j] = mul[j ^ k, inv[(k + i) ^ j]]  # fact (B)
    return a


def _encode(spec, x, m):
    _, mul, _ = spec
    a = _matrix(spec, x.shape[0], m)
    rec = np.zeros((m, x.shape[1]), np.uint8)
    for i in range(m):
        for j in range(x.shape[0]):
            rec[i] ^= mul[a[i, j]][x[j]]
    return rec


def _solve(spec, k, rows, data):
    """originals from any k of the k + m blocks: rows[t] = block index (< k: original, >= k: recovery row - k), data[t] its bytes."""
    _, mul, inv = spec
    m = max([r - k + 1 for r in rows if r >= k] + [1])
    a = _matrix(spec, k, m)
    g = np.zeros((k, k), np.uint8)
    for t, r in enumerate(rows):
        if r < k:
            g[t, r] = 1
        else:
            g[t] = a[r - k]
    g, d = g.copy(), data.copy()
    for c in range(k):  # Gauss-Jordan over GF(2^8)
        p = next(t for t in range(c, k) if g[t, c])
        if p != c:
            g[[c, p]] = g[[p, c]]
            d[[c, p]] = d[[p, c]]
        s = inv[g[c, c]]
        g[c] = mul[s][g[c]]
        d[c] = mul[s][d[c]]
        for t in range(k):
            if t != c and g[t, c]:
                f = g[t, c]
                g[t] ^= mul[f][g[c]]
                d[t] ^= mul[f][d[c]]
    return d


# ------------------------------------------------------------------ the geometries and deliveries the CM256 tests share
# (OriginalCount, RecoveryCount, erasures): both small extremes, k + m = 256 from both sides, and the erasure counts at which the GPU
# kernel behind the generic entry points changes its row tile (16 | 17, 24 | 25) or its workgroup count (32 | 33, 64 | 65)
GEOMETRIES = [(2, 2, 2), (2, 254, 1), (3, 5, 3), (5, 3, 2),
              (16, 16, 16), (17, 17, 17), (20, 20, 20), (24, 40, 24), (25, 40, 25), (33, 33, 33),
              (100, 40, 16), (100, 40, 17), (100, 40, 32), (100, 40, 33),
              (200, 56, 56), (255, 1, 1), (254, 2, 2), (129, 127, 65), (127, 129, 127)]


def pick(rs, k, m, n, include=()):
    """n erased originals (ascending, `include` among them) and n distinct recovery rows from anywhere in 0 .. m - 1, in any order"""
    rest = [j for j in range(k) if j not in include]
    erased = sorted(list(include) + rs.choice(rest, n - len(include), replace=False).tolist()) if n > len(include) else sorted(include)
    rows = rs.choice(m, n, replace=False).tolist()
    return erased, rows


def arrival(rs, k, erased, rows, mode):
    """block numbers (original j, or k + recovery row) in arrival order: "recovery_last" = originals shuffled, recovery blocks
    behind them (SDRdaemonFECBuffer.cpp:210), "shuffled" = everything anywhere"""
    keep = [j for j in range(k) if j not in set(erased)]
    rs.shuffle(keep)
    order = keep + [k + r for r in rows]
    if mode == "shuffled":
        rs.shuffle(order)
    else:
        assert mode == "recovery_last"
    return np.array(order)
