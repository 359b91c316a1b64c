"""The bit-sliced form of the FFT encoder (sdrdaemon_amd/csrc/gf_encode128_bs.h) restated in numpy, lane by lane: the table-form
stages on 4-byte columns, the octet bit transpose (the kernel's delta swaps on uint32), the inverse stages 3..5, the folds and the
first forward stage as XOR trees on bit planes with the matrices derived by the header's rules (field 0x14D, constants from the
subspace polynomials -- not from the oracle), the transpose back, and the rest in the table form.  Checked against the oracle's
cm256_encode for every row count the kernel serves, on random and all-0xFF payloads.  CPU only."""
import numpy as np
import pytest


def gmul(a, b):  # bs_gmul
    r = 0
    for i in range(8):
        if b >> i & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x14D
    return r


def ginv(a):  # bs_ginv: a^254
    r = 1
    for _ in range(254):
        r = gmul(r, a)
    return r


def s_k(k, x):  # bs_s
    v = x
    for i in range(k):
        v = gmul(v, v ^ s_k(i, 1 << i))
    return v


def shat(k, x):  # bs_shat
    return gmul(s_k(k, x), ginv(s_k(k, 1 << k)))


def mat_rows(c):  # bs_mat: row p has bit q when bit p of c * 2^q is set
    rows = [0] * 8
    for q in range(8):
        col = gmul(c, 1 << q)
        for p in range(8):
            if col >> p & 1:
                rows[p] |= 1 << q
    return rows


MUL = np.array([[gmul(a, b) for b in range(256)] for a in range(256)], np.uint8)


def tmul(c, v):  # the table form on uint32 columns: every byte times c
    return MUL[c][v.view(np.uint8)].view(np.uint32)


def bs_muladd(c, a, b):  # a ^= c * b on 8 planes (lists of uint32 arrays)
    for p, row in enumerate(mat_rows(c)):
        for q in range(8):
            if row >> q & 1:
                a[p] = a[p] ^ b[q]


def transpose8(x):  # bs_transpose8: three delta-swap stages, an involution
    x = list(x)
    for j, m in ((4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
        m = np.uint32(m)
        for t in range(8):
            if t & j:
                continue
            a, b = x[t], x[t + j]
            x[t] = (a & m) | ((b << np.uint32(j)) & ~m)
            x[t + j] = ((a >> np.uint32(j)) & m) | (b & ~m)
    return x


def wave_inverse(d, hf):
    """one wave's 64 values (d[i]: uint32 column array of block 64 hf + i) -> 4 octets of planes: the half's 32 coefficients"""
    d = [v.copy() for v in d]
    for m in range(8):  # 1. stages 0..2 per octet in the table form, then the octet to planes
        for k in range(3):
            h = 1 << k
            for jj in range(4 >> k):
                j = m * (4 >> k) + jj
                blk = j * 2 * h
                c = shat(k, (64 * hf) ^ (j << (k + 1)))
                for i in range(h):
                    d[blk + h + i] = d[blk + h + i] ^ d[blk + i]
                    d[blk + i] = d[blk + i] ^ tmul(c, d[blk + h + i])
        d[8 * m:8 * m + 8] = transpose8(d[8 * m:8 * m + 8])
    o = [d[8 * i:8 * i + 8] for i in range(8)]
    for k in range(3, 6):  # 2. stages 3..5 on planes, octet pairs
        ho = 1 << (k - 3)
        for j in range(32 >> k):
            c = shat(k, (64 * hf) ^ (j << (k + 1)))
            for i in range(ho):
                lo, hi = 2 * j * ho + i, 2 * j * ho + i + ho
                for p in range(8):
                    o[hi][p] = o[hi][p] ^ o[lo][p]
                bs_muladd(c, o[lo], o[hi])
    for i in range(4):  # t5 fold
        bs_muladd(shat(5, 128), o[i], o[i + 4])
    return o[:4]


def encode_model(data, R):
    """data (128, 508) -> (R, 508) through the kernel's steps"""
    cols = data.view(np.uint32)  # (128, 127): one lane per column, all columns at once
    d = [[cols[64 * hf + i].copy() for i in range(64)] for hf in range(2)]
    par = np.bitwise_xor.reduce(cols, axis=0)
    lo, hi = wave_inverse(d[0], 0), wave_inverse(d[1], 1)
    t6, s4 = shat(6, 128), shat(4, 128)
    e = [None, None]
    e[0], e[1] = [], []
    for o in range(2):  # 3. the exchange on planes: t6, stage 4 of the size-32 transform
        va, vb = list(lo[o]), list(lo[o + 2])
        dl, dh = hi[o], hi[o + 2]
        dl = [dl[p] ^ va[p] for p in range(8)]
        bs_muladd(t6, va, dl)
        dh = [dh[p] ^ vb[p] for p in range(8)]
        bs_muladd(t6, vb, dh)
        bs_muladd(s4, va, vb)
        e[0].append(va)
        e[1].append([vb[p] ^ va[p] for p in range(8)])
    c = 1
    for v in range(1, 128):
        c = gmul(c, v)
    q = s_k(7, 128)
    rows = []
    for hf in range(2):  # 4. stage 3 on planes, back to bytes, stages 2..0 and the row scales
        a, b = e[hf]
        bs_muladd(shat(3, 128 ^ (hf << 4)), a, b)
        b = [b[p] ^ a[p] for p in range(8)]
        v = transpose8(a) + transpose8(b)
        for k in (2, 1, 0):
            h = 1 << k
            for j in range(8 >> k):
                cc = shat(k, 128 ^ (((8 >> k) * hf + j) << (k + 1)))
                blk = j * 2 * h
                for i in range(h):
                    v[blk + i] = v[blk + i] ^ tmul(cc, v[blk + h + i])
                    v[blk + h + i] = v[blk + h + i] ^ v[blk + i]
        for i in range(16):
            r = 16 * hf + i
            rows.append(par ^ tmul(gmul(gmul(r, c), ginv(q)), v[i]))
    return np.stack(rows[:R]).view(np.uint8).reshape(R, 508)


def test_constants_match_the_field(oracle):
    """the header's compile-time arithmetic is the oracle's field"""
    for a, b in ((3, 77), (128, 19), (200, 255), (1, 1), (0x8E, 0x47)):
        assert gmul(a, b) == oracle.gf_mul(a, b)
    for a in (1, 2, 77, 255):
        assert gmul(a, ginv(a)) == 1


def test_transpose_is_a_bit_transpose_and_an_involution():
    rs = np.random.RandomState(5)
    x = [rs.randint(0, 1 << 32, size=16, dtype=np.uint64).astype(np.uint32) for _ in range(8)]
    y = transpose8(x)
    for t in range(8):
        for p in range(8):
            for B in range(4):
                assert np.array_equal((x[t] >> np.uint32(8 * B + p)) & 1, (y[p] >> np.uint32(8 * B + t)) & 1)
    assert all(np.array_equal(a, b) for a, b in zip(transpose8(y), x))


@pytest.mark.parametrize("fill", ["random", "ff"])
def test_bitslice_model_equals_cm256_encode(oracle, fill):
    rs = np.random.RandomState(17)
    data = rs.randint(0, 256, size=(128, 508)).astype(np.uint8) if fill == "random" else np.full((128, 508), 0xFF, np.uint8)
    full = encode_model(data, 32)
    for R in range(1, 33):
        assert np.array_equal(full[:R], oracle.cm256_encode(data, R)), (fill, R)
