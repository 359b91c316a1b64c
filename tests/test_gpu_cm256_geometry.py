"""sdrhip_cm256_encode / sdrhip_cm256_decode (the generic "any geometry the library accepts" entry points behind the cm256.h adapter)
at the edges of the kernel that serves them, against TWO references: the oracle (the C restatement of upstream) and the
from-the-specification CM256 of tests/cm256_spec.py (bit-serial field, Gauss-Jordan), which share no code.  Byte for byte.

What the edges are (gf_kernels.hip, sdrhip_fec.cpp): launch_gf_apply picks gf_apply_kernel<4> for rows <= 16, <6> for rows <= 24, <8>
with gridDim.y = ceil(rows / 32) above; wave w of a workgroup owns rows w * RB .. w * RB + RB - 1 and leaves when it has none; the
coefficient tile is zero-filled beyond the matrix; a block is cut into 508-byte slabs that ride as frames, two per wave (an odd slab
count leaves a half-wave without a frame), the last lane of a slab carries 12 bytes, not 16; cols = OriginalCount goes up to 255 against
an LDS pitch of 256.  rows = RecoveryCount when encoding and = the number of erasures when decoding."""
import ctypes as C

import numpy as np
import pytest

import cm256_spec
import oracle_lib
import signals
from cm256_spec import GEOMETRIES, arrival, pick

pytestmark = pytest.mark.gpu

GUARD = (np.arange(64) * 37 + 11).astype(np.uint8)  # behind the recovery buffer of every encode
ROW_GUARD = 16                                      # behind every block of the strided decodes


@pytest.fixture(scope="module")
def ctx():
    import sdrdaemon_amd as sd

    assert sd.device_count() > 0
    return sd.Context(0)


@pytest.fixture(scope="module")
def cm(ctx):
    import sdrdaemon_amd as sd

    return sd.CM256(ctx)


@pytest.fixture(scope="module")
def spec():
    return cm256_spec.field()


# ---------------------------------------------------------------------------------------------------------------------- encode
def _encode(cm, x, m):
    """through sd.CM256 into a buffer with the guard behind it: whatever the buffer held is overwritten, the guard comes back"""
    k, bb = x.shape
    buf = np.concatenate([np.full(m * bb, 0xA5, np.uint8), GUARD])
    before = x.copy()
    rc, rec = cm.cm256_encode((k, m, bb), x, recovery_out=buf[: m * bb].reshape(m, bb))
    assert rc == 0, (k, m, bb, rc)
    assert np.array_equal(buf[m * bb:], GUARD), (k, m, bb, "bytes written behind the recovery blocks")
    assert np.array_equal(x, before), (k, m, bb, "originals modified")
    return rec


def _check_encode(cm, oracle, spec, x, m):
    k, bb = x.shape
    got = _encode(cm, x, m)
    for name, exp in (("oracle", oracle.cm256_encode(x, m)), ("specification", cm256_spec._encode(spec, x, m))):
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (k, m, bb, name, "first wrong (row, byte):", bad[0].tolist(), "wrong rows:", sorted(set(bad[:, 0].tolist())))


# row counts on both sides of every dispatch (16 | 17, 24 | 25), wave (RB = 4: 4 | 5, 6: 18 | 19, 8: 32 | 33) and workgroup
# (32 | 33, 64 | 65) boundary; k + m = 256 from every side; the smallest and the widest (255 against the LDS pitch of 256) matrices
ENC_ROWS = [(100, m) for m in (1, 3, 4, 5, 16, 17, 18, 19, 24, 25, 31, 32, 33, 64, 65)] \
    + [(2, 254), (191, 65), (255, 1), (129, 127), (127, 129)] + [(k, 8) for k in (2, 3, 127, 129)]


@pytest.mark.parametrize("k,m", ENC_ROWS, ids=["%d+%d" % g for g in ENC_ROWS])
def test_encode_row_counts(cm, oracle, spec, k, m):
    # 1021 bytes = three slabs (the second wave's upper half has no frame), the last of 5 bytes
    x = np.random.RandomState(1000 * k + m).randint(0, 256, size=(k, 1021)).astype(np.uint8)
    _check_encode(cm, oracle, spec, x, m)


# slab counts 1 .. 5, tails of 1, 2, 3, 4 (below and at one dword), 5, 15, 16, 17 (around one lane), 507, 508 (the 12-byte lane) bytes
ENC_BB = (1, 2, 3, 4, 5, 15, 16, 17, 507, 508, 509, 1015, 1016, 1017, 1524, 2033)


@pytest.mark.parametrize("bb", ENC_BB)
@pytest.mark.parametrize("k,m", [(10, 4), (100, 33)], ids=["10+4", "100+33"])
def test_encode_block_sizes(cm, oracle, spec, k, m, bb):
    x = np.random.RandomState(77 * bb + k).randint(0, 256, size=(k, bb)).astype(np.uint8)
    _check_encode(cm, oracle, spec, x, m)


def _every_value_everywhere(k, bb):
    """every byte value in every column class: the multiplier splits a byte into 3 + 3 + 2 bits and looks each part up in a table of
    its own, a lane owns bytes 16 l .. 16 l + 15 of a slab (lane 31: twelve).  Class = byte position inside the lane's sixteen."""
    j, c = np.meshgrid(np.arange(k), np.arange(bb), indexing="ij")
    cs = c % 508
    x = ((cs // 16) + 31 * j + 7 * (cs % 16)).astype(np.uint8)
    for b in range(16):
        assert len(np.unique(x[:, (cs[0] % 16) == b])) == 256, b
    return x


@pytest.mark.parametrize("fill", ["zero", "ff", "every_value"])
@pytest.mark.parametrize("k,m", [(10, 4), (100, 33)], ids=["10+4", "100+33"])
def test_encode_fills(cm, oracle, spec, k, m, fill):
    bb = 1021
    x = {"zero": lambda: np.zeros((k, bb), np.uint8), "ff": lambda: np.full((k, bb), 0xFF, np.uint8),
         "every_value": lambda: _every_value_everywhere(k, bb)}[fill]()
    _check_encode(cm, oracle, spec, x, m)


@pytest.mark.parametrize("m", [1, 5, 255])
def test_encode_one_original_gives_copies(cm, oracle, m):
    x = np.random.RandomState(m).randint(0, 256, size=(1, 509)).astype(np.uint8)
    got = _encode(cm, x, m)
    assert np.array_equal(got, np.repeat(x, m, axis=0))
    assert np.array_equal(got, oracle.cm256_encode(x, m))


# ---------------------------------------------------------------------------------------------------------------------- decode
def _delivery(oracle, rs, k, m, bb, erased, rows, mode):
    """-> originals, received blocks and their block numbers in arrival order (the oracle encodes: the specification solving its
    blocks below is a cross check of its own)"""
    x = rs.randint(0, 256, size=(k, bb)).astype(np.uint8)
    allb = np.concatenate([x, oracle.cm256_encode(x, m)])
    idx = arrival(rs, k, erased, rows, mode)
    return x, np.ascontiguousarray(allb[idx]), idx


def _check_in_place(k, data, idx, d1, j1, gives_back=True):
    """cm256_decode's contract: received originals stay as they are, every recovery descriptor ends holding an erased original"""
    for p in range(k):
        if idx[p] < k:
            assert j1[p] == idx[p] and np.array_equal(d1[p], data[p]), ("received original touched", p)
        else:
            assert j1[p] < k, ("recovery descriptor not rewritten", p)
    if gives_back:
        assert sorted(j1.tolist()) == list(range(k))


def _check_decode(cm, oracle, spec, x, data, idx, m, gives_back=True):
    k, bb = x.shape
    d1, d2 = data.copy(), data.copy()
    rc1, j1 = cm.cm256_decode((k, m, bb), d1, idx)
    rc2, j2 = oracle.cm256_decode(d2, idx, k, m)
    assert rc1 == rc2 == 0, (rc1, rc2)
    assert np.array_equal(j1, j2), "Index fields differ from the oracle's"
    bad = np.argwhere(d1 != d2)
    assert bad.size == 0, (k, m, bb, "first wrong (descriptor, byte):", bad[0].tolist(), "wrong descriptors:", sorted(set(bad[:, 0].tolist())))
    _check_in_place(k, data, idx, d1, j1, gives_back)
    if gives_back:
        out = np.zeros_like(x)
        out[j1] = d1
        assert np.array_equal(out, x), "scattered by Index, the blocks are not the originals"
        assert np.array_equal(cm256_spec._solve(spec, k, idx.tolist(), data), x), "the specification does not decode this delivery"
    return d1, j1


@pytest.mark.parametrize("wide", [0, 1], ids=["bb508", "bb_other"])
@pytest.mark.parametrize("g", range(len(GEOMETRIES)), ids=["%d+%d_lose%d" % g for g in GEOMETRIES])
def test_decode_geometries(cm, oracle, spec, g, wide):
    """the 19 geometries at one whole slab and at one of 3 (below a dword), 509 (one byte into a second slab), 1400 (three slabs)
    bytes; each geometry once with the recovery blocks last and once fully shuffled; blocks 0 and k - 1 erased in every other one"""
    k, m, n = GEOMETRIES[g]
    bb = (3, 509, 1400)[g % 3] if wide else 508
    rs = np.random.RandomState(5000 + 10 * g + wide)
    erased, rows = pick(rs, k, m, n, include=(0, k - 1) if n >= 2 and g % 2 == 0 else ())
    x, data, idx = _delivery(oracle, rs, k, m, bb, erased, rows, "shuffled" if (g + wide) % 2 == 0 else "recovery_last")
    _check_decode(cm, oracle, spec, x, data, idx, m)


# erasure counts = kernel rows at the dispatch and workgroup boundaries (one recovery block with RecoveryCount = 40 is NOT upstream's
# DecodeM1 shortcut: its row is honoured); every original lost: the coefficient rows are the inverse of a whole Cauchy block
DEC_COUNTS = [(100, 40, n) for n in (1, 16, 17, 24, 25, 32, 33, 40)] + [(20, 20, 20), (33, 40, 33)]


@pytest.mark.parametrize("mode", ["recovery_last", "shuffled"])
@pytest.mark.parametrize("k,m,n", DEC_COUNTS, ids=["%d+%d_lose%d" % g for g in DEC_COUNTS])
def test_decode_erasure_counts(cm, oracle, spec, k, m, n, mode):
    rs = np.random.RandomState(100 * n + k + len(mode))
    erased, rows = pick(rs, k, m, n, include=(0, k - 1) if n >= 2 else ())
    if n == 1:
        rows = [int(rs.randint(1, m))]  # not the parity row
    x, data, idx = _delivery(oracle, rs, k, m, 509, erased, rows, mode)
    _check_decode(cm, oracle, spec, x, data, idx, m)


def _blocks(cls, base, stride, idx):
    b = (cls * len(idx))()
    for i in range(len(idx)):
        b[i].Block = base + i * stride
        b[i].Index = int(idx[i])
    return b


@pytest.mark.parametrize("k,m,n,bb", [(5, 3, 2, 3), (17, 17, 17, 508), (100, 40, 33, 509), (200, 56, 56, 1400)])
def test_decode_in_place_with_strided_rows(ctx, oracle, spec, k, m, n, bb):
    """the descriptors point into rows bb + 16 bytes apart: the 16 bytes behind every block keep their pattern, received originals
    keep bytes and Index, every recovery descriptor ends holding the erased original its new Index names"""
    from sdrdaemon_amd import _lib

    rs = np.random.RandomState(k + n)
    erased, rows = pick(rs, k, m, n, include=(0, k - 1))
    x, data, idx = _delivery(oracle, rs, k, m, bb, erased, rows, "shuffled")
    buf = np.empty((k, bb + ROW_GUARD), np.uint8)
    buf[:, :bb] = data
    buf[:, bb:] = rs.randint(0, 256, size=(k, ROW_GUARD))
    guard = buf[:, bb:].copy()
    blocks = _blocks(_lib.CM256Block, buf.ctypes.data, bb + ROW_GUARD, idx)
    assert ctx.lib.sdrhip_cm256_decode(ctx.h, _lib.CM256Params(k, m, bb), blocks) == 0
    assert np.array_equal(buf[:, bb:], guard), "bytes behind a block modified"
    assert [blocks[i].Block for i in range(k)] == [buf.ctypes.data + i * (bb + ROW_GUARD) for i in range(k)]
    j1 = np.array([blocks[i].Index for i in range(k)], np.uint8)
    d2 = data.copy()
    rc2, j2 = oracle.cm256_decode(d2, idx, k, m)
    assert rc2 == 0 and np.array_equal(j1, j2) and np.array_equal(buf[:, :bb], d2)
    _check_in_place(k, data, idx, buf[:, :bb], j1)
    for p in range(k):
        assert np.array_equal(buf[p, :bb], x[j1[p]]), p


@pytest.mark.parametrize("row", [0, 2], ids=["parity_row", "row_k_plus_2"])
@pytest.mark.parametrize("k", [10, 200])
def test_decode_recovery_count_one(cm, oracle, spec, k, row):
    """RecoveryCount = 1 is upstream's DecodeM1: XOR of everything received, whatever the recovery block's row.  With row k that is
    the original; with row k + 2 it is not, and the bytes are upstream's all the same (the one delivery excused from decoding)."""
    rs = np.random.RandomState(31 * k + row)
    lost = int(rs.randint(k))
    x, data, idx = _delivery(oracle, rs, k, row + 1, 509, [lost], [row], "shuffled")
    d1, j1 = _check_decode(cm, oracle, spec, x, data, idx, 1, gives_back=(row == 0))
    p = int(np.nonzero(idx >= k)[0][0])
    assert j1[p] == lost and np.array_equal(d1[p], np.bitwise_xor.reduce(data, axis=0))


def test_decode_one_original(cm, oracle):
    """k = 1: every block is the original; Index becomes 0, the data is not touched"""
    x = np.random.RandomState(1).randint(0, 256, size=(1, 509)).astype(np.uint8)
    for first in (0, 3):
        d1, d2 = x.copy(), x.copy()
        rc1, j1 = cm.cm256_decode((1, 5, 509), d1, [first])
        rc2, j2 = oracle.cm256_decode(d2, [first], 1, 5)
        assert rc1 == rc2 == 0 and j1.tolist() == j2.tolist() == [0]
        assert np.array_equal(d1, x) and np.array_equal(d2, x)


def test_decode_without_erasures_touches_nothing(cm, oracle):
    rs = np.random.RandomState(7)
    x, data, idx = _delivery(oracle, rs, 7, 3, 509, [], [], "shuffled")
    d1 = data.copy()
    rc, j1 = cm.cm256_decode((7, 3, 509), d1, idx)
    assert rc == 0 and np.array_equal(j1, idx) and np.array_equal(d1, data)
    d2 = data.copy()
    rc2, j2 = oracle.cm256_decode(d2, idx, 7, 3)
    assert rc2 == 0 and np.array_equal(j2, idx) and np.array_equal(d2, data)


# ---------------------------------------------------------------------------------------------------------------------- errors
def _valid_calls_still_work(cm, oracle):
    rs = np.random.RandomState(99)
    x = rs.randint(0, 256, size=(5, 33)).astype(np.uint8)
    rec = _encode(cm, x, 3)
    assert np.array_equal(rec, oracle.cm256_encode(x, 3))
    idx = np.array([4, 6, 1, 5, 2])  # 0 and 3 lost, recovery rows 1 and 0
    data = np.concatenate([x, rec])[idx].copy()
    rc, j = cm.cm256_decode((5, 3, 33), data, idx)
    assert rc == 0
    out = np.zeros_like(x)
    out[j] = data
    assert np.array_equal(out, x)


BAD_PARAMS = [((0, 4, 8), -1), ((4, 0, 8), -1), ((4, 4, 0), -1), ((-1, 4, 8), -1), ((4, -2, 8), -1), ((4, 4, -8), -1), ((200, 57, 8), -2)]


# (upstream checks the parameters before the pointers: the last case)
ENC_ERRORS = [(p, "", w) for p, w in BAD_PARAMS] + [((4, 4, 8), "originals", -3), ((4, 4, 8), "recovery", -3), ((0, 4, 8), "originals", -1)]


@pytest.mark.parametrize("params,null,want", ENC_ERRORS, ids=["x".join(map(str, p)) + ("_null_" + n if n else "") for p, n, _ in ENC_ERRORS])
def test_encode_errors(ctx, cm, oracle, params, null, want):
    from sdrdaemon_amd import _lib

    rows = max(params[0], 4)
    x = np.random.RandomState(3).randint(0, 256, size=(rows, 8)).astype(np.uint8)
    rec = np.full(256 * 8, 0x5A, np.uint8)
    x0, rec0 = x.copy(), rec.copy()
    rcs = []
    for lib, mod, head in ((ctx.lib.sdrhip_cm256_encode, _lib, (ctx.h,)), (oracle.lib.orc_cm256_encode, oracle_lib, ())):
        blocks = None if null == "originals" else _blocks(mod.CM256Block, x.ctypes.data, 8, np.arange(rows))
        rcs.append(lib(*head, mod.CM256Params(*params), blocks, C.c_void_p(0 if null == "recovery" else rec.ctypes.data)))
        assert np.array_equal(x, x0) and np.array_equal(rec, rec0), "an error return modified the caller's data"
    assert rcs == [want, want], rcs
    _valid_calls_still_work(cm, oracle)


def _decode_error(ctx, oracle, params, data, idx, null=False, with_oracle=True):
    from sdrdaemon_amd import _lib

    d0 = data.copy()
    rcs = []
    for lib, mod, head in ((ctx.lib.sdrhip_cm256_decode, _lib, (ctx.h,)), (oracle.lib.orc_cm256_decode, oracle_lib, ()))[: 2 if with_oracle else 1]:
        blocks = _blocks(mod.CM256Block, data.ctypes.data, data.shape[1], idx)
        rcs.append(lib(*head, mod.CM256Params(*params), None if null else blocks))
        assert np.array_equal(data, d0), "an error return modified the caller's blocks"
        assert [blocks[i].Index for i in range(len(idx))] == [int(i) for i in idx], "an error return modified the Index fields"
        assert [blocks[i].Block for i in range(len(idx))] == [data.ctypes.data + i * data.shape[1] for i in range(len(idx))]
    return rcs


@pytest.mark.parametrize("params,want", BAD_PARAMS, ids=["x".join(map(str, p)) for p, _ in BAD_PARAMS])
def test_decode_bad_parameters(ctx, cm, oracle, params, want):
    rows = max(params[0], 4)
    data = np.random.RandomState(4).randint(0, 256, size=(rows, 8)).astype(np.uint8)
    assert _decode_error(ctx, oracle, params, data, np.arange(rows)) == [want, want]
    _valid_calls_still_work(cm, oracle)


def test_decode_null_blocks(ctx, cm, oracle):
    data = np.zeros((4, 8), np.uint8)
    assert _decode_error(ctx, oracle, (4, 4, 8), data, np.arange(4), null=True) == [-3, -3]
    _valid_calls_still_work(cm, oracle)


def test_decode_duplicate_original(ctx, cm, oracle):
    rs = np.random.RandomState(6)
    data = rs.randint(0, 256, size=(10, 509)).astype(np.uint8)
    idx = np.arange(10)
    idx[7] = 2    # original 2 twice
    idx[9] = 11   # and a recovery block, so that there is something to decode
    assert _decode_error(ctx, oracle, (10, 4, 509), data, idx) == [-5, -5]
    _valid_calls_still_work(cm, oracle)


def test_decode_same_recovery_row_twice(ctx, cm, oracle):
    """Two descriptors with the same recovery row make the system singular.  The product plans before it touches anything and
    returns SDRHIP_EDECODE with the caller's data as it was.  (Not compared with the oracle: upstream does not detect this and
    writes garbage; the oracle's elimination fails with -6 after it has modified the recovery blocks.)"""
    rs = np.random.RandomState(8)
    x = rs.randint(0, 256, size=(10, 509)).astype(np.uint8)
    allb = np.concatenate([x, oracle.cm256_encode(x, 4)])
    idx = np.array([5, 13, 0, 9, 2, 13, 7, 3, 8, 1])  # 4 and 6 lost, recovery row 3 twice
    data = allb[idx].copy()
    assert _decode_error(ctx, oracle, (10, 4, 509), data, idx, with_oracle=False) == [-5]
    _valid_calls_still_work(cm, oracle)


# ---------------------------------------------------------------------------------------------------------------------- shared staging
def test_generic_and_batched_calls_share_one_context(ctx, cm, oracle, spec):
    """The generic calls and the batched frame calls stage through the same device buffers of their context (in, out, aux).
    Interleaved on one context, every one of them gives what it gives alone on a fresh context."""
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(2025)
    # generic decode at (200, 56, 1400), generic encode at (5, 3, 33)
    k, m, bb = 200, 56, 1400
    erased, rows = pick(rs, k, m, 56, include=(0, k - 1))
    xd, data, idx = _delivery(oracle, rs, k, m, bb, erased, rows, "shuffled")
    xe = rs.randint(0, 256, size=(5, 33)).astype(np.uint8)
    # batched: 5 frames, R = 32, 24 erasures each (one pattern per frame)
    F, R = 5, 32
    iq = signals.noise(F * 16129, 314)
    frames = oracle.framer(nb_fec_blocks=R, tv_sec=7, tv_usec=8).write(iq)
    exp_rec = np.stack([oracle.frame_encode(frames[f], R) for f in range(F)])
    rx = np.zeros((F, 128, 512), np.uint8)
    for f in range(F):
        lost = set(pick(rs, 128, R, 24, include=(0,) if f == 1 else ())[0])
        rx[f] = np.concatenate([frames[f], exp_rec[f]])[[i for i in range(160) if i not in lost][:128]]

    def generic_decode(c):
        d = data.copy()
        rc, j = sd.CM256(c).cm256_decode((k, m, bb), d, idx)
        assert rc == 0
        return d, j

    def generic_encode(c):
        return _encode(sd.CM256(c), xe, 3)

    def batched(c):
        rec = sd.fec_encode_frames(c, frames, R)
        payload, b0 = sd.fec_decode_frames(c, rx, want_block0=True)
        return rec, payload, b0

    def batched_dense(c):
        c.set_option("dec_path", "dense")
        try:
            return batched(c)
        finally:
            c.set_option("dec_path", "syndrome")

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))

    alone = {}
    for name, fn in (("decode", generic_decode), ("encode", generic_encode), ("batched", batched), ("dense", batched_dense)):
        fresh = sd.Context(0)
        try:
            alone[name] = fn(fresh)
        finally:
            fresh.close()
    # alone, they are right
    out = np.zeros_like(xd)
    out[alone["decode"][1]] = alone["decode"][0]
    assert np.array_equal(out, xd)
    assert np.array_equal(alone["encode"], oracle.cm256_encode(xe, 3))
    for name in ("batched", "dense"):
        rec, payload, b0 = alone[name]
        assert np.array_equal(rec, exp_rec), name
        for f in range(F):
            assert np.array_equal(payload[f].view(np.int16).reshape(-1, 2), iq[f * 16129:(f + 1) * 16129]), (name, f)
            assert np.array_equal(b0[f], frames[f, 0, 4:]), (name, f)
    # together, they are the same
    assert same(generic_decode(ctx), alone["decode"]), "generic decode"
    assert same(batched(ctx), alone["batched"]), "batched calls after a generic decode"
    assert np.array_equal(generic_encode(ctx), alone["encode"]), "generic encode after the batched calls"
    assert same(batched(ctx), alone["batched"]), "batched calls after a generic encode"
    assert same(batched_dense(ctx), alone["dense"]), "batched calls through the dense decoder"
    assert same(generic_decode(ctx), alone["decode"]), "generic decode after the batched calls"
