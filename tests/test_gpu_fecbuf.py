"""The FEC buffer bank (sdrhip_fecbuf) against one SDRdaemonFECBuffer per stream: the reference's own class
(oracle/_ref/libsdrref_fecbuf_hip.so) and the oracle's restatement (orc_fecbuffer), datagram by datagram."""
import ctypes as C

import numpy as np
import pytest

import test_ref_fecbuffer as tr

pytestmark = pytest.mark.gpu

INIT_META = bytes(11) + b"\xff" + bytes(8)  # MetaDataFEC::init()


class Model:
    """one SDRdaemonFECBuffer (the oracle's) plus what the bank reports beside the data: records, block 0, the two metas"""

    def __init__(self, oracle):
        self.b = oracle.fecbuffer()
        self.cur_meta = self.out_meta = INIT_META
        self.idx = []
        self.frames, self.block0, self.recs = [], [], []

    def _frame0(self):
        return bytes(self.b.s.frame)[:508]

    def feed(self, d):
        s = self.b.s
        fi = int(d[0]) | (int(d[1]) << 8)
        if s.frame_head != fi:
            b0 = self._frame0()
            orig = [i for i in self.idx if i < 128]
            dup = len(orig) != len(set(orig))
            fl = (1 if s.decoded else 0) | (2 if s.meta_retrieved else 0)
            if s.decoded and s.recovery_count > 0:
                fl |= 8 if dup else 4
            self.recs.append(dict(frame_index=s.frame_head, block_count=s.block_count, recovery_count=s.recovery_count, flags=fl))
            self.block0.append(np.frombuffer(b0, np.uint8).copy())
            if s.meta_retrieved and b0[:12] != self.out_meta[:12]:
                self.out_meta = b0[:20]
            self.idx = []
        if len(self.idx) < 128:
            self.idx.append(int(d[2]))
        o = self.b.write_and_read(d)
        if o is not None:
            self.frames.append(o)
        if s.block_count == 128 and s.meta_retrieved:
            b0 = self._frame0()
            if b0[:12] != self.cur_meta[:12]:
                self.cur_meta = b0[:20]
        return self

    def run(self, dgrams):
        for d in dgrams:
            self.feed(d)
        return self


def make_frames(oracle, rs, nframes, R, fi0=0):
    """nframes frames of 128 + R super blocks, random payload, frame indices fi0, fi0 + 1, ... (mod 2^16)"""
    out = []
    for f in range(nframes):
        fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
        fi = (fi0 + f) & 0xFFFF
        fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = fi & 0xFF, fi >> 8, np.arange(128), 0
        rec = oracle.frame_encode(fr, R) if R else np.zeros((0, 512), np.uint8)
        out.append(np.concatenate([fr, rec]))
    return out


def lossy(rs, blocks, nlost):
    keep = sorted(set(range(len(blocks))) - set(rs.choice(len(blocks), nlost, replace=False).tolist()))
    return [blocks[i] for i in keep]


def run_bank(bank, per_stream, cuts=None, device=True):
    """feeds every stream's datagrams; cuts: list of per-call datagram counts (the same for every stream); -> per stream
    (frames, block0, records)"""
    import torch

    S = len(per_stream)
    arrs = [np.asarray(p, np.uint8).reshape(-1, 512) for p in per_stream]
    if cuts is None:
        cuts = [max(a.shape[0] for a in arrs)]
    res = [([], [], []) for _ in range(S)]
    pos = [0] * S
    for n in cuts:
        chunk = []
        for s in range(S):
            c = arrs[s][pos[s]:pos[s] + n]
            pos[s] += c.shape[0]
            chunk.append(torch.from_numpy(c).cuda() if device else c)
        out = bank.write_and_read(chunk)
        for s in range(S):
            data, b0, recs = out[s]
            if device:
                data, b0 = data.cpu().numpy(), b0.cpu().numpy()
            res[s][0].extend(list(data))
            res[s][1].extend(list(b0))
            res[s][2].extend(recs)
    assert all(pos[s] == arrs[s].shape[0] for s in range(S)), "cuts do not cover the datagrams"
    return res


def check_against_model(bank, got, models, data=True):
    for s, m in enumerate(models):
        frames, b0, recs = got[s]
        assert recs == m.recs, (s, recs[:3], m.recs[:3])
        assert len(frames) == len(m.frames)
        if data:
            for k in range(len(frames)):
                assert np.array_equal(frames[k], m.frames[k]), (s, k, recs[k])
                assert np.array_equal(b0[k], m.block0[k]), (s, k, "block0")
        st = bank.stats(s)
        assert st["cur_nb_blocks"] == m.b.s.cur_nb_blocks and st["cur_nb_recovery"] == m.b.s.cur_nb_recovery, s
        assert st["min_nb_blocks"] == m.b.s.min_nb_blocks and st["max_nb_recovery"] == m.b.s.max_nb_recovery, s
        assert st["current_meta"][:20] == m.cur_meta and st["output_meta"][:20] == m.out_meta, s
        m.b.s.min_nb_blocks, m.b.s.max_nb_recovery = 256, 0  # (the getters reset them)


def counter(ctx):
    v = C.c_uint64()
    assert ctx.lib.sdrhip_ctx_get_counter(ctx.h, b"dec_rows_exceeded", C.byref(v)) == 0
    return v.value


@pytest.fixture
def ctx():
    import sdrdaemon_amd as sd

    assert sd.device_count() > 0
    c = sd.Context(0)
    c.set_option("dec_strict", 1)
    c.rows0 = counter(c)
    yield c
    assert counter(c) == c.rows0, "dec_rows_exceeded grew"


def _cuts(n, size, rs=None):
    out = []
    while sum(out) < n:
        out.append(size if size else int(rs.randint(0, 300)))
        if rs is not None and rs.rand() < 0.3:
            out.append(0)
    return out


@pytest.mark.parametrize("seed", [1, 4])
def test_reference_class_whole_and_cut(oracle, ctx, seed):
    import sdrdaemon_amd as sd

    L = tr._load("libsdrref_fecbuf_hip.so")
    _, dg = tr._datagrams(oracle, seed)
    ro, rstats, _ = tr._run_ref(L, dg)
    rs = np.random.RandomState(seed)
    for cuts in [None, _cuts(len(dg), 1), _cuts(len(dg), 7), _cuts(len(dg), 127), _cuts(len(dg), 128), _cuts(len(dg), 129),
                 _cuts(len(dg), 0, rs)]:
        m = Model(oracle).run(dg)
        bank = sd.FECBufferBank(ctx, 1)
        got = run_bank(bank, [dg], cuts)
        frames = got[0][0]
        assert len(frames) == len(ro) == 6
        for i in range(1, 6):
            assert np.array_equal(frames[i], ro[i]), (cuts[:4], i)
        assert [(r["block_count"], r["recovery_count"]) for r in got[0][2]][1:] == rstats[1:]
        check_against_model(bank, got, [m])


def _hostile(oracle, rs, R=32, fi0=0, nframes=8):
    """nframes frames (a multiple of 8), every eight of them the seven hostile patterns below"""
    assert nframes % 8 == 0
    frames = make_frames(oracle, rs, nframes, R, fi0)
    out = []
    for g in range(0, nframes, 8):
        fr = frames[g:g + 8]
        out += lossy(rs, fr[0], 20)                                  # plain
        f1 = lossy(rs, fr[1], 24)
        out += f1[:10] + f1[:10] + f1[10:]                            # identical duplicates among the first 128
        a, b = lossy(rs, fr[2], 10), lossy(rs, fr[3], 10)
        out += a[:60] + b[:30] + a[60:] + b[30:]                      # A B A interleaving
        f4 = lossy(rs, fr[4], 16)
        rs.shuffle(f4)
        out += f4                                                     # reordered inside the frame
        out += list(fr[5]) + list(fr[5][:40])                         # more than 128 arrivals
        f6 = [x for x in fr[6] if x[2] != 0]
        out += lossy(rs, f6, 20)                                      # block 0 lost (restored: no META)
        out += lossy(rs, fr[7], R + 20)[:100]                         # incomplete, with recovery blocks
    return out


@pytest.mark.parametrize("R", [1, 32, 33, 64, 127])
def test_hostile_sequences(oracle, ctx, R):
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(100 + R)
    dg = _hostile(oracle, rs, R, fi0=65531)  # (frame indices wrap from 65535 to 0)
    dg.append(np.full(512, 0xEE, np.uint8))
    m = Model(oracle).run(dg)
    bank = sd.FECBufferBank(ctx, 1)
    got = run_bank(bank, [dg], _cuts(len(dg), 0, rs))
    check_against_model(bank, got, [m])
    assert any(r["flags"] & sd.engine.FECBUF_DECODE_ERROR for r in got[0][2]) or R < 32
    # the same patterns three times over in ONE call: the classify pass walks them in chunks of 1024 datagrams
    rs = np.random.RandomState(200 + R)
    dg = _hostile(oracle, rs, R, fi0=65519, nframes=24)
    dg.append(np.full(512, 0xEE, np.uint8))
    assert len(dg) >= 2100
    m = Model(oracle).run(dg)
    bank = sd.FECBufferBank(ctx, 1)
    got = run_bank(bank, [dg])
    check_against_model(bank, got, [m])
    assert any(r["flags"] & sd.engine.FECBUF_DECODE_ERROR for r in got[0][2]) or R < 32


def test_advice_rows_above_32(oracle, ctx):
    """fecblk 64, recovery rows >= 32 among the first 128 and at most 32 recovery blocks in all"""
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(7)
    dg = []
    for fr in make_frames(oracle, rs, 6, 64):
        lost = set(rs.choice(128, 20, replace=False).tolist()) | set(range(128, 128 + 40))  # rows 0..39 lost
        dg += [fr[i] for i in range(192) if i not in lost]
    dg.append(np.full(512, 0xEE, np.uint8))
    m = Model(oracle).run(dg)
    bank = sd.FECBufferBank(ctx, 1)
    got = run_bank(bank, [dg])
    check_against_model(bank, got, [m])
    assert sum(1 for r in got[0][2] if r["flags"] & sd.engine.FECBUF_REPAIRED) == 6


def _bank64(oracle, seed, R, lose_rows):
    rs = np.random.RandomState(seed)
    per = []
    for s in range(64):
        nf = 0 if s % 13 == 5 else int(rs.randint(12, 24))
        dg = []
        fi0 = int(rs.randint(0, 65536))
        for fr in make_frames(oracle, rs, nf, R, fi0):
            lost = set(rs.choice(128, int(rs.randint(0, R // 2 + 1)), replace=False).tolist())
            if lose_rows:
                lost |= set(range(128, 128 + lose_rows))
            dg += [fr[i] for i in range(128 + R) if i not in lost]
        if nf:
            dg.append(np.full(512, 0xEE, np.uint8))
        per.append(dg)
    return rs, per


@pytest.mark.parametrize("R,lose_rows", [(32, 0), (64, 36)])
def test_64_streams(oracle, ctx, R, lose_rows):
    import sdrdaemon_amd as sd

    rs, per = _bank64(oracle, 11 + R, R, lose_rows)
    models = [Model(oracle).run(p) for p in per]
    assert sum(len(m.frames) for m in models) >= 1024
    bank = sd.FECBufferBank(ctx, 64)
    got = run_bank(bank, per, _cuts(max(len(p) for p in per), 0, rs) if lose_rows else None)
    check_against_model(bank, got, models)


def test_default_mode_delivers_a_superset(oracle):
    import sdrdaemon_amd as sd

    c = sd.Context(0)
    rows0 = counter(c)
    rs = np.random.RandomState(3)
    frames = make_frames(oracle, rs, 10, 32)
    dg = []
    for f, fr in enumerate(frames):
        blk = lossy(rs, fr, 24)
        if f % 2:  # recovery blocks first: the reference's copy-back leaves holes
            blk = [x for x in blk if x[2] >= 128] + [x for x in blk if x[2] < 128]
        dg += blk
    dg.append(np.full(512, 0xEE, np.uint8))
    m = Model(oracle).run(dg)
    bank = sd.FECBufferBank(c, 1)
    got = run_bank(bank, [dg])
    frames_got = got[0][0]
    assert len(frames_got) == len(m.frames) == 11
    for k in range(1, 11):
        exp = m.frames[k].reshape(127, 508)
        g = frames_got[k].reshape(127, 508)
        nz = exp.any(axis=1)
        assert np.array_equal(g[nz], exp[nz]), k
        assert np.array_equal(g, frames[k - 1][1:128, 4:]), k  # the original stream
    assert counter(c) == rows0


def test_host_and_device_memory_agree(oracle, ctx):
    import sdrdaemon_amd as sd

    rs, per = _bank64(oracle, 5, 32, 0)
    per = per[:8]
    cuts = _cuts(max(len(p) for p in per), 0, rs)
    a = run_bank(sd.FECBufferBank(ctx, 8), per, cuts, device=True)
    b = run_bank(sd.FECBufferBank(ctx, 8), per, cuts, device=False)
    for s in range(8):
        assert a[s][2] == b[s][2]
        assert len(a[s][0]) == len(b[s][0])
        for k in range(len(a[s][0])):
            assert np.array_equal(a[s][0][k], b[s][0][k]) and np.array_equal(a[s][1][k], b[s][1][k])


def test_reset_and_einval_retry(oracle, ctx):
    import torch

    import sdrdaemon_amd as sd

    rs = np.random.RandomState(9)
    dg = []
    for fr in make_frames(oracle, rs, 6, 32):
        dg += lossy(rs, fr, 10)
    dg.append(np.full(512, 0xEE, np.uint8))
    m = Model(oracle).run(dg)
    bank = sd.FECBufferBank(ctx, 1)
    run_bank(bank, [dg[:300]])
    bank.reset()
    got = run_bank(bank, [dg])  # after reset: a new bank
    check_against_model(bank, got, [m])
    bank.reset()
    m = Model(oracle).run(dg)
    first = run_bank(bank, [dg[:200]])
    x = torch.from_numpy(np.asarray(dg[200:], np.uint8)).cuda()
    with pytest.raises(sd.SdrHipError) as e:
        bank.write_and_read([x], max_frames=2)
    assert e.value.code == -1 and bank.last_n_frames == [len(m.frames) - len(first[0][0])]
    rest = bank.write_and_read([x])[0]
    frames = first[0][0] + list(rest[0].cpu().numpy())
    assert len(frames) == len(m.frames)
    for k in range(len(frames)):
        assert np.array_equal(frames[k], m.frames[k]), k
    assert first[0][2] + rest[2] == m.recs
