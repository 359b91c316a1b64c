"""The placement-directed datagram builder (tests/fecbuf_edges.py) and the two yardsticks on its sequences, without a GPU test.

Placement: from the headers alone, every event lies at the datagram position of the main call the builder was asked for -- this
is what keeps tests/test_gpu_fecbuf_edges.py from quietly testing something else after an edit, so nothing here skips.
Yardstick: every sequence, datagram by datagram, through the reference's own SDRdaemonFECBuffer (oracle/_ref/
libsdrref_fecbuf_hip.so) and through the oracle's restatement (test_gpu_fecbuf.Model): the released payloads and the
(block_count, recovery_count) pairs are equal, bar the initial slot.  The reference class decodes through the product's cm256.h
adapter, that is on a GPU: where there is none it runs without a decoder (m_cm256_OK false, SDRdaemonFECBuffer.cpp:42-49), the
frames the restatement repairs come out as received, and for those the comparison is: every row is the restatement's or a hole,
and the holes are as many as the originals that did not arrive.  With a device every frame is compared byte for byte."""
import numpy as np
import pytest

import fecbuf_edges as fe
import test_gpu_fecbuf as tg
import test_ref_fecbuffer as tr

CL = fe.CL
EDGES = (CL, 2 * CL)


def hdr(dg):
    dg = np.asarray(dg, np.uint8).reshape(-1, 512)
    return dg[:, 0].astype(int) | (dg[:, 1].astype(int) << 8), dg[:, 2].astype(int)


def seg(fi, pos):
    """(first, one past the last) position of the run of one frame index around pos"""
    a, b = pos, pos + 1
    while a > 0 and fi[a - 1] == fi[pos]:
        a -= 1
    while b < len(fi) and fi[b] == fi[pos]:
        b += 1
    return a, b


@pytest.fixture(scope="module")
def st(oracle):
    return fe.streams(oracle)


def events(st, kind):
    got = [(s, e) for s in st for e in s.events if e["kind"] == kind]
    assert got, kind
    return got


def test_bank_layout(st):
    assert st[0].name == "long" and sum(1 for s in st if not s.dg) == 1 and st[-1].dg
    off = np.cumsum([0] + [len(s.dg) for s in st])
    for s, o in zip(st[1:], off[1:]):
        assert o > 2 * CL and o % CL, (s.name, o)  # (packed: no later stream starts on a multiple of 1024 datagrams)
    for s in st:
        if s.dg:
            last = (s.dg + s.tail)[-1]
            assert bytes(last) == bytes([0xEE]) * 512 and len(s.tail) <= 1, s.name
            assert CL <= len(s.dg) <= 2500, s.name
    assert 20000 < off[-1] < 30000


def test_head_frames_and_carries(st):
    for s, e in events(st, "head"):
        fi, bi = hdr(s.dg)
        n = e["n_main"]
        assert seg(fi, 0) == (0, n) and fi[0] == e["fi"], s.name
        for c in fe.CARRIES:
            ca = s.carry(c)
            assert len(ca) == c
            if not c:
                continue
            cfi, cbi = hdr(ca)
            assert (cfi == e["fi"]).all() and cbi[0] == 0, (s.name, c)
            first = list(cbi) + list(bi[:n])
            first = first[:128]
            assert len(set(first)) == len(first), (s.name, c)                      # (no repeat among the first 128)
            assert len(first) < 128 or any(b >= 128 for b in first), (s.name, c)   # (a complete one has recovery blocks)
            assert 0 not in bi[:max(128 - c, 0)], (s.name, c)                       # (block 0 comes from the carry buffer)
    assert fe.CARRIES == (0, 37, 128 + 5)


def test_start_at_edge(st):
    seen = set()
    for s, e in events(st, "start"):
        fi, _ = hdr(s.dg)
        p = e["pos"]
        assert fi[p] != fi[p - 1] and fi[p - 1] == fi[p - 2] and fi[p + 1] == fi[p], (s.name, p)
        seen.add(p)
    assert seen == {B + d for B in EDGES for d in (-1, 0, 1)}


def test_rank_128_at_edge(st):
    seen = set()
    for s, e in events(st, "rank128"):
        fi, bi = hdr(s.dg)
        p = e["pos"]
        a, b = seg(fi, p)
        assert fi[p] == e["fi"] and a == p - 127, (s.name, p, a)                   # (the 128th arrival lies at p)
        under, past = bi[a:p + 1], bi[p + 1:b]
        assert len(set(under)) == 128 and (under[:127] < 128 + 32).all() and under[127] >= 128 + 32  # (rows >= 32: at p alone)
        assert (under[:127] >= 128).sum() >= 8 and len(past) >= 8 and (past >= 128).all()       # (recovery both sides of 128)
        assert (under >= 128 + 10).sum() == (under >= 128).sum()                                 # (the low rows are lost)
        k = (p + 1) // CL * CL if p % CL else p                                                  # the boundary
        assert k in EDGES and a < k < b and (bi[a:k] >= 128).any() and (bi[k:b] >= 128).any()
        seen.add(p)
    assert seen == {CL - 1, 2 * CL}


def test_dup_across_edge(st):
    under = set()
    for s, e in events(st, "dup"):
        fi, bi = hdr(s.dg)
        p, q = e["first"], e["second"]
        a, b = seg(fi, p)
        assert fi[p] == fi[q] == e["fi"] and a <= p < q < b, s.name
        assert bi[p] == bi[q] < 128 and p // CL + 1 == q // CL, s.name            # (the two copies lie in different chunks)
        assert bytes(s.dg[p][:4]) == bytes(s.dg[q][:4]) and bytes(s.dg[p]) != bytes(s.dg[q])    # (which copy won shows)
        first = bi[a:a + 128]
        assert (first >= 128).any() and p - a < 128 and (q - a < 128) == e["under"], s.name
        others = [x for i, x in enumerate(bi[a:min(b, a + 128)]) if a + i != q]
        assert len(set(others)) == len(others), s.name                              # (no other repeat among the first 128)
        if not e["under"]:
            k = q // CL * CL
            assert (bi[a:k] >= 128).any() and (bi[k:a + 128] >= 128).any(), s.name  # (recovery rows both sides, below rank 128)
        under.add(e["under"])
    assert under == {True, False}


def test_block0_across_edge(st):
    for s, e in events(st, "block0") + events(st, "block0_same"):
        fi, bi = hdr(s.dg)
        p, r = e["pos"], e["released"]
        a, b = seg(fi, p)
        assert fi[p] == e["fi"] and bi[p] == 0 and b == r and p // CL + 1 == r // CL, s.name  # (released one chunk later)
        assert list(np.flatnonzero(bi[a:b] == 0) + a) == [p] and b - a >= 128, s.name
        prev = seg(fi, a - 1)
        p0 = [i for i in range(prev[0], min(prev[1], prev[0] + 128)) if bi[i] == 0]
        assert len(p0) == 1, s.name                                                  # (the frame in front has a META too)
        mine, before = bytes(s.dg[p][4:24]), bytes(s.dg[p0[0]][4:24])
        if e["kind"] == "block0":
            assert mine[:12] != before[:12], s.name
        else:
            assert mine[:12] == before[:12] and mine[12:] != before[12:], s.name
            assert fi[r] == 0xEEEE or s.tail, s.name                                 # (the stream's last META: the metas stay)
    for s, e in events(st, "block0"):
        assert hdr(s.dg)[0][e["released"]] == 0xEEEE                                 # (the stream's last META: the metas change)
    for s, e in events(st, "block0_twice"):
        fi, bi = hdr(s.dg)
        p, q = e["first"], e["second"]
        a, b = seg(fi, p)
        assert fi[p] == fi[q] == e["fi"] and bi[p] == bi[q] == 0 and p // CL + 1 == q // CL and q - a < 128 and q < b, s.name
        assert list(np.flatnonzero(bi[a:b] == 0) + a) == [p, q] and bytes(s.dg[p][4:]) != bytes(s.dg[q][4:]), s.name
    for s, e in events(st, "block0_late"):
        fi, bi = hdr(s.dg)
        p = e["pos"]
        a, b = seg(fi, p)
        assert fi[p] == e["fi"] and list(np.flatnonzero(bi[a:b] == 0) + a) == [p] and p - a >= 128, s.name
        assert len(set(bi[a:a + 128])) == 128 and a // CL + 1 == p // CL, s.name     # (decodable; the block 0 one chunk on)


def test_long_frame(st):
    (s, e), = events(st, "long")
    fi, bi = hdr(s.dg)
    assert seg(fi, 0) == (0, e["n"]) and e["n"] > 2 * CL + 128                       # (chunk 1: no frame start at all)
    assert len(set(bi[:128])) == 128 and (bi[:128] >= 128).any() and (bi[:128] < 128).any()
    assert len(set(bi[128:e["n"]])) > 100                                            # (repeats of its own blocks behind)


def test_one_datagram_frames(st):
    (s, e), = events(st, "singles")
    fi, bi = hdr(s.dg)
    p, n = e["pos"], e["n"]
    assert p == CL and n == 1030 and fi[p - 1] != fi[p]
    run = fi[p:p + n + 1]
    assert (np.diff(run[:n]) % 65536 == 1).all() and run[n] != run[n - 1]            # (every datagram opens a frame)
    assert 65535 in run[:n] and 0 in run[:n]                                         # (through the wrap)
    assert {0, 5, 131} <= set(bi[p:p + n])


def test_aba_at_edge(st):
    seen = set()
    for s, e in events(st, "aba"):
        fi, bi = hdr(s.dg)
        B = e["pos"]
        assert fi[B - 2] == fi[B] == e["fi"] != fi[B - 1] and fi[B + 1] == e["fi"], s.name
        assert seg(fi, B - 2) == (B - 1 - e["n_first"], B - 1) and fi[B - 1] != fi[B - 2 - e["n_first"]], s.name
        seen.add((B, e["n_first"] >= 128))
    assert seen == {(CL, False), (2 * CL, True)}


def test_exact_lengths(st):
    seen = {}
    for s, e in events(st, "exact"):
        fi, _ = hdr(s.dg)
        assert len(s.dg) == e["n"] and len(s.tail) == 1, s.name
        a, b = seg(fi, e["n"] - 1)
        assert b == e["n"] and b - a == e["last"] and fi[-1] == e["fi"], s.name
        seen[e["n"]] = e["last"]
    assert sorted(seen) == [CL, CL + 1, 2 * CL] and max(seen.values()) >= 128 and seen[CL + 1] == 1


@pytest.fixture(scope="module")
def reference(oracle):
    """(the compiled reference class, whether it has a decoder).  torch brings its device runtime up before the reference's
    library is first used (the order test_gpu_rx_datagrams.torch_first keeps)"""
    import torch

    gpu = torch.cuda.is_available()
    if gpu:
        torch.zeros(1).cuda()
    return tr._load("libsdrref_fecbuf_hip.so"), gpu


@pytest.mark.parametrize("carry", fe.CARRIES)
def test_yardsticks_agree(oracle, st, reference, carry):
    L, decoder = reference
    repaired = errors = 0
    for s, seq in zip(st, fe.sequences(oracle, carry)):
        m = tg.Model(oracle).run(list(seq))
        ro, rstats, _ = tr._run_ref(L, list(seq))
        assert len(ro) == len(m.frames) == len(m.recs), s.name
        assert rstats[1:] == [(r["block_count"], r["recovery_count"]) for r in m.recs][1:], s.name
        for k in range(1, len(ro)):
            r = m.recs[k]
            if decoder or not r["flags"] & 4:
                assert np.array_equal(ro[k], m.frames[k]), (s.name, k, r)
            else:
                got, exp = ro[k].reshape(127, 508), m.frames[k].reshape(127, 508)
                hole = ~got.any(axis=1)
                assert np.array_equal(got[~hole], exp[~hole]), (s.name, k, r)
                assert int(hole.sum()) == r["recovery_count"] - (0 if r["flags"] & 2 else 1), (s.name, k, r)
            repaired += 1 if r["flags"] & 4 else 0
            errors += 1 if r["flags"] & 8 else 0
        if s.name == "long":
            assert any(r["block_count"] > 2 * CL and r["flags"] & 4 for r in m.recs)
        if s.name == "singles":
            assert len(m.recs) >= 1030
    assert repaired >= 20 and errors >= 2


@pytest.mark.parametrize("carry", fe.CARRIES)
def test_the_events_happen_in_the_restatement(oracle, carry):
    """what the GPU tests assert of the records they get back (fecbuf_edges.check_events) holds for the restatement's"""
    ms, counts = fe.models(oracle, carry)
    fe.check_events(oracle, [m.recs for m in ms], counts, lambda s: dict(output_meta=ms[s].out_meta, current_meta=ms[s].cur_meta))


@pytest.mark.parametrize("S", fe.TABLE_SIZES)
def test_table_calls(oracle, reference, S):
    """the small banks' two calls (fecbuf_edges.table_calls): what the GPU tests assert of their records holds for the
    restatement's, and the reference class releases the restatement's frames"""
    L, decoder = reference
    calls = fe.table_calls(oracle, S)
    assert len(calls) == 2 and len(calls[0]) == len(calls[1]) == S
    assert [len(c) for c in calls[0]] == [0 if s == 1 else 136 for s in range(S)]
    assert [len(c) for c in calls[1]] == [264 if s == 1 else 128 for s in range(S)]
    ms, counts = fe.models_of(oracle, calls)
    fe.check_table_events([m.recs for m in ms], counts)
    for s, m in enumerate(ms):
        ro, rstats, _ = tr._run_ref(L, list(np.concatenate([c[s] for c in calls])))
        assert rstats[1:] == [(r["block_count"], r["recovery_count"]) for r in m.recs][1:], s
        assert np.array_equal(ro[2], m.frames[2]), s
        if decoder:
            assert np.array_equal(ro[1], m.frames[1]), s
