"""Datagram sequences that put a named event of the FEC buffer's classify rule at a named datagram position of one call.

The classify kernel (sdrdaemon_amd/csrc/fecbuf_passes.h) walks a stream's datagrams of one call in chunks of CL = 1024 and hands
the frame open at a chunk's end to the next chunk; the host's shadow (fecbuf_shadow_run) restates the rule datagram by datagram.
Positions here count from the first datagram of the MAIN call, as the kernel's chunks do.  A Stream builds the main call by
filling in front of every event with ordinary lossy frames (test_gpu_fecbuf.make_frames, trimmed by dropping originals and
recovery blocks); carry(c) gives c more datagrams of the main call's first frame for a call in front of it, so that the main call
starts with that frame open in the carry buffer and no position in it moves; tail is a last call (the 0xEE datagram of the
streams whose main call has an exact length).  Every event is recorded in Stream.events for tests/test_fecbuf_edges_model.py,
which asserts from the headers alone that it lies where it was asked to lie."""
import numpy as np

import test_gpu_fecbuf as tg

CL = 1024                # datagrams per classify chunk
CARRIES = (0, 37, 133)   # datagrams of the first frame in a call of their own, in front of the main call
RUN = 1030               # the run of one-datagram frames
LONG = 2300              # the long frame's datagrams in the main call
META, REPAIRED, ERROR = 2, 4, 8  # sdrhip_fecbuf_frame.flags: FECBUF_META, FECBUF_REPAIRED, FECBUF_DECODE_ERROR
NRES = 37                # blocks of the first frame kept out of the main call's first 128 (block 0 among them): the carry's


def ee():
    return np.full(512, 0xEE, np.uint8)


def altered(d):
    """the same header, another payload"""
    d = d.copy()
    d[4:] ^= 0x5A
    return d


class Stream:
    def __init__(self, oracle, name, seed, fi0, flen=136):
        self.o, self.name, self.rs, self.fi, self.flen = oracle, name, np.random.RandomState(seed), fi0, flen
        self.dg, self.tail, self.events = [], [], []
        self._head = None

    # ---- frames
    def frame(self, R=32, b0_prefix=None):
        """(frame index, the 128 + R super blocks) of the next frame index; b0_prefix: the first bytes of block 0's payload"""
        fi, self.fi = self.fi, (self.fi + 1) & 0xFFFF
        if b0_prefix is None:
            return fi, tg.make_frames(self.o, self.rs, 1, R, fi)[0]
        fr = self.rs.randint(0, 256, (128, 512)).astype(np.uint8)
        fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = fi & 0xFF, fi >> 8, np.arange(128), 0
        fr[0, 4:4 + len(b0_prefix)] = np.frombuffer(bytes(b0_prefix), np.uint8)
        return fi, np.concatenate([fr, self.o.frame_encode(fr, R)])

    def lose(self, n, lo=1):
        """the originals lo .. 127 but n of them, ascending"""
        lost = set(self.rs.choice(np.arange(lo, 128), n, replace=False).tolist())
        return [i for i in range(lo, 128) if i not in lost]

    def put(self, blocks):
        self.dg += [np.asarray(b, np.uint8) for b in blocks]

    def mark(self, kind, **kw):
        self.events.append(dict(kind=kind, **kw))

    def ordinary(self, n):
        """an ordinary frame trimmed to n datagrams: block 0 and n - 1 more of its 128 + 32 blocks in wire order"""
        _, fr = self.frame(32)
        self.put(fr[i] for i in [0] + sorted(self.rs.choice(np.arange(1, 160), n - 1, replace=False).tolist()))

    def fill_to(self, pos):
        """ordinary frames of flen datagrams up to position pos; the last ones are trimmed, none below 8 datagrams"""
        gap = pos - len(self.dg)
        assert gap == 0 or gap >= 8, (self.name, pos, gap)
        while gap:
            n = gap if gap <= self.flen else gap - 8 if gap < self.flen + 8 else self.flen
            self.ordinary(n)
            gap -= n

    def end(self, exact=False):
        """the datagram of another frame that releases the last one: behind the main call, or (exact) in a call of its own"""
        (self.tail if exact else self.dg).append(ee())
        return self

    # ---- the first frame of the main call and its carry
    def head(self, n_main):
        """the stream's first frame (fecblk 64): n_main datagrams of it open the main call, the first 128 of them distinct and
        none of the NRES blocks kept for the carry; behind 128 come repeats of its own blocks"""
        fi, fr = self.frame(64)
        res = [0] + self.rs.choice(np.arange(1, 192), NRES - 1, replace=False).tolist()
        rest = [i for i in range(192) if i not in res]
        first = sorted(self.rs.choice(rest, min(n_main, 128), replace=False).tolist())
        more = [int(x) for x in self.rs.randint(0, 192, max(n_main - 128, 0))]
        self.put(fr[i] for i in first + more)
        self._head = (fr, res, rest)
        self.mark("head", fi=fi, n_main=n_main)

    def carry(self, c):
        """c datagrams of the first frame for a call in front of the main call: block 0 first, no block of the main call's first
        128 - c, no repeat among the first 128"""
        if self._head is None or c == 0:
            return []
        fr, res, rest = self._head
        assert c <= len(res) + len(rest)
        return [fr[i] for i in (res + rest)[:c]]

    # ---- events at a chunk boundary B
    def start_at(self, pos, n=None):
        """a frame whose first datagram lies at pos"""
        self.fill_to(pos)
        self.mark("start", pos=pos)
        self.ordinary(n or self.flen)

    def rank128_at(self, pos):
        """fecblk 64, recovery rows 0 .. 9 lost: the frame's 128th arrival, the only row >= 32 among its first 128, lies at pos;
        recovery rows in front of it and (ignored) behind it"""
        self.fill_to(pos - 127)
        fi, fr = self.frame(64)
        self.mark("rank128", pos=pos, fi=fi)
        self.put(fr[i] for i in self.lose(20, lo=0) + list(range(138, 157)) + [128 + 45] + list(range(128 + 46, 192)))

    def dup_under_128(self, B):
        """an original at B - 50 repeated (another payload) at B + 10, ranks 10 and 70, recovery blocks among the first 128:
        a decode error, delivered as received, the last copy wins"""
        self.fill_to(B - 60)
        fi, fr = self.frame(32)
        o = self.lose(30, lo=0)
        self.mark("dup", fi=fi, first=B - 50, second=B + 10, under=True)
        self.put([fr[i] for i in o[:70]] + [altered(fr[o[10]])] + [fr[i] for i in o[70:]] + list(fr[128:]))

    def dup_past_128(self, B):
        """the twin: an original at B - 90 repeated at B + 20, rank 140: ignored, the frame is repaired; recovery rows on both
        sides of B below rank 128"""
        self.fill_to(B - 120)
        fi, fr = self.frame(32)
        o = self.lose(20, lo=0)
        self.mark("dup", fi=fi, first=B - 90, second=B + 20, under=False)
        self.put([fr[i] for i in o] + list(fr[128:]) + [altered(fr[o[30]])])

    def block0_then_release(self, B, rank=0, b0_prefix=None, kind="block0"):
        """block 0 at B - 50 + rank, the frame released at B + 90"""
        self.fill_to(B - 50)
        fi, fr = self.frame(32, b0_prefix)
        o = self.lose(20)
        o.insert(rank, 0)
        self.mark(kind, fi=fi, pos=B - 50 + rank, released=B + 90)
        self.put([fr[i] for i in o] + list(fr[128:]))
        return fr[0, 4:24].copy()

    def block0_same_12_bytes(self, B):
        """a frame P and, directly behind it, one whose MetaDataFEC equals P's in the first 12 bytes alone: block 0 at B - 30,
        released at B + 90: the metas stay P's"""
        self.fill_to(B - 50 - 140)
        meta = self.block0_then_release(B - 140, kind="block0_p")
        self.block0_then_release(B, rank=20, b0_prefix=meta[:12], kind="block0_same")

    def block0_twice(self, B):
        """block 0 at B - 35 and, with another payload, at B + 20 (ranks 5 and 60): the later copy is the frame's (a repeat:
        delivered as received)"""
        self.fill_to(B - 40)
        fi, fr = self.frame(32)
        o = self.lose(20)
        seq = [fr[i] for i in o]
        seq.insert(5, altered(fr[0]))
        seq.insert(60, fr[0])
        self.mark("block0_twice", fi=fi, first=B - 35, second=B + 20)
        self.put(seq + list(fr[128:]))

    def block0_past_128(self, B):
        """block 0 at rank 139 only (B + 39): no META, the decoder restores it"""
        self.fill_to(B - 100)
        fi, fr = self.frame(32)
        self.mark("block0_late", fi=fi, pos=B + 39)
        self.put([fr[i] for i in self.lose(20)] + list(fr[128:]) + [fr[0]])

    def aba(self, B, n_first):
        """frame A's first n_first datagrams up to B - 2, one datagram of another frame at B - 1, frame A again from B"""
        self.fill_to(B - 1 - n_first)
        fi, fr = self.frame(32)
        a = [fr[i] for i in self.lose(10, lo=0)] + list(fr[128:])
        _, other = self.frame(32)
        self.mark("aba", fi=fi, pos=B, n_first=n_first)
        self.put(a[:n_first] + [other[7]] + a[n_first:])

    def one_datagram_frames(self, pos, n):
        """n datagrams from pos on, each of a frame index of its own, through the wrap 65535 -> 0"""
        self.fill_to(pos)
        self.fi = 65536 - n // 2
        self.mark("singles", pos=pos, n=n)
        for k in range(n):
            d = self.rs.randint(0, 256, 512).astype(np.uint8)
            fi, self.fi = self.fi, (self.fi + 1) & 0xFFFF
            d[0], d[1], d[2], d[3] = fi & 0xFF, fi >> 8, (0, 131, 5, 77, 200)[k % 5] if k % 3 else k % 256, 0
            self.dg.append(d)

    def exact(self, n, last):
        """a main call of exactly n datagrams whose last frame has `last` of them; the 0xEE datagram comes in the call behind"""
        self.fill_to(n - last)
        fi, fr = self.frame(32)
        self.mark("exact", n=n, fi=fi, last=last)
        self.put(([fr[i] for i in self.lose(10, lo=0)] + list(fr[128:]))[:last])
        assert len(self.dg) == n
        return self.end(exact=True)


_BUILT = {}


def streams(oracle):
    """the bank: the long frame first (every later stream's packed offset is large and no multiple of 1024 datagrams), one
    empty stream among the others"""
    if "s" in _BUILT:
        return _BUILT["s"]
    B1, B2 = CL, 2 * CL
    out = []

    def new(name, flen=136, n_head=100):
        s = Stream(oracle, name, 1000 + len(out), 300 * len(out) + 7, flen)
        if n_head:
            s.head(n_head)
        out.append(s)
        return s

    s = new("long", n_head=LONG)          # no frame start in chunk 1 (and, behind a carry, none in chunk 0)
    s.mark("long", n=LONG)
    s.ordinary(140)
    s.end()
    s = new("start-a", 131)
    s.start_at(B1 - 1)
    s.start_at(B2 + 1)
    s.end()
    new("empty", n_head=0)
    s = new("start-b", 149)
    s.start_at(B1)
    s.start_at(B2 - 1)
    s.end()
    s = new("start-c", 140)
    s.start_at(B1 + 1)
    s.start_at(B2)
    s.end()
    s = new("rank128", 133)
    s.rank128_at(B1 - 1)
    s.rank128_at(B2)
    s.end()
    s = new("dup", 138)
    s.dup_under_128(B1)
    s.dup_past_128(B2)
    s.end()
    s = new("block0-a", 135)
    s.block0_twice(B1)
    s.block0_same_12_bytes(B2)
    s.end()
    s = new("block0-b", 137)
    s.block0_past_128(B1)
    s.block0_then_release(B2)
    s.end()
    s = new("singles", 134)
    s.one_datagram_frames(B1, RUN)
    s.fi = 40000
    s.ordinary(140)
    s.end()
    s = new("aba", 139)
    s.aba(B1, 79)
    s.aba(B2, 130)
    s.end()
    new("exact-1024", 132).exact(B1, 130)
    new("exact-1025", 136).exact(B1 + 1, 1)
    new("exact-2048", 141).exact(B2, 60)
    _BUILT["s"] = out
    return out


def index(oracle, name):
    return [s.name for s in streams(oracle)].index(name)


def _arr(dg):
    return np.asarray(dg, np.uint8).reshape(-1, 512)


def calls(oracle, carry):
    """per call, per stream an (n, 512) uint8 array: [the carry call (carry > 0)], the main call, the tail call"""
    st = streams(oracle)
    out = [[_arr(s.carry(carry)) for s in st]] if carry else []
    return out + [[_arr(s.dg) for s in st], [_arr(s.tail) for s in st]]


def sequences(oracle, carry):
    """per stream the whole datagram sequence"""
    return [np.concatenate([c[s] for c in calls(oracle, carry)]) for s in range(len(streams(oracle)))]


def models_of(oracle, the_calls):
    """per stream the oracle's restatement fed every call (fresh: check_against_model resets its statistics), and per call, per
    stream the number of frames the call releases"""
    ms = [tg.Model(oracle) for _ in the_calls[0]]
    counts = []
    for chunk in the_calls:
        before = [len(m.recs) for m in ms]
        for m, c in zip(ms, chunk):
            m.run(list(c))
        counts.append([len(m.recs) - b for m, b in zip(ms, before)])
    return ms, counts


def models(oracle, carry):
    return models_of(oracle, calls(oracle, carry))


TABLE_SIZES = (1, 3, 5)  # bank sizes 1 and 3 mod 4 (the main bank has 14 streams, the other datagram tests mostly 4, 8, 32 or 64)


def table_calls(oracle, S):
    """two calls that fill every column of the drivers' per-call table at a bank size of S: its 64-bit arrays lie behind a padded
    run of ints, so their offsets move with S mod 4.  The smallest such input, fecblk 4.  Call 1, per stream: a frame with one
    original lost (it goes to the decoder: dbase, a staging slot), then the first five datagrams of the next frame (an open
    slot in the carry buffer).  Call 2: the rest of that frame, nothing lost (the straight path), and one datagram of another
    frame that releases it.  Stream 1 (a bank of one has none) gets nothing in call 1 and both parts in call 2."""
    if ("table", S) not in _BUILT:
        rs = np.random.RandomState(4000 + S)
        one, two = [], []
        for s in range(S):
            a, b = tg.make_frames(oracle, rs, 2, 4, 500 * s + 11)
            lost = 1 + int(rs.randint(127))
            c1 = [a[i] for i in range(132) if i != lost] + list(b[:5])
            c2 = list(b[5:]) + [ee()]
            if s == 1:
                c1, c2 = [], c1 + c2
            one.append(_arr(c1))
            two.append(_arr(c2))
        _BUILT[("table", S)] = [one, two]
    return _BUILT[("table", S)]


def check_table_events(recs, counts):
    """recs[s]: every record stream s got back.  Every stream released its initial slot, a repaired frame and a complete one;
    all but stream 1 the first two in call 1"""
    S = len(recs)
    assert counts == [[0 if s == 1 else 2 for s in range(S)], [3 if s == 1 else 1 for s in range(S)]], counts
    for r in recs:
        assert [x["block_count"] for x in r] == [0, 131, 132] and [x["recovery_count"] for x in r[1:]] == [1, 0], r
        assert r[1]["flags"] & REPAIRED and not r[2]["flags"] & (REPAIRED | ERROR), r


def event(oracle, name, kind):
    s = streams(oracle)[index(oracle, name)]
    return s, [e for e in s.events if e["kind"] == kind]


def check_events(oracle, recs, counts, stats):
    """recs[s]: every record stream s got back; counts[call][s]: frames per call; stats(s): the collector's statistics.  The
    events happened."""
    ix = lambda name: index(oracle, name)  # noqa: E731
    by_fi = lambda name, fi: [r for r in recs[ix(name)] if r["frame_index"] == fi]  # noqa: E731
    _, dups = event(oracle, "dup", "dup")
    for e in dups:
        r, = by_fi("dup", e["fi"])
        assert r["flags"] & (ERROR if e["under"] else REPAIRED), (e, r)
        assert not r["flags"] & (REPAIRED if e["under"] else ERROR), (e, r)
    big = [r for r in recs[ix("long")] if r["block_count"] > CL]
    assert len(big) == 1 and big[0]["block_count"] >= LONG and big[0]["flags"] & REPAIRED, big
    assert max(c[ix("singles")] for c in counts) >= RUN                       # (that many records in one call)
    assert any(r["frame_index"] == 65535 for r in recs[ix("singles")]) and any(r["frame_index"] == 0 for r in recs[ix("singles")])
    _, (a1, a2) = event(oracle, "aba", "aba")
    assert [r["block_count"] for r in by_fi("aba", a1["fi"])] == [79, 150 - 79]  # (the second A starts afresh)
    assert [r["block_count"] for r in by_fi("aba", a2["fi"])] == [130, 150 - 130]
    # a meta change: the last META of "block0-b" differs from the one in front in its first 12 bytes
    s, (e,) = event(oracle, "block0-b", "block0")
    assert stats(ix("block0-b"))["output_meta"][:20] == bytes(s.dg[e["pos"]][4:24])
    # and a non-change: the last META of "block0-a" equals the one in front in its first 12 bytes alone
    s, (e,) = event(oracle, "block0-a", "block0_same")
    _, (p,) = event(oracle, "block0-a", "block0_p")
    st = stats(ix("block0-a"))
    assert st["output_meta"][:20] == st["current_meta"][:20] == bytes(s.dg[p["pos"]][4:24]) != bytes(s.dg[e["pos"]][4:24])
    r, = by_fi("block0-a", event(oracle, "block0-a", "block0_twice")[1][0]["fi"])
    assert r["flags"] & META and r["flags"] & ERROR
    r, = by_fi("block0-b", event(oracle, "block0-b", "block0_late")[1][0]["fi"])
    assert not r["flags"] & META and r["flags"] & REPAIRED
    for name in ("exact-1024", "exact-1025", "exact-2048"):
        s, (e,) = event(oracle, name, "exact")
        r, = by_fi(name, e["fi"])
        assert r["block_count"] == e["last"] and bool(r["flags"] & REPAIRED) == (e["last"] >= 128), (name, r)


def run_bank(bank, the_calls, device=True, max_frames=None):
    """test_gpu_fecbuf.run_bank with per-stream counts: -> per stream (frames, block0, records) over all calls, and per call
    the bank's last_n_frames"""
    import torch

    S = bank.nstreams
    res, counts = [([], [], []) for _ in range(S)], []
    for chunk in the_calls:
        out = bank.write_and_read([torch.from_numpy(c).cuda() for c in chunk] if device else chunk, max_frames)
        counts.append(list(bank.last_n_frames))
        for s in range(S):
            data, b0, recs = out[s]
            if device:
                data, b0 = data.cpu().numpy(), b0.cpu().numpy()
            res[s][0].extend(list(data))
            res[s][1].extend(list(b0))
            res[s][2].extend(recs)
    return res, counts
