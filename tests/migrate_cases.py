"""The scenario table of stream export / import (sdrhip_*_export_stream / _import_stream): every state a stream and a bank can be in
when a stream moves.  A scenario is a script of calls on a driver -- banks, datagram-fed and sample-fed calls, asynchronous batches,
the move -- and the driver keeps, per stream, the UNINTERRUPTED reference chain: the reference's SDRdaemonFECBuffer (or, without a
device, the oracle's restatement of it: the compiled class has no decoder there), a remainder buffer, the compiled-reference
decimators, the oracle framer and frame_encode for Rx; the collector and the oracle interpolators for Tx.  A chain that moves is
replayed into a second object (the exported stream runs on in the source as well) and gets the destination's settings from the
first frame completed after the move: log2decim and fcpos, the destination stream's nb_fec, its centre frequency and sample rate or
the followed incoming meta, log2interp.

The drivers here run the chains alone (tests/test_migrate_cases_model.py asserts that every move point is in the state its scenario
is named for); tests/test_gpu_stream_migrate_states.py derives drivers that make the same calls on the library and compare every
call's output with the chains'.  Inputs are seeded np.random.RandomState; F = 16129 decimated samples per frame."""
import numpy as np

import test_gpu_fecbuf as tg
import test_gpu_rx_datagrams as tr
import test_gpu_rx_follow_meta as tf
import test_gpu_stream_reset as ts
import test_gpu_tx_datagrams as tt

F = 16129
HOST = (435000, 625000)  # the defaults of RxPipe and of the oracle framer: centre frequency in kHz, sample rate of the sink
CUTS = [(2, 60), (3, 20)]
EMPTY = ts.EMPTY
PAYLOAD = 127 * 508


def iq(seed, n):
    return np.random.RandomState(seed).randint(-32768, 32768, size=(n, 2)).astype(np.int16)


class Collector:
    """one SDRdaemonFECBuffer: the reference's own class when its library is given, else the oracle's restatement; the restatement
    runs beside it either way (the block count of the open slot, m_outputMeta and the statistics come from there)"""

    def __init__(self, oracle, lib):
        self.ref = tt.RefChain(lib, oracle) if lib is not None else None
        self.model = tg.Model(oracle)
        self.first = True
        self.fed = 0

    def collect(self, dg):
        n0 = len(self.model.frames)
        self.model.run(dg)
        self.fed += len(dg)
        if self.ref is not None:
            return self.ref.collect(dg)
        out = [np.ascontiguousarray(np.asarray(p, np.uint8).reshape(-1)) for p in self.model.frames[n0:]]
        if out and self.first:  # (the initial slot: uninitialised memory in the reference, zero in the library -- include/sdrhip.h)
            out[0] = np.zeros(PAYLOAD, np.uint8)
        self.first = self.first and not out
        return out

    @property
    def open_blocks(self):
        return int(self.model.b.s.block_count) if self.fed else 0


class RxChain(tr.HubChain):
    """HubChain that remembers its calls (clone() replays them into a second object), counts its decimated samples and takes the
    two meta words of the frames a call opens"""

    def __init__(self, oracle, lib=None, hb=0):
        from oracle_lib import Reference

        self.oracle, self.lib, self.hb = oracle, lib, hb
        self.col = Collector(oracle, lib)
        flavour = "db" if hb else "eo1"
        self.dec = Reference(flavour).decimators() if Reference.available(flavour) else oracle.decimators(hb)
        self.fr = oracle.framer(center_frequency_khz=HOST[0], sample_rate=HOST[1])
        self.rem = np.zeros((0, 2), np.int16)
        self.log, self.ndec, self.done = [], 0, 0

    def clone(self):
        c = RxChain(self.oracle, self.lib, self.hb)
        for kind, args in self.log:
            getattr(c, kind)(*args)
        assert (c.ndec, c.done, len(c.rem)) == (self.ndec, self.done, len(self.rem))
        return c

    held = property(lambda self: len(self.rem))
    pending = property(lambda self: self.ndec % F)
    open_blocks = property(lambda self: self.col.open_blocks)

    def _frames(self, x, L, fcpos, R, sec, usec, words):
        self.fr.s.center_frequency_khz, self.fr.s.sample_rate = words
        out = tr.HubChain.samples(self, x, L, fcpos, R, sec, usec)
        self.ndec += len(x) >> L
        self.done += len(out)
        assert self.done == self.ndec // F, (self.done, self.ndec)
        return out

    def samples(self, x, L, fcpos, R, sec, usec, host=HOST):
        self.log.append(("samples", (x, L, fcpos, R, sec, usec, host)))
        return self._frames(x, L, fcpos, R, sec, usec, host)

    def dgrams(self, dg, L, fcpos, R, sec, usec, host=HOST, follow=False):
        self.log.append(("dgrams", (dg, L, fcpos, R, sec, usec, host, follow)))
        pay = self.col.collect(dg)
        if pay:
            self.rem = np.concatenate([self.rem] + [p.view(np.int16).reshape(-1, 2) for p in pay])
        u = tr.unit(L, fcpos)
        n = len(self.rem) // u * u
        x, self.rem = self.rem[:n], self.rem[n:]
        words = tf.rule(self.col.model.out_meta, L, host) if follow else host
        return self._frames(x, L, fcpos, R, sec, usec, words)


class TxChain:
    """one stream of sdrdaemontx: the collector and the oracle's interpolators (one Upsampler), with the log of its calls"""

    def __init__(self, oracle, lib=None):
        self.oracle, self.lib = oracle, lib
        self.col = Collector(oracle, lib)
        self.itp = oracle.interpolators()
        self.log, self.done = [], 0

    def clone(self):
        c = TxChain(self.oracle, self.lib)
        for kind, args in self.log:
            getattr(c, kind)(*args)
        assert c.done == self.done
        return c

    open_blocks = property(lambda self: self.col.open_blocks)

    def _out(self, pay, L):
        self.done += len(pay)
        if not len(pay):
            return np.zeros((0, 2), np.int16)
        return self.itp.interpolate(L, np.concatenate(pay).view(np.int16).reshape(-1, 2))

    def feed(self, dg, L):
        self.log.append(("feed", (dg, L)))
        return self._out(self.col.collect(dg), L)

    def frames(self, fr, L):
        """frames through sdrhip_tx_process: the 127 payload blocks of each"""
        self.log.append(("frames", (fr, L)))
        return self._out([np.ascontiguousarray(f[1:128, 4:]).reshape(-1) for f in fr], L)


class Bank:
    def __init__(self, name, kind, S, ctx=0, **cfg):
        self.name, self.kind, self.S, self.ctx = name, kind, S, ctx
        self.L, self.fcpos, self.R, self.hb = cfg.pop("L", 2), cfg.pop("fcpos", 2), cfg.pop("R", 8), cfg.pop("hb", 0)
        self.fec, self.meta, self.follow = cfg.pop("fec", None), cfg.pop("meta", None), cfg.pop("follow", False)
        self.fmt, self.depth, self.egress = cfg.pop("fmt", "s16"), cfg.pop("depth", 0), cfg.pop("egress", False)
        assert not cfg, cfg
        self.chains, self.queue, self.ncalls, self.has_col = [], [], 0, False

    def R_of(self, s):
        return self.fec[s] if self.fec else self.R

    def host_of(self, s):
        return tuple(self.meta[s]) if self.meta else HOST


class Run:
    """what both kinds of driver share: the banks, the moves and what the model test asserts of them"""

    kind = None

    def __init__(self, oracle, lib=None, case="", params=None):
        self.oracle, self.lib, self.case, self.p = oracle, lib, case, dict(params or {})
        self.banks, self.moves = [], []

    def new_chain(self, b):
        return RxChain(self.oracle, self.lib, b.hb) if self.kind == "rx" else TxChain(self.oracle, self.lib)

    def bank(self, name, S, **cfg):
        b = Bank(name, self.kind, S, **cfg)
        b.chains = [self.new_chain(b) for _ in range(S)]
        self.banks.append(b)
        self.on_bank(b)
        return b

    def where(self, b, s=None):
        return (self.case, b.name, "call %d" % b.ncalls) + (() if s is None else ("stream %d" % s,))

    def _called(self, b, exp):
        """the frames (Rx: their two meta words) every moved chain of this bank has completed since its move"""
        for m in self.moves:
            if m["dst"] is b:
                e = exp[m["d"]]
                m["after"] += [tf.meta_of(f)[:2] for f in e] if self.kind == "rx" else [None] * e
        b.ncalls += 1

    def move(self, src, s, dst, d):
        """stream s of src continues as stream d of dst (and runs on in src)"""
        ch, old = src.chains[s], dst.chains[d]
        m = dict(src=src, s=s, dst=dst, d=d, after=[], open_blocks=ch.open_blocks, has_col=src.has_col, dst_has_col=dst.has_col,
                 src_done=[c.done for c in src.chains], dst_done=[c.done for c in dst.chains], dst_calls=dst.ncalls,
                 old_open_blocks=old.open_blocks)
        if self.kind == "rx":
            m.update(held=ch.held, pending=ch.pending, old_held=old.held, old_pending=old.pending)
        dst.chains[d] = ch.clone()
        self.moves.append(m)
        self.on_move(src, s, dst, d)
        dst.has_col = dst.has_col or src.has_col
        return m

    def restart(self, b, s):
        """stream s of b begins again: a fresh chain (a reset, or the import of a never-used stream's blob)"""
        b.chains[s] = self.new_chain(b)

    # ---- what a library driver overrides
    def on_bank(self, b): pass
    def on_move(self, src, s, dst, d): pass
    def option(self, ctx, key, value): pass
    def assert_path(self, b, path): pass
    def assert_refusals_of_an_unaligned_bank(self, b, x): pass
    def roundtrip(self, b, s): pass
    def fresh_blobs_equal(self, b, s_reset, s_unused): pass
    def import_fresh_blob(self, b, s, s_unused): self.restart(b, s)
    def reset(self, b, s): self.restart(b, s)
    def finish(self): pass


class RxRun(Run):
    kind = "rx"

    def _exp_dgrams(self, b, chunk, sec, usec):
        b.has_col = True
        return [c.dgrams(chunk[s], b.L, b.fcpos, b.R_of(s), sec, usec, b.host_of(s), b.follow) for s, c in enumerate(b.chains)]

    def dgrams(self, b, chunk, sec, usec=5, device=True):
        exp = self._exp_dgrams(b, chunk, sec, usec)
        self.on_dgrams(b, chunk, sec, usec, device, exp)
        self._called(b, exp)

    def ragged(self, b, xs, sec, usec=1, uniform=False):
        """xs: per stream its (n_s, 2) samples; uniform: through sdrhip_rx_process (equal counts)"""
        exp = [c.samples(np.ascontiguousarray(xs[s]), b.L, b.fcpos, b.R_of(s), sec, usec, b.host_of(s)) for s, c in enumerate(b.chains)]
        self.on_ragged(b, xs, sec, usec, uniform, exp)
        self._called(b, exp)

    def submit(self, b, chunk, sec, usec=5, tagged=None):
        """tagged: the seed of the arrival-order merge (None: per-stream arrays)"""
        exp = self._exp_dgrams(b, chunk, sec, usec)
        b.queue.append(exp)
        self.on_submit(b, chunk, sec, usec, tagged)

    def collect(self, b):
        exp = b.queue.pop(0)
        self.on_collect(b, exp)
        self._called(b, exp)

    def on_dgrams(self, b, chunk, sec, usec, device, exp): pass
    def on_ragged(self, b, xs, sec, usec, uniform, exp): pass
    def on_submit(self, b, chunk, sec, usec, tagged): pass
    def on_collect(self, b, exp): pass


class TxRun(Run):
    kind = "tx"

    def _exp(self, b, chunk):
        b.has_col = True
        return [c.feed(chunk[s], b.L) for s, c in enumerate(b.chains)]

    def _called(self, b, exp):
        Run._called(self, b, [e.shape[0] // (F << b.L) for e in exp])

    def dgrams(self, b, chunk, device=True):
        exp = self._exp(b, chunk)
        self.on_dgrams(b, chunk, device, exp)
        self._called(b, exp)

    def process(self, b, frames):
        """frames: per stream the same number of (128, 512) frames, through sdrhip_tx_process"""
        exp = [c.frames(frames[s], b.L) for s, c in enumerate(b.chains)]
        self.on_process(b, frames, exp)
        self._called(b, exp)

    def submit(self, b, chunk, tagged=None):
        b.queue.append(self._exp(b, chunk))
        self.on_submit(b, chunk, tagged)

    def collect(self, b):
        exp = b.queue.pop(0)
        self.on_collect(b, exp)
        self._called(b, exp)

    def on_dgrams(self, b, chunk, device, exp): pass
    def on_process(self, b, frames, exp): pass
    def on_submit(self, b, chunk, tagged): pass
    def on_collect(self, b, exp): pass


# ------------------------------------------------------------------------------------------------ inputs, kept per seed
_KEPT = {}


def kept(key, make):
    if key not in _KEPT:
        _KEPT[key] = make()
    return _KEPT[key]


def follow_calls(oracle, seed, S, cuts=CUTS, nframes=10):
    """ts.follow_streams (real meta blocks: centre frequency 900000 + s, rate 2000000 + 2 s; incoming fecblk 4, three blocks other
    than block 0 lost per frame) cut into calls at `cuts`: per call, per stream an (n, 512) array"""
    return kept(("follow", seed, S, tuple(cuts), nframes), lambda: ts.dgram_calls(ts.follow_streams(oracle, seed, S, nframes), cuts))


def frame_starts(dg):
    """positions at which a datagram sequence begins another frame index"""
    fi = dg[:, 0].astype(int) | (dg[:, 1].astype(int) << 8)
    return [0] + (1 + np.flatnonzero(np.diff(fi))).tolist()


def long_stream(oracle, seed, nframes, cuts):
    """one stream of tt.stream_dgrams (incoming fecblk 2, random payload) cut at (frame, datagrams into it) positions"""
    def make():
        dg = np.asarray(tt.stream_dgrams(oracle, np.random.RandomState(seed), nframes, 2), np.uint8).reshape(-1, 512)
        st = frame_starts(dg)
        b = [0] + [st[k] + off for k, off in cuts] + [dg.shape[0]]
        return [dg[b[i]:b[i + 1]] for i in range(len(b) - 1)]
    return kept(("long", seed, nframes, tuple(cuts)), make)


def tx_cuts(oracle, seed, S, bounds=(200, 420), nframes=4):
    """per stream tt.stream_dgrams (nframes frames of fecblk 32 with random losses, one datagram of the next) cut at `bounds`:
    per call, per stream an (n, 512) array.  200 datagrams: one released frame and an open slot"""
    def make():
        rs = np.random.RandomState(seed)
        per = [np.asarray(tt.stream_dgrams(oracle, rs, nframes, 32), np.uint8).reshape(-1, 512) for _ in range(S)]
        b = [0] + list(bounds) + [None]
        return [[p[b[i]:b[i + 1]] for p in per] for i in range(len(b) - 1)]
    return kept(("tx", seed, S, tuple(bounds), nframes), make)


def tx_frames(oracle, seed, S, n):
    """per stream n whole frames (128 originals) for sdrhip_tx_process"""
    return kept(("txfr", seed, S, n), lambda: [tg.make_frames(oracle, np.random.RandomState(seed + s), n, 0, 10 * s) for s in range(S)])


# ------------------------------------------------------------------------------------------------ Rx scenarios
def rx_fresh_destination(run, feed):
    """1. B is created and never called before the import; the blob has an open frame, an open collector slot and 3 held-back
    samples (feed = samples: the blob of a sample-fed source, B's first call is process_ragged)"""
    A, B = run.bank("A", 3, R=8), run.bank("B", 2, ctx=1, R=32)
    if feed == "dgrams":
        ca, cb = follow_calls(run.oracle, 101, 3), follow_calls(run.oracle, 102, 2)
        run.dgrams(A, ca[0], 300)
        run.move(A, 1, B, 0)
        for i in (1, 2):
            run.dgrams(A, ca[i], 300 + i, device=i == 1)
            run.dgrams(B, [ca[i][1], cb[i - 1][1]], 400 + i, device=i == 2)
    else:
        f = F << 2
        run.ragged(A, [iq(110 + s, n) for s, n in enumerate([3 * f // 2, 7 * f // 10, 11 * f // 5 + 3])], 300)
        run.move(A, 1, B, 0)
        for i in (1, 2):
            run.ragged(A, [iq(120 + 10 * i + s, n) for s, n in enumerate([4 * f // 5, 13 * f // 10, f // 3 + i])], 300 + i)
            run.ragged(B, [iq(140 + 10 * i + s, n) for s, n in enumerate([13 * f // 10, 6 * f // 5 + 5])], 400 + i)


def rx_collector_on_one_side(run, side):
    """2. side = dst: the source was only ever sample-fed; the destination stream has an open collector slot of 60 blocks and a
    carry of 3, and behaves as a constructor-fresh collector with no carry after the import.  side = src: the source has a
    collector, the destination has only been sample-fed, then gets datagrams"""
    f = F << 2
    A, B = run.bank("A", 3, R=8), run.bank("B", 2, ctx=1, R=32)
    ca, cb = follow_calls(run.oracle, 103, 3), follow_calls(run.oracle, 104, 2)
    if side == "dst":
        run.ragged(A, [iq(150 + s, n) for s, n in enumerate([3 * f // 2, 7 * f // 10, 11 * f // 5 + 3])], 300)
        run.dgrams(B, cb[0], 400)
        run.move(A, 1, B, 0)
        for i in (1, 2, 3):
            run.ragged(A, [iq(160 + 10 * i + s, n) for s, n in enumerate([4 * f // 5, 13 * f // 10, f // 3 + i])], 300 + i)
        run.dgrams(B, [ca[0][1], cb[1][1]], 401)  # (the moved stream's first datagrams ever: the zero initial slot is released)
        run.dgrams(B, [ca[1][1], cb[2][1]], 402, device=False)
        run.dgrams(B, [ca[2][1], EMPTY], 403)
    else:
        run.dgrams(A, ca[0], 300)
        run.ragged(B, [iq(170 + s, n) for s, n in enumerate([6 * f // 5, f // 2 + 7])], 400)
        run.move(A, 1, B, 0)
        for i in (1, 2):
            run.dgrams(A, ca[i], 300 + i)
            run.dgrams(B, [ca[i][1], cb[i - 1][1]], 400 + i, device=i == 1)


def rx_wide_first_stage_history(run, path):
    """3. the source leaves rotate-sums wider than 16 bits in the first stage's history (decimate8 sup on full-scale noise, the DB
    half-band filter: test_short_centred_call_after_inf_keeps_wide_history); the destination has only run centred calls of at
    least 128 samples, so its bank-wide "first-stage history fits int16" shortcut is set.  After the import: a centred call of 40
    samples (shorter than the history: the wide values stay), one of 70000 on `path`, one that completes a second frame"""
    A, B = run.bank("A", 2, L=3, fcpos=1, hb=1, R=8), run.bank("B", 2, ctx=1, L=4, fcpos=2, hb=1, R=8)
    run.ragged(A, [iq(180 + s, (F - 1536 - 300) << 3) for s in range(2)], 300)
    run.ragged(A, [iq(1 + s, 12289) for s in range(2)], 301)  # (signals.noise(12289, 1) on stream 0)
    run.ragged(B, [iq(190, 4096), iq(191, 2048)], 400)
    run.move(A, 0, B, 1)
    run.ragged(A, [iq(192 + s, 5000 + 8 * s) for s in range(2)], 302)
    run.ragged(A, [iq(194 + s, (F // 2) << 3) for s in range(2)], 303)
    run.ragged(B, [iq(196, 200), iq(2, 40)], 401)
    run.option(1, "decim_path", path)
    run.option(1, "mfma_span", 1024)
    run.ragged(B, [iq(197, 70000 + 16), iq(7, 70000)], 402)
    run.assert_path(B, path)
    run.option(1, "decim_path", "auto")
    run.option(1, "mfma_span", 0)
    run.ragged(B, [iq(198, F << 4), iq(199, (F + 100) << 4)], 403)


def rx_another_decimation(run, L, fcpos):
    """4. the source runs decimate64 centred (primed so that the few payloads complete frames) and holds 36 samples back at the
    move; the destination runs decimate4 centred or decimate2 inf, unit 4 either way.  The first call after the import feeds only
    3 datagrams: the held-back samples alone go through the destination's unit"""
    A, B = run.bank("A", 2, L=6, R=8), run.bank("B", 2, ctx=1, L=L, fcpos=fcpos, R=32)
    mv = long_stream(run.oracle, 105, 42, [(35, 10), (35, 13), (38, 50)])
    nb, cb = follow_calls(run.oracle, 106, 1), follow_calls(run.oracle, 107, 2)
    run.ragged(A, [iq(200 + s, (F - 300) << 6) for s in range(2)], 299)
    run.dgrams(A, [mv[0], nb[0][0]], 300)
    run.dgrams(B, cb[0], 400)
    run.move(A, 0, B, 1)
    run.dgrams(A, [mv[1], nb[1][0]], 301)
    run.dgrams(A, [np.concatenate([mv[2], mv[3]]), nb[2][0]], 302)
    run.dgrams(B, [cb[1][0], mv[1]], 401)
    run.dgrams(B, [EMPTY, mv[2]], 402, device=False)
    run.dgrams(B, [cb[2][0], mv[3]], 403)


DST_FEC = [0, 13, 33]  # one stream per encoder form with enc_min_rows = 1: no recovery blocks, the FFT form (<= 32), the walk


def rx_destination_settings(run, d):
    """5. B has its own fecblk per stream (three encoder forms in one bank, one slot pitch), its own centre frequency and sample
    rate per stream, and follows the incoming meta.  The imported open frame completes with 128 + nb_fec[d] blocks and the meta
    block it was opened with (A's host values); the next frame announces the incoming meta that came with the blob's m_outputMeta"""
    A = run.bank("A", 2, R=8)
    B = run.bank("B", 3, ctx=1, R=8, fec=DST_FEC, meta=[(1000 + s, 2000000 + s) for s in range(3)], follow=True)
    ca, cb = follow_calls(run.oracle, 108, 2), follow_calls(run.oracle, 109, 3)
    run.dgrams(A, ca[0], 300)
    run.dgrams(B, cb[0], 400)
    run.move(A, 1, B, d)
    for i in (1, 2):
        run.dgrams(A, ca[i], 300 + i)
        run.dgrams(B, [ca[i][1] if s == d else cb[i][s] for s in range(3)], 400 + i, device=i == 1)


def rx_open_frame_on_the_matrix_cores(run, direct):
    """6. the destination runs decimate16 forced onto the matrix cores (span 1024); the import carries an open frame of 13097
    samples (not a multiple of 4); a ragged call that feeds the imported stream nothing, then one that completes the frame 5000
    samples into the next"""
    A, B = run.bank("A", 2, R=8), run.bank("B", 3, ctx=1, L=4, R=32)
    ca, cb = follow_calls(run.oracle, 111, 2), follow_calls(run.oracle, 112, 3)
    run.option(1, "rx_direct", direct)
    run.dgrams(A, ca[0], 300)
    run.ragged(A, [iq(210, 1001 << 2), iq(211, 64)], 301)
    run.ragged(B, [iq(212 + s, n) for s, n in enumerate([3000 << 4, 1000 << 4, 2048])], 400)
    m = run.move(A, 0, B, 1)
    run.dgrams(A, ca[1], 302)
    run.dgrams(A, ca[2], 303)
    run.option(1, "decim_path", "mfma")
    run.option(1, "mfma_span", 1024)
    run.ragged(B, [iq(221, 40000), iq(222, 0), iq(223, 30000 + 5)], 401)  # (the imported stream idle: its history is copied through)
    run.assert_path(B, "mfma")
    run.ragged(B, [iq(215, (3000 << 4) + 16), iq(216, (F - m["pending"] + 5000) << 4), iq(217, 50000)], 401)
    run.assert_path(B, "mfma")
    run.option(1, "decim_path", "auto")
    run.option(1, "mfma_span", 0)
    run.dgrams(B, [cb[0][0], ca[1][0], cb[0][2]], 402)
    run.ragged(B, [iq(218, 4096), iq(219, F << 4), iq(220, 100)], 403)
    run.option(1, "rx_direct", 1)


def rx_windows_away_from_slot_0(run):
    """7. rx_window = 1 (the area holds one call's window).  The exported stream completes 3 frames while its neighbours complete
    none: its window stands at slot 3.  The destination stream stands at slot 2 of 3, its neighbour at 0.  After the import one
    call makes the imported window wrap in place, a later one makes the area grow"""
    f = F << 2
    run.option(0, "rx_window", 1)
    run.option(1, "rx_window", 1)
    A, B = run.bank("A", 3, R=8), run.bank("B", 2, ctx=1, R=32)
    run.ragged(A, [iq(230 + s, n) for s, n in enumerate([f // 2, 3 * f + f // 2 + 3, f // 3])], 300)
    run.ragged(B, [iq(233, 2 * f + f // 4), iq(234, f // 5)], 400)
    run.move(A, 1, B, 0)
    run.ragged(A, [iq(235 + s, n) for s, n in enumerate([f, f // 4, f // 3])], 301)
    run.ragged(A, [iq(238 + s, n) for s, n in enumerate([f // 2, 2 * f, 4 * f])], 302)
    run.ragged(B, [iq(241, f), iq(242, 400)], 401)              # (slot 2 + 1 frame + the open one: past the 3 slots, back to slot 0)
    run.ragged(B, [iq(243, f // 4), iq(244, f)], 402)
    run.ragged(B, [iq(245, 5 * f), iq(246, f // 2)], 403)       # (6 slots needed: a new area)
    run.option(0, "rx_window", 0)
    run.option(1, "rx_window", 0)


def rx_asynchronous_continuation(run, mode, shadow):
    """8. after the import two batches are in flight (depth 2), then collected.  mode: per-stream arrays, a tagged arrival-order
    batch, or departure-order egress.  shadow = patched: an asynchronous batch ran on B before the import (the host's shadow of the
    collector is valid and the import patches it); refreshed: B only ran a synchronous call"""
    A = run.bank("A", 3, R=8)
    B = run.bank("B", 2, ctx=1, R=32, depth=2, egress=mode == "egress")
    ca, cb = follow_calls(run.oracle, 113, 3), follow_calls(run.oracle, 114, 2)
    run.dgrams(A, ca[0], 300)
    if shadow == "patched":
        run.submit(B, cb[0], 400)
        run.collect(B)
    else:
        run.dgrams(B, cb[0], 400)
    run.move(A, 1, B, 0)
    for i in (1, 2):
        run.submit(B, [ca[i][1], cb[i][1]], 400 + i, tagged=60 + i if mode == "tagged" else None)
    for i in (1, 2):
        run.dgrams(A, ca[i], 300 + i)
        run.collect(B)


REBALANCE_CUTS = [(2, 60), (3, 20), (6, 40)]


def rx_whole_bank_rebalance(run):
    """9. all 6 streams of A go into a fresh 6-stream B back to back with no call in between (four staging buffers: the fifth
    import waits for the first upload), stream s to stream (s + 1) mod 6; then three calls"""
    A, B = run.bank("A", 6, R=8), run.bank("B", 6, ctx=1, R=32)
    ca = follow_calls(run.oracle, 115, 6, REBALANCE_CUTS)
    run.dgrams(A, ca[0], 300)
    for s in range(6):
        run.move(A, s, B, (s + 1) % 6)
    for i in (1, 2, 3):
        run.dgrams(B, [ca[i][(d - 1) % 6] for d in range(6)], 400 + i, device=i != 2)
    for i in (1, 2):
        run.dgrams(A, ca[i], 300 + i)


def rx_round_trip_and_fresh_blobs(run):
    """10. export -> import into the same stream -> export gives the same bytes; a just-reset stream's blob equals a never-used
    stream's; importing such a blob into a live stream is reset_streams([s]): a fresh chain"""
    A = run.bank("A", 4, R=8)
    ca = follow_calls(run.oracle, 116, 3)
    run.dgrams(A, ca[0] + [EMPTY], 300)  # (stream 3 is never used)
    run.roundtrip(A, 1)
    run.dgrams(A, ca[1] + [EMPTY], 301)
    run.reset(A, 0)
    run.fresh_blobs_equal(A, 0, 3)
    run.import_fresh_blob(A, 2, 3)
    run.dgrams(A, ca[2] + [EMPTY], 302)
    run.dgrams(A, [ca[0][s] for s in (2, 0, 1)] + [EMPTY], 303)


def rx_alignment_after_an_import(run):
    """11. a sample-fed bank whose streams stood aligned: after an import it is what it is after a partial reset -- sdrhip_rx_process
    takes its ragged step and still matches the chains; set_async + submit and pipelined mode refuse, nothing consumed"""
    f = F << 2
    A, B = run.bank("A", 2, R=8), run.bank("B", 3, ctx=1, R=8)
    run.ragged(A, [iq(250, 2 * f // 3), iq(251, 6 * f // 5 + 2)], 300)
    run.ragged(B, [iq(252 + s, 3 * f // 2) for s in range(3)], 400, uniform=True)
    run.move(A, 1, B, 1)
    run.assert_refusals_of_an_unaligned_bank(B, [iq(255 + s, 64) for s in range(3)])
    run.ragged(A, [iq(258, f), iq(259, f // 2)], 301)
    run.ragged(A, [iq(260, f // 2), iq(261, f)], 302)
    run.ragged(B, [iq(262 + s, 6 * f // 5) for s in range(3)], 401, uniform=True)
    run.ragged(B, [iq(265 + s, f) for s in range(3)], 402, uniform=True)


# ------------------------------------------------------------------------------------------------ Tx scenarios
def tx_fresh_destination(run):
    """1. B is created and never called before the import"""
    A, B = run.bank("A", 3), run.bank("B", 2, ctx=1)
    ca, cb = tx_cuts(run.oracle, 301, 3), tx_cuts(run.oracle, 302, 1)
    run.dgrams(A, ca[0])
    run.move(A, 1, B, 0)
    for i in (1, 2):
        run.dgrams(A, ca[i], device=i == 1)
        run.dgrams(B, [ca[i][1], cb[i - 1][0]], device=i == 2)


def tx_another_interpolation(run):
    """2. source interpolate4, destination interpolate32"""
    A, B = run.bank("A", 2), run.bank("B", 2, ctx=1, L=5)
    ca, cb = tx_cuts(run.oracle, 303, 2), tx_cuts(run.oracle, 304, 1, nframes=2, bounds=(140, 200))
    run.dgrams(A, ca[0])
    run.dgrams(B, [cb[0][0], EMPTY])
    run.move(A, 1, B, 1)
    for i in (1, 2):
        run.dgrams(A, ca[i])
        run.dgrams(B, [cb[i][0], ca[i][1]])


def tx_collector_on_one_side(run, side):
    """3. side = dst: the source is fed frames through sdrhip_tx_process and never had a collector, the destination stream has an
    open slot and begins as a fresh collector; side = src: the destination has only been fed frames, then gets datagrams"""
    A, B = run.bank("A", 3), run.bank("B", 2, ctx=1)
    ca, cb = tx_cuts(run.oracle, 305, 3), tx_cuts(run.oracle, 306, 2)
    fa, fb = tx_frames(run.oracle, 310, 3, 3), tx_frames(run.oracle, 320, 2, 3)
    if side == "dst":
        run.process(A, [f[:1] for f in fa])
        run.dgrams(B, cb[0])
        run.move(A, 1, B, 0)
        for i in (1, 2):
            run.process(A, [f[i:i + 1] for f in fa])
        run.dgrams(B, [ca[0][1], cb[1][1]])
        run.dgrams(B, [ca[1][1], cb[2][1]])
        run.dgrams(B, [ca[2][1], EMPTY])
    else:
        run.dgrams(A, ca[0])
        run.process(B, [f[:1] for f in fb])
        run.move(A, 1, B, 0)
        for i in (1, 2):
            run.dgrams(A, ca[i])
            run.dgrams(B, [ca[i][1], cb[i - 1][1]])


def tx_asynchronous_continuation(run, shadow):
    """4. after the import a submit_datagrams and a submit_datagrams_tagged batch are in flight together, then collected"""
    A, B = run.bank("A", 3), run.bank("B", 2, ctx=1, depth=2)
    ca, cb = tx_cuts(run.oracle, 307, 3), tx_cuts(run.oracle, 308, 2)
    run.dgrams(A, ca[0])
    if shadow == "patched":
        run.submit(B, cb[0])
        run.collect(B)
    else:
        run.dgrams(B, cb[0])
    run.move(A, 1, B, 0)
    run.submit(B, [ca[1][1], cb[1][1]])
    run.submit(B, [ca[2][1], cb[2][1]], tagged=70)
    for i in (1, 2):
        run.dgrams(A, ca[i])
        run.collect(B)


def tx_int8_output(run, path):
    """5. the destination delivers int8 ("s8") with segments of 128 inputs: every segment warms up on the imported history"""
    A, B = run.bank("A", 2), run.bank("B", 2, ctx=1, fmt="s8")
    ca, cb = tx_cuts(run.oracle, 309, 2), tx_cuts(run.oracle, 311, 1)
    run.option(1, "interp_path", path)
    run.option(1, "interp_span", 128)
    run.dgrams(A, ca[0])
    run.dgrams(B, [cb[0][0], EMPTY])
    run.move(A, 0, B, 1)
    run.dgrams(B, [cb[1][0], EMPTY])  # (the imported stream idle while its neighbour releases frames: its history is copied through)
    run.dgrams(B, [cb[2][0], ca[1][0]], device=False)
    run.dgrams(B, [EMPTY, ca[2][0]])
    for i in (1, 2):
        run.dgrams(A, ca[i])
    run.option(1, "interp_path", "auto")
    run.option(1, "interp_span", 0)


def tx_whole_bank_rebalance(run):
    """6. six imports in a row into a fresh bank, stream s to stream (s + 1) mod 6"""
    A, B = run.bank("A", 6), run.bank("B", 6, ctx=1)
    ca = tx_cuts(run.oracle, 312, 6)
    run.dgrams(A, ca[0])
    for s in range(6):
        run.move(A, s, B, (s + 1) % 6)
    for i in (1, 2):
        run.dgrams(B, [ca[i][(d - 1) % 6] for d in range(6)], device=i == 1)
        run.dgrams(A, ca[i])


def tx_round_trip_and_fresh_blobs(run):
    """7. the blob round trip and the fresh blobs of Rx scenario 10"""
    A = run.bank("A", 4)
    ca = tx_cuts(run.oracle, 313, 3)
    run.dgrams(A, ca[0] + [EMPTY])
    run.roundtrip(A, 1)
    run.dgrams(A, ca[1] + [EMPTY])
    run.reset(A, 0)
    run.fresh_blobs_equal(A, 0, 3)
    run.import_fresh_blob(A, 2, 3)
    run.dgrams(A, ca[2] + [EMPTY])
    run.dgrams(A, [ca[0][s] for s in (2, 0, 1)] + [EMPTY])
    run.dgrams(A, [ca[1][s] for s in (2, 0, 1)] + [EMPTY])


# ------------------------------------------------------------------------------------------------ the table
class Case:
    """name, the script and its arguments, and what the chains alone must show at every move (the model test's conditions):
    held = (lo, hi) samples held back; open_frame; blocks = fewest blocks in the exported stream's open collector slot (None: the
    blob has no collector); old = what the destination stream it replaces must hold: (fewest blocks of its open slot, fewest
    held-back samples); src_done / dst_done = frames completed per stream before the move; after = fewest frames completed in the
    destination after the move; words = the two meta words of the first frames completed after the move"""

    def __init__(self, kind, fn, args=(), **expect):
        self.kind, self.fn, self.args, self.expect = kind, fn, tuple(args), expect
        self.id = "-".join([fn.__name__] + [str(a) for a in args])

    def run(self, run):
        self.fn(run, *self.args)
        run.finish()
        return run


RX_DEFAULT = dict(held=(1, 63), open_frame=True, blocks=1, after=2)
NO_COLLECTOR = dict(held=(0, 0), open_frame=True, blocks=None, after=2)

RX_CASES = [
    Case("rx", rx_fresh_destination, ["dgrams"], dst_calls=0, **RX_DEFAULT),
    Case("rx", rx_fresh_destination, ["samples"], dst_calls=0, **NO_COLLECTOR),
    Case("rx", rx_collector_on_one_side, ["dst"], old=(20, 1), **NO_COLLECTOR),
    Case("rx", rx_collector_on_one_side, ["src"], dst_collector=False, **RX_DEFAULT),
    Case("rx", rx_wide_first_stage_history, ["valu"], **NO_COLLECTOR),
    Case("rx", rx_wide_first_stage_history, ["mfma"], **NO_COLLECTOR),
    Case("rx", rx_another_decimation, [2, 2], held=(33, 63), open_frame=True, blocks=1, after=2),
    Case("rx", rx_another_decimation, [1, 0], held=(33, 63), open_frame=True, blocks=1, after=2),
] + [
    Case("rx", rx_destination_settings, [d], words=[HOST, (900001, 2000002 >> 2)], **RX_DEFAULT) for d in range(3)
] + [
    Case("rx", rx_open_frame_on_the_matrix_cores, [1], pending_mod4=True, **RX_DEFAULT),
    Case("rx", rx_open_frame_on_the_matrix_cores, [0], pending_mod4=True, **RX_DEFAULT),
    Case("rx", rx_windows_away_from_slot_0, [], src_done=[0, 3, 0], dst_done=[2, 0], **NO_COLLECTOR),
] + [
    Case("rx", rx_asynchronous_continuation, [mode, shadow], **RX_DEFAULT)
    for mode in ("plain", "tagged", "egress") for shadow in ("patched", "refreshed")
] + [
    Case("rx", rx_whole_bank_rebalance, [], moves=6, dst_calls=0, **RX_DEFAULT),
    Case("rx", rx_round_trip_and_fresh_blobs, [], moves=0),
    Case("rx", rx_alignment_after_an_import, [], dst_done=[1, 1, 1], **NO_COLLECTOR),
]

TX_DEFAULT = dict(blocks=1, after=2)
TX_CASES = [
    Case("tx", tx_fresh_destination, [], dst_calls=0, **TX_DEFAULT),
    Case("tx", tx_another_interpolation, [], **TX_DEFAULT),
    Case("tx", tx_collector_on_one_side, ["dst"], blocks=None, old=(1, 0), after=2),
    Case("tx", tx_collector_on_one_side, ["src"], dst_collector=False, **TX_DEFAULT),
    Case("tx", tx_asynchronous_continuation, ["patched"], **TX_DEFAULT),
    Case("tx", tx_asynchronous_continuation, ["refreshed"], **TX_DEFAULT),
    Case("tx", tx_int8_output, ["wave"], **TX_DEFAULT),
    Case("tx", tx_int8_output, ["valu"], **TX_DEFAULT),
    Case("tx", tx_whole_bank_rebalance, [], moves=6, dst_calls=0, **TX_DEFAULT),
    Case("tx", tx_round_trip_and_fresh_blobs, [], moves=0),
]


def check_conditions(case, run):
    """the conditions of the model test: every move of the run is in the state the case is named for"""
    e = case.expect
    assert len(run.moves) == e.get("moves", 1), (case.id, len(run.moves))
    for m in run.moves:
        who = (case.id, m["src"].name, m["s"], m["dst"].name, m["d"])
        if e["blocks"] is None:
            assert not m["has_col"] and m["open_blocks"] == 0, who
        else:
            assert m["has_col"] and m["open_blocks"] >= e["blocks"], (who, m["open_blocks"])
        if "old" in e:
            assert m["old_open_blocks"] >= e["old"][0] and m.get("old_held", 0) >= e["old"][1], (who, m["old_open_blocks"], m.get("old_held"))
        if "dst_collector" in e:  # (whether the destination bank had a collector before the import)
            assert m["dst_has_col"] == e["dst_collector"], who
        if "dst_calls" in e:
            assert m["dst_calls"] == e["dst_calls"], (who, m["dst_calls"])
        for key in ("src_done", "dst_done"):
            if key in e:
                assert m[key] == e[key], (who, key, m[key])
        assert len(m["after"]) >= e["after"], (who, len(m["after"]))
        if case.kind == "rx":
            assert e["held"][0] <= m["held"] <= e["held"][1], (who, m["held"])
            assert (0 < m["pending"] < F) == e["open_frame"], (who, m["pending"])  # (the first frame completed afterwards was opened in the source)
            if e.get("pending_mod4"):
                assert m["pending"] % 4, (who, m["pending"])
            if "words" in e:
                assert m["after"][:len(e["words"])] == [tuple(w) for w in e["words"]], (who, m["after"])
