"""Stream export / import (sdrhip_*_export_stream / _import_stream) in every state a stream and a bank can be in: the scenarios of
tests/migrate_cases.py made on the library, call by call, beside the reference chains.

Expected output everywhere is the UNINTERRUPTED chain of the stream (migrate_cases.RxChain: the reference's SDRdaemonFECBuffer, a
remainder buffer, the compiled-reference decimators, the oracle framer and frame_encode; migrate_cases.TxChain: the collector and the
oracle interpolators), fed as if the move had never happened and given the destination's settings from the first frame completed
after it.  Nothing is compared with the library's own output.  Every stream of both banks is checked on every call -- frames,
recovery blocks, sdrhip_rx_carry -- the exported stream still running in the source included; after every import the collector
statistics of the imported stream, and at the end those of every stream, equal the restatement's; the host's shadow of the
collectors never disagrees with the device ("fecbuf_shadow_mismatch" does not move).  Everything is byte-exact; an assertion names
the scenario, the bank, the call, the stream and the frame.

tests/test_migrate_cases_model.py asserts, without a GPU, that every move happens in the state its scenario is named for; the same
conditions are asserted here again, on the chains fed through the compiled collector."""
import numpy as np
import pytest

import migrate_cases as mc
import test_gpu_rx_datagrams as tr
import test_gpu_stream_reset as ts
import test_gpu_tx_datagrams as tt
from test_gpu_dgram_tagged import merge
from test_gpu_rx_egress import rounds
from test_gpu_stream_migrate import second_context

pytestmark = pytest.mark.gpu

ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)
reflib = tt.reflib
torch_first = ts.torch_first
EINVAL = -1
FRESH = (0, 0, 256, 0)


def first_difference(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return ("shapes", a.shape, b.shape)
    d = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
    return None if not d.size else ("first of %d differences at" % d.size, np.unravel_index(int(d[0]), a.shape))


class OnTheLibrary:
    """the part of a driver that Rx and Tx share: contexts, options, the move itself, the blobs, the collector statistics"""

    blob_kind = None

    def setup(self, ctx):
        self.ctxs, self.saved, self.blobs = {0: ctx}, [], []
        self.shadow0 = {}

    def ctx_of(self, i):
        if i not in self.ctxs:
            self.ctxs[i] = second_context()
        c = self.ctxs[i]
        if i not in self.shadow0:
            self.shadow0[i] = c.counter("fecbuf_shadow_mismatch")
        return c

    def option(self, ctx, key, value):
        c = self.ctx_of(ctx)
        self.saved.append((c, key, c.option(key)))
        c.set_option(key, value)

    def restore(self):
        """every option back to what it was before the scenario set it (also behind a failed assertion)"""
        for c, key, old in reversed(self.saved):
            if old is not None:
                c.set_option(key, old)
        self.saved = []

    def check_stats(self, b, s):
        st, m = b.pipe.collector_stats(s), b.chains[s].col.model
        got = (st["cur_nb_blocks"], st["cur_nb_recovery"], st["min_nb_blocks"], st["max_nb_recovery"])
        exp = (m.b.s.cur_nb_blocks, m.b.s.cur_nb_recovery, m.b.s.min_nb_blocks, m.b.s.max_nb_recovery)
        assert got == exp, (self.where(b, s), "collector statistics", got, exp)
        assert st["current_meta"][:20] == m.cur_meta and st["output_meta"][:20] == m.out_meta, (self.where(b, s), "collector metas")
        m.b.s.min_nb_blocks, m.b.s.max_nb_recovery = 256, 0  # (the getters reset them)
        return got

    def after_import(self, b, s):
        pass

    def on_move(self, src, s, dst, d):
        blob = src.pipe.export_stream(s)
        assert blob[:4] == b"SDRS" and int.from_bytes(blob[8:12], "little") == self.blob_kind and int.from_bytes(blob[12:16], "little") == len(blob)
        dst.pipe.import_stream(d, blob)
        self.blobs.append(blob)
        dst.unaligned = True
        if dst.has_col or src.has_col:
            got = self.check_stats(dst, d)
            if not src.has_col:  # (a blob without a collector: the constructor's collector state)
                assert got == FRESH, (self.where(dst, d), got)
        dst.has_col = dst.has_col or src.has_col
        self.after_import(dst, d)

    def roundtrip(self, b, s):
        first = b.pipe.export_stream(s)
        b.pipe.import_stream(s, first)
        again = b.pipe.export_stream(s)
        assert first == again, (self.where(b, s), "round trip", first_difference(np.frombuffer(first, np.uint8), np.frombuffer(again, np.uint8)))
        self.after_import(b, s)

    def reset(self, b, s):
        self.restart(b, s)
        b.pipe.reset_streams([s])

    def fresh_blobs_equal(self, b, s_reset, s_unused):
        a, u = b.pipe.export_stream(s_reset), b.pipe.export_stream(s_unused)
        assert a == u, (self.where(b, s_reset), "a reset stream's blob against a never-used stream's",
                        first_difference(np.frombuffer(a, np.uint8), np.frombuffer(u, np.uint8)))

    def import_fresh_blob(self, b, s, s_unused):
        self.restart(b, s)
        b.pipe.import_stream(s, b.pipe.export_stream(s_unused))
        assert self.check_stats(b, s) == FRESH
        self.after_import(b, s)

    def finish(self):
        for b in self.banks:
            assert not b.queue, b.name
            if b.has_col:
                for s in range(b.S):
                    self.check_stats(b, s)
        for i, c in self.ctxs.items():
            if i in self.shadow0:
                assert c.counter("fecbuf_shadow_mismatch") == self.shadow0[i], (self.case, "context", i)


class RxOnTheLibrary(OnTheLibrary, mc.RxRun):
    blob_kind = 1

    def on_bank(self, b):
        import sdrdaemon_amd as sd

        b.pipe = sd.RxPipe(self.ctx_of(b.ctx), b.S, log2decim=b.L, fcpos=b.fcpos, hb_variant=b.hb, nb_fec=b.R)
        b.unaligned = False
        if b.fec:
            b.pipe.set_stream_fec(b.fec)
            for s in range(b.S):
                assert b.pipe.stream_fec(s) == (b.fec[s], 128 + max(b.fec))
        if b.meta:
            b.pipe.set_stream_meta([m[0] for m in b.meta], [m[1] for m in b.meta])
        if b.follow:
            b.pipe.set_follow_meta(True)
        if b.depth:
            b.pipe.set_async(depth=b.depth)
        if b.egress:
            b.pipe.set_egress("round_robin")

    def check_carry(self, b):
        if b.has_col:
            assert list(b.pipe.carry()) == [c.held for c in b.chains], (self.where(b), "carry")

    def after_import(self, b, s):
        self.check_carry(b)

    def check_frames(self, b, got, exp):
        assert len(got) == b.S
        for s in range(b.S):
            tr.check_frames(np.asarray(got[s]), exp[s], self.where(b, s))

    def on_dgrams(self, b, chunk, sec, usec, device, exp):
        got = tr.run_call(b.pipe, chunk, sec, usec, device=device)
        self.check_frames(b, [g[0] for g in got], exp)
        self.check_carry(b)

    def on_ragged(self, b, xs, sec, usec, uniform, exp):
        counts = [len(x) for x in xs]
        if uniform:
            out = b.pipe.process(np.stack(xs), sec, usec)
            nf = [v.shape[0] for v in b.pipe.frames_view_ragged()] if b.unaligned else [out.shape[1]] * b.S
            got = [np.asarray(out[s])[:nf[s]] for s in range(b.S)]
        else:
            rows = np.zeros((b.S, max(max(counts), 1), 2), np.int16)
            for s, x in enumerate(xs):
                rows[s, :counts[s]] = x
            out, nf = b.pipe.process_ragged(rows, counts, sec, usec)
            got = [np.asarray(out[s])[:int(nf[s])] for s in range(b.S)]
            b.unaligned = True
        assert [int(n) for n in nf] == [len(e) for e in exp], (self.where(b), [int(n) for n in nf], [len(e) for e in exp])
        self.check_frames(b, got, exp)
        self.check_carry(b)  # (sample-fed calls neither read nor clear the remainder)

    def on_submit(self, b, chunk, sec, usec, tagged):
        if tagged is None:
            b.pipe.submit_datagrams(chunk, sec, usec)
        else:
            arr, tags = merge(chunk, tagged, skip=3)
            b.pipe.submit_datagrams_tagged(arr, tags, sec, usec)

    def on_collect(self, b, exp):
        if b.egress:
            dg, tags, nf, _ = b.pipe.collect_egress()
            blocks = 128 + b.R
            frames = [np.stack(e) if e else np.zeros((0, blocks, 512), np.uint8) for e in exp]
            exp_dg, exp_tags = rounds(frames)
            assert list(nf) == [len(e) for e in exp], (self.where(b), list(nf), [len(e) for e in exp])
            assert not len(exp_dg) or b.pipe.last_blocks_per_frame == blocks, (self.where(b), b.pipe.last_blocks_per_frame)
            assert np.array_equal(tags, exp_tags), (self.where(b), "tags", first_difference(tags, exp_tags))
            bad = first_difference(dg, exp_dg)
            if bad and bad[0] != "shapes":  # (stream, frame and block of the first wrong datagram)
                k = int(bad[1][0])
                s = int(exp_tags[k])
                j = int(np.count_nonzero(exp_tags[:k] == s))
                bad = bad + ("stream %d" % s, "frame %d" % (j // blocks), "block %d" % (j % blocks))
            assert bad is None, (self.where(b), "egress array", bad)
        else:
            got = b.pipe.collect_datagrams()
            self.check_frames(b, [g[0] for g in got], exp)
        if not b.queue:
            self.check_carry(b)

    def assert_path(self, b, path):
        assert b.pipe.last_plan()["path"] == path, (self.where(b), b.pipe.last_plan())

    def assert_refusals_of_an_unaligned_bank(self, b, xs):
        import sdrdaemon_amd as sd

        with pytest.raises(sd.SdrHipError) as e:
            sd.engine.check(b.pipe.ctx.lib.sdrhip_rx_set_pipelined(b.pipe.h, 1))
        assert e.value.code == EINVAL, e.value
        b.pipe.set_async(depth=2, blocks=1)
        with pytest.raises(sd.SdrHipError) as e:
            b.pipe.submit(np.stack(xs), 9, 9)
        assert e.value.code == EINVAL, e.value
        assert b.pipe.collect(wait=False) is None  # (nothing was consumed: the calls that follow continue the chains)


class TxOnTheLibrary(OnTheLibrary, mc.TxRun):
    blob_kind = 2

    def on_bank(self, b):
        import sdrdaemon_amd as sd

        b.pipe = sd.TxPipe(self.ctx_of(b.ctx), b.S, b.L, output_format=b.fmt)
        if b.depth:
            b.pipe.set_async(b.depth)

    def check_samples(self, b, got, exp):
        assert len(got) == b.S
        for s in range(b.S):
            e = exp[s] if b.fmt == "s16" else np.right_shift(exp[s], 8).astype(np.int8)  # ("s8": v >> 8 of each component)
            g = np.asarray(got[s])
            assert g.dtype == e.dtype and g.shape == e.shape, (self.where(b, s), g.shape, e.shape)
            assert np.array_equal(g, e), (self.where(b, s), first_difference(g, e), "frame %d" % (first_difference(g, e)[1][0] // (mc.F << b.L)))

    def on_dgrams(self, b, chunk, device, exp):
        got, = tt.run_calls(b.pipe, [chunk], device=device)
        self.check_samples(b, [g[0] for g in got], exp)

    def on_process(self, b, frames, exp):
        out = b.pipe.process(np.stack([np.stack(f) for f in frames]))
        self.check_samples(b, [out[s] for s in range(b.S)], exp)

    def on_submit(self, b, chunk, tagged):
        if tagged is None:
            b.pipe.submit_datagrams(chunk)
        else:
            arr, tags = merge(chunk, tagged, skip=3)
            b.pipe.submit_datagrams_tagged(arr, tags)

    def on_collect(self, b, exp):
        got = b.pipe.collect_datagrams()
        self.check_samples(b, [tt.as_np(g[0]) for g in got], exp)


def drive(run, case, ctx):
    run.setup(ctx)
    try:
        case.run(run)
    finally:
        run.restore()
    mc.check_conditions(case, run)


@pytest.mark.parametrize("case", mc.RX_CASES, ids=lambda c: c.id)
def test_rx_stream_moves(oracle, ctx, reflib, case):
    """the Rx scenarios 1 .. 11 of tests/migrate_cases.py (the docstring of each rx_* function there says what the state is)"""
    drive(RxOnTheLibrary(oracle, reflib, case.id), case, ctx)


@pytest.mark.parametrize("case", mc.TX_CASES, ids=lambda c: c.id)
def test_tx_stream_moves(oracle, ctx, reflib, case):
    """the Tx scenarios 1 .. 7 of tests/migrate_cases.py"""
    drive(TxOnTheLibrary(oracle, reflib, case.id), case, ctx)


def test_the_destination_encoder_forms_are_all_hit(ctx):
    """scenario 5's counts give one stream per encoder form with the enc_min_rows in force: no recovery blocks, at most 32 (the FFT
    form), more (the walk)"""
    lo = int(ctx.option("enc_min_rows", 1))
    r0, r1, r2 = mc.DST_FEC
    assert r0 == 0 and lo <= r1 <= 32 < r2, (lo, mc.DST_FEC)
