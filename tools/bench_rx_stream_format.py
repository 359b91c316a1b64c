#!/usr/bin/env python3
"""A host-fed bank whose radios differ in format -- 8 streams, half RTL-SDR (u8) and half int16 -- through submit_ragged /
collect_ragged: 16 blocks of 65 536 samples per batch, packed input in pinned memory used in place, three batches in flight,
decimate16_cen.  Three ways:
  a   one bank with sdrhip_rx_set_stream_format (K0x): 2 bytes per u8 sample and 4 per int16 sample cross the link
  b   one int16 bank, the u8 rows widened by numpy on the host into the pinned buffer, the host's time included: the way out
      without the setter that keeps one launch chain (4 bytes per sample cross the link)
  c   two banks on one context, one per format: the way out that keeps the link bytes (two launch chains per batch)
Then K0x against K0p on the same batch in the same process (an array of equal entries against the bank-wide format, all-int16 and
all-u8: host ms per batch and the convert class's kernel time), and the synchronous device-memory call with the array set against
the same call bank-wide int16 (the extra pass over the int16 rows).
The variants alternate round by round in one process; a round is eight batches back to back with three in flight, from an idle
pipe to an idle pipe, on the host's clock from the first submit to the last collect; the figure is host ms per batch, the median
over --rounds rounds.  Prints one JSON line; --out FILE writes the table too.

    python tools/bench_rx_stream_format.py [--rounds N] [--blocks B] [--block-samples N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, L, R, DEPTH = 8, 4, 8, 3
K_CONVERT = 4


class Feed:
    """one bank and its ring of pinned batch buffers (DEPTH + 1: a buffer is reused once its batch was collected).  fmts: the
    formats the bank's rows cross the link in; widen: the streams whose rows are u8 at the source and widened by the host"""

    def __init__(self, sd, ctx, fmts, per_stream, blocks, n, widen=()):
        self.ctx, self.blocks, self.n, self.widen = ctx, blocks, n, list(widen)
        S_ = len(fmts)
        self.rx = sd.RxPipe(ctx, S_, log2decim=L, fcpos=sd.FC_CEN, nb_fec=R,
                            input_format=fmts[0] if not per_stream else "s16")
        if per_stream:
            self.rx.set_stream_formats(fmts)
        self.packed_u8 = per_stream or fmts[0] != "s16"
        self.rx.set_async(depth=DEPTH, blocks=blocks)
        self.row_bytes = [n * (4 if f == "s16" else 2) for f in fmts]
        self.block_bytes = sum(self.row_bytes)
        self.counts = [n] * S_
        rs = np.random.RandomState(1)
        self.src_u8 = rs.randint(0, 256, size=(n, 2)).astype(np.uint8)  # what a widened stream's radio delivers per block
        self.ring = []
        for _ in range(DEPTH + 1):
            buf = ctx.host_alloc((blocks * self.block_bytes,), np.uint8)
            buf[:] = np.frombuffer(rs.bytes(buf.size), np.uint8)
            self.ring.append(buf)
        self.at = 0
        self.in_flight = 0

    def submit_batch(self):
        buf = self.ring[self.at % len(self.ring)]
        self.at += 1
        for j in range(self.blocks):
            blk = buf[j * self.block_bytes:(j + 1) * self.block_bytes]
            off = 0
            for s, rb in enumerate(self.row_bytes):
                if s in self.widen:  # (the host's share of way b: u8 -> int16 into the pinned row)
                    np.subtract(self.src_u8, 128, out=blk[off:off + rb].view(np.int16).reshape(-1, 2), dtype=np.int16, casting="unsafe")
                off += rb
            self.rx.submit_ragged(blk if self.packed_u8 else blk.view(np.int16), self.counts, 1, 2)
        self.in_flight += 1

    def collect(self):
        fr = self.rx.collect_ragged()
        self.in_flight -= 1
        return sum(f.shape[0] for f in fr)

    def free(self):
        while self.in_flight:
            self.collect()
        for b in self.ring:
            self.ctx.host_free(b)


PER_ROUND = 8  # batches of a round


def one_round(feeds):
    """PER_ROUND batches through every feed of a variant, DEPTH in flight, from an idle pipe to an idle pipe (nothing of a round
    runs beside another variant's round) -> host ms per batch"""
    t0 = time.perf_counter()
    for _ in range(PER_ROUND):
        for f in feeds:
            f.submit_batch()
        for f in feeds:
            if f.in_flight == DEPTH:
                f.collect()
    for f in feeds:
        while f.in_flight:
            f.collect()
    return (time.perf_counter() - t0) * 1e3 / PER_ROUND


def median_rounds(variants, rounds):
    """variants: name -> list of feeds served per round; the variants alternate round by round"""
    ms = {k: [] for k in variants}
    for r in range(rounds + 3):
        for name, feeds in variants.items():
            v = one_round(feeds)
            if r >= 3:  # (three rounds of warm-up: buffers grown, clocks up)
                ms[name].append(v)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-samples", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd

    ctx = sd.Context(0)
    n, B = a.block_samples, a.blocks
    mixed = ["u8"] * (S // 2) + ["s16"] * (S // 2)
    lines, res = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("rx stream format A/B: %d streams (%s), %d blocks of %d samples per batch, %d batches in flight, decimate16_cen, nb_fec %d, median of %d rounds"
        % (S, " ".join(mixed), B, n, DEPTH, R, a.rounds))
    # ---- the three ways
    fa = Feed(sd, ctx, mixed, True, B, n)
    fb = Feed(sd, ctx, ["s16"] * S, False, B, n, widen=range(S // 2))
    fc = [Feed(sd, ctx, ["u8"] * (S // 2), False, B, n), Feed(sd, ctx, ["s16"] * (S // 2), False, B, n)]
    up = {"a": B * fa.block_bytes, "b": B * fb.block_bytes, "c": B * sum(f.block_bytes for f in fc)}
    h0 = ctx.counter("h2d_bytes")
    fa.submit_batch()
    fa.collect()
    assert ctx.counter("h2d_bytes") - h0 == up["a"], "way a uploads exactly sum n * bytes(fmt)"
    m = median_rounds({"a": [fa], "b": [fb], "c": fc}, a.rounds)
    for k in "abc":
        samples = S * B * n
        say("  %s  %8.3f ms per batch (min %.3f, max %.3f)  %6.2f G samples/s  upload %d bytes" % (k, m[k][0], m[k][1], m[k][2], samples / m[k][0] / 1e6, up[k]))
        res[k] = {"ms": m[k][0], "min": m[k][1], "max": m[k][2], "h2d_bytes": up[k]}
    say("  a / b = %.3f (uploaded bytes: %.3f)   a / c = %.3f" % (m["a"][0] / m["b"][0], up["a"] / up["b"], m["a"][0] / m["c"][0]))
    for f in [fa, fb] + fc:
        f.free()
    # ---- K0x against K0p on the same batch
    for fmt in ("s16", "u8"):
        fp, fx = Feed(sd, ctx, [fmt] * S, False, B, n), Feed(sd, ctx, [fmt] * S, True, B, n)
        m = median_rounds({"K0p": [fp], "K0x": [fx]}, a.rounds)
        kt = {"K0p": [], "K0x": []}
        for _ in range(5):  # (the convert class's own time, timers on: five alternating repetitions of ten batches each)
            for name, f in (("K0p", fp), ("K0x", fx)):
                ctx.kernel_timing(True)
                ctx.kernel_timing_read(K_CONVERT)
                for _ in range(10):
                    f.submit_batch()
                    f.collect()
                ctx.synchronize()
                tm, cnt = ctx.kernel_timing_read(K_CONVERT)
                ctx.kernel_timing(False)
                kt[name].append(tm / max(cnt, 1))
        say("  all-%s batch: K0p %.3f ms per batch (min %.3f, max %.3f), K0x %.3f (min %.3f, max %.3f)"
            % (fmt, m["K0p"][0], m["K0p"][1], m["K0p"][2], m["K0x"][0], m["K0x"][1], m["K0x"][2]))
        say("    unpack launch, us per launch, five repetitions: K0p %s   K0x %s"
            % (" ".join("%.2f" % (1e3 * v) for v in kt["K0p"]), " ".join("%.2f" % (1e3 * v) for v in kt["K0x"])))
        res["all_" + fmt] = {"K0p_ms": m["K0p"][0], "K0x_ms": m["K0x"][0], "K0p_kernel_us": [1e3 * v for v in kt["K0p"]],
                             "K0x_kernel_us": [1e3 * v for v in kt["K0x"]]}
        fp.free()
        fx.free()
    # ---- the synchronous device-memory call: the array set (K0x copies the int16 rows) against bank-wide int16 (read in place)
    nd = 4 * n
    x = torch.randint(-32768, 32767, (S, nd, 2), dtype=torch.int16, device="cuda")
    rows = x.view(torch.uint8).reshape(S, -1)
    plain = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    withx = sd.RxPipe(ctx, S, log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    withx.set_stream_formats(["s16"] * S)
    ms = {"bank-wide": [], "array": []}
    for r in range(a.rounds + 3):
        for name, rx, arg in (("bank-wide", plain, x), ("array", withx, rows)):
            ctx.synchronize()
            t0 = time.perf_counter()
            rx.process_view_ragged(arg, [nd] * S, 1, 2)
            ctx.synchronize()
            if r >= 3:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    mp, mx = statistics.median(ms["bank-wide"]), statistics.median(ms["array"])
    say("  synchronous device call, %d x %d int16 samples: bank-wide %.3f ms (min %.3f, max %.3f), array set %.3f ms (min %.3f, max %.3f): +%.3f ms"
        % (S, nd, mp, min(ms["bank-wide"]), max(ms["bank-wide"]), mx, min(ms["array"]), max(ms["array"]), mx - mp))
    res["sync_device"] = {"bank_wide_ms": mp, "array_ms": mx}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
