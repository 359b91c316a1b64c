#!/usr/bin/env python3
"""A hub of 64 streams whose heads deliver different sample sizes -- 8 bits (RTL-SDR, HackRF), 12 (Airspy, BladeRF) and 16 -- through
submit_datagrams_tagged + collect_egress (departure order, lent buffers), decimate16_cen, three ways:
  A   three banks of 22 / 21 / 21 streams, one per sample size: the work-around without sdrhip_rx_set_stream_bits (three launch
      chains, three tagged uploads and three departure-order arrays per batch)
  A2  the same again, a handle set of its own: the A/A pair, whose spread is the noise floor
  B   one bank of 64 streams with the array (one launch chain, one upload, one array)
  C   one bank of 64 streams at a uniform 16 bits (what B costs without the array)
Every stream receives --frames whole frames per batch (incoming fecblk 4, nothing lost); 16 of them make one outgoing frame, so with
the default every batch delivers one frame per stream.  The same arrival-order array is submitted again with its frame indices moved
on.  The variants run interleaved in rounds of at least --window seconds of back-to-back batches (submit, collect, release, move the
frame indices on: one batch in flight); the figure is host ms per batch, median over the rounds.
Then, on B and C alone, the decimator launch's own time (kernel timers, class K_DECIMATE) per batch.  Prints one JSON line.

    python tools/bench_rx_stream_bits.py [--rounds N] [--window SECONDS] [--frames F] [--variants A,B,C,A2] [--out FILE]
(--variants C alone needs no per-stream entry: it also runs on a library built from the parent commit, SDRHIP_LIB_PATH, for the
decimator launch's time before and after.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S, R_IN, L, R_OUT = 64, 4, 4, 8
BITS = [8, 12, 16]
BANKS = [(0, 22), (22, 21), (43, 21)]  # A's banks: (first stream, streams), bank i at BITS[i]
STREAM_BITS = [BITS[i] for i, (_, n) in enumerate(BANKS) for _ in range(n)]


def arrival(orc, rs, nstreams, frames):
    """`frames` whole frames per stream, interleaved datagram by datagram as a socket delivers them: ((n, 512) uint8, tags (n,)).
    One random frame per stream, repeated with its frame index moved on (the decimator's work does not depend on the values)"""
    per = []
    for s in range(nstreams):
        fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
        fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = 0, 0, np.arange(128), 0
        full = np.concatenate([fr, orc.frame_encode(fr, R_IN)])
        rows = []
        for f in range(frames):
            g = full.copy()
            g[:, 0] = f
            rows.append(g)
        per.append(np.concatenate(rows))
    n = per[0].shape[0]
    arr = np.stack(per, axis=1).reshape(nstreams * n, 512)  # round j = datagram j of every stream
    tags = np.tile(np.arange(nstreams, dtype=np.uint16), n)
    return np.ascontiguousarray(arr), tags


class Variant:
    """a set of banks that together serve the 64 streams; banks[i] = (pipe, first stream, streams)"""

    def __init__(self, sd, name, frames, arr, tags):
        self.name, self.frames = name, frames
        self.ctx = sd.Context(0)
        self.banks = []
        cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R_OUT)
        if name in ("A", "A2"):
            for b, (s0, n) in zip(BITS, BANKS):
                self.banks.append((sd.RxPipe(self.ctx, n, sample_bits=b, **cfg), s0, n))
        elif name == "B":
            rx = sd.RxPipe(self.ctx, S, sample_bits=16, **cfg)
            rx.set_stream_bits(STREAM_BITS)
            self.banks.append((rx, 0, S))
        else:
            self.banks.append((sd.RxPipe(self.ctx, S, sample_bits=16, **cfg), 0, S))
        self.inputs = []
        for rx, s0, n in self.banks:
            rx.set_async(depth=1)
            rx.set_egress("round_robin")
            keep = (tags >= s0) & (tags < s0 + n)
            a = self.ctx.host_alloc((int(keep.sum()), 512), np.uint8)  # (pinned: goes up in place)
            a[:] = arr[keep]
            self.inputs.append((a, np.ascontiguousarray(tags[keep] - s0), a.view(np.uint16)))
        self.in_flight = 0
        self.last = None

    def batch(self):
        for (rx, _, n), (a, t, a16) in zip(self.banks, self.inputs):
            rx.submit_datagrams_tagged(a, t, 1, 2)
        self.in_flight += 1

    def advance(self):
        """frame indices of the next batch (the arrays are free: every batch that read them has been collected)"""
        for _, _, a16 in self.inputs:
            a16[:, 0] += self.frames

    def collect(self):
        self.last = [rx.collect_egress(copy=False) for rx, _, _ in self.banks]
        self.in_flight -= 1

    def drain(self):
        while self.in_flight:
            self.collect()
        for rx, _, _ in self.banks:
            rx.release_egress()
        self.ctx.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--frames", type=int, default=16, help="incoming frames per stream and batch (16 make one outgoing frame)")
    ap.add_argument("--timed-batches", type=int, default=20)
    ap.add_argument("--variants", default="A,B,C,A2", help="the variants to run, in this order")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first)

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle

    if sd.device_count() <= 0:
        raise SystemExit("bench_rx_stream_bits: no GPU")
    arr, tags = arrival(Oracle(), np.random.RandomState(1), S, args.frames)
    names = args.variants.split(",")
    v = {n: Variant(sd, n, args.frames, arr, tags) for n in names}

    def one(x):
        x.batch()
        x.drain()
        x.advance()

    for x in v.values():  # steady state, and the frames a batch delivers
        for _ in range(3):
            one(x)
    delivered = {n: int(sum(int(g[2].sum()) for g in x.last)) for n, x in v.items()}
    assert len(set(delivered.values())) == 1, delivered
    # (sampleBits of the first delivered meta block)
    says = sorted({int(np.asarray(g[0]).reshape(-1, 512)[0, 13]) for g in v["B"].last if g[0].shape[0]}) if "B" in v else None

    def window(x):
        x.ctx.synchronize()
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.window:
            one(x)
            n += 1
        return (time.perf_counter() - t0) / n * 1e3

    ms = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:  # (interleaved)
            ms[n].append(round(window(v[n]), 4))
    med = {n: round(float(np.median(x)), 4) for n, x in ms.items()}
    # ---- the decimator launch alone, and its plan
    k_us, plans = {}, {}
    for n in [n for n in ("B", "C") if n in v]:
        x = v[n]
        one(x)
        x.ctx.kernel_timing(True)
        x.ctx.kernel_timing_read(sd.engine.K_DECIMATE)
        for _ in range(args.timed_batches):
            one(x)
        kms, kn = x.ctx.kernel_timing_read(sd.engine.K_DECIMATE)
        x.ctx.kernel_timing(False)
        k_us[n] = dict(launches=kn, us_per_launch=round(kms / max(kn, 1) * 1e3, 3))
        plans[n] = x.banks[0][0].last_plan()

    def diff(a, b, absolute=False):
        if a not in med or b not in med:
            return None
        return round(abs(med[a] - med[b]) if absolute else med[a] - med[b], 4)

    res = dict(bench="rx_stream_bits",
               workload="64 streams, sample bits 8 / 12 / 16 on 22 / 21 / 21, %d frames per stream and batch in (fecblk 4, nothing lost), "
                        "decimate16_cen, fecblk %d out, submit_datagrams_tagged + collect_egress(copy=False), one batch in flight" % (args.frames, R_OUT),
               ms_per_batch_median=med, ms_per_batch_min={n: float(np.min(x)) for n, x in ms.items()},
               ms_per_batch_max={n: float(np.max(x)) for n, x in ms.items()}, rounds=ms,
               aa_spread_ms=diff("A", "A2", True), a_minus_b_ms=diff("A", "B"), b_minus_c_ms=diff("B", "C"),
               frames_per_batch=delivered, first_sample_bits_b=says, decimator_kernel=k_us, plan=plans)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
