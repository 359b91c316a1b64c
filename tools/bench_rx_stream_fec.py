#!/usr/bin/env python3
"""A hub of 64 streams whose clients want different fecblk -- 4, 8, 16 and 32 on 16 streams each -- through
submit_datagrams_tagged + collect_egress (departure order, lent buffers), three ways:
  A   four banks of 16 streams, one per fecblk value: the work-around without sdrhip_rx_set_stream_fec (four launch chains and four
      departure-order arrays per batch)
  A2  the same again, a handle set of its own: the A/A pair, whose spread is the noise floor
  B   one bank of 64 streams with the array (one launch chain, one array; KR delivers)
  C   one bank of 64 streams at a uniform fecblk 32 (KR delivers, one run per frame; more recovery blocks than B computes and sends)
Every stream receives --frames whole frames per batch (incoming fecblk 4, nothing lost, decimate1), so every batch releases and
delivers that many frames per stream; the same arrival-order array is submitted again with its frame indices moved on.
The variants run interleaved in rounds of at least --window seconds of back-to-back batches (submit, collect, release, move the
frame indices on: one batch in flight, the pinned input is free again once its batch is collected); the figure is host ms per
batch, median over the rounds.
Then, on B and C alone, the delivery kernel's own time (kernel timers, class K_CONVERT, untagged submits so that nothing else of
the batch runs in that class) per datagram, and the bytes one batch brings down ("d2h_bytes").  Prints one JSON line.

    python tools/bench_rx_stream_fec.py [--rounds N] [--window SECONDS] [--frames F] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S, R_IN = 64, 4
FEC = [4, 8, 16, 32]
PER = S // len(FEC)


def arrival(orc, rs, nstreams, frames):
    """`frames` whole frames per stream, interleaved datagram by datagram as a socket delivers them: ((n, 512) uint8, tags (n,))"""
    per = []
    for s in range(nstreams):
        rows = []
        for f in range(frames):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            rows.append(np.concatenate([fr, orc.frame_encode(fr, R_IN)]))
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
        if name in ("A", "A2"):
            for i, r in enumerate(FEC):
                self.banks.append((sd.RxPipe(self.ctx, PER, log2decim=0, nb_fec=r), i * PER, PER))
        elif name == "B":
            rx = sd.RxPipe(self.ctx, S, log2decim=0, nb_fec=8)
            rx.set_stream_fec([r for r in FEC for _ in range(PER)])
            self.banks.append((rx, 0, S))
        else:
            self.banks.append((sd.RxPipe(self.ctx, S, log2decim=0, nb_fec=32), 0, S))
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

    def batch(self, tagged=True):
        for (rx, _, n), (a, t, a16) in zip(self.banks, self.inputs):
            if tagged:
                rx.submit_datagrams_tagged(a, t, 1, 2)
            else:  # (the arrival order here is stream-minor: the packed form is its transpose, made once per call -- kernel timing only)
                rx.submit_datagrams([np.ascontiguousarray(a[s::n]) for s in range(n)], 1, 2)
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
    ap.add_argument("--frames", type=int, default=2, help="frames per stream and batch")
    ap.add_argument("--timed-batches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first)

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle

    if sd.device_count() <= 0:
        raise SystemExit("bench_rx_stream_fec: no GPU")
    arr, tags = arrival(Oracle(), np.random.RandomState(1), S, args.frames)
    names = ["A", "B", "C", "A2"]
    v = {n: Variant(sd, n, args.frames, arr, tags) for n in names}

    def one(x, tagged=True):
        x.batch(tagged)
        x.drain()
        x.advance()

    for x in v.values():  # steady state: every later batch releases and delivers `frames` frames per stream
        for _ in range(3):
            one(x)
        assert all(list(g[2]) == [args.frames] * n for g, (_, _, n) in zip(x.last, x.banks)), (x.name, [list(g[2]) for g in x.last])

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
    # ---- one batch's download, and the delivery kernel alone
    d2h, dgrams, k_us = {}, {}, {}
    for n in ("A", "B", "C"):
        x = v[n]
        d0 = x.ctx.counter("d2h_bytes")
        one(x)
        d2h[n] = x.ctx.counter("d2h_bytes") - d0
        dgrams[n] = int(sum(g[0].shape[0] for g in x.last))
    for n in ("B", "C"):
        x = v[n]
        one(x, tagged=False)
        x.ctx.kernel_timing(True)
        x.ctx.kernel_timing_read(sd.engine.K_CONVERT)
        for _ in range(args.timed_batches):
            one(x, tagged=False)
        kms, kn = x.ctx.kernel_timing_read(sd.engine.K_CONVERT)
        x.ctx.kernel_timing(False)
        k_us[n] = dict(launches=kn, us_per_launch=round(kms / max(kn, 1) * 1e3, 3), ns_per_dgram=round(kms / max(kn, 1) * 1e6 / dgrams[n], 3))
    res = dict(bench="rx_stream_fec",
               workload="64 streams, fecblk 4 / 8 / 16 / 32 on 16 each, %d frames per stream and batch in (fecblk 4, nothing lost), decimate1, "
                        "submit_datagrams_tagged + collect_egress(copy=False), one batch in flight" % args.frames,
               ms_per_batch_median=med, ms_per_batch_min={n: float(np.min(x)) for n, x in ms.items()},
               ms_per_batch_max={n: float(np.max(x)) for n, x in ms.items()}, rounds=ms,
               aa_spread_ms=round(abs(med["A"] - med["A2"]), 4), a_minus_b_ms=round(med["A"] - med["B"], 4), c_minus_b_ms=round(med["C"] - med["B"], 4),
               dgrams_per_batch=dgrams, d2h_bytes_per_batch=d2h, delivery_kernel=k_us)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
