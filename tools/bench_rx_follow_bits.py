#!/usr/bin/env python3
"""The Rx pipe fed datagrams with the sample size following the incoming meta blocks (sdrhip_rx_set_follow_bits) against the same
pipe with the flag off, on the hub's shape of tools/bench_rx_follow_meta.py (whose handle, batch shape and parent loader this tool
uses): 8 streams x 64 released frames per call, incoming fecblk 32 with 24 erasures per frame, decimate16_cen, outgoing nb_fec 32.
Block 0 of every incoming frame is a meta block; its sampleBits byte says 8, 12 or 16 by stream (an RTL-SDR / HackRF, an Airspy /
BladeRF and a test-source head), the hub's configuration says 16.

Callers, each a handle of its own, in alternating rounds in one process:
  sync_off / sync_on     sdrhip_rx_process_datagrams, device memory
  async_off / async_on   sdrhip_rx_submit_datagrams / _collect_datagrams, packed pinned host memory in place, --depth batches in flight
  parent_sync / parent_async   (--parent-lib FILE) the same two entries of a library built from the parent commit, loaded beside
                         the product with a context of its own: the yardstick for flag off
A round is a window of at least --window seconds of back-to-back calls (batches), the clock stops behind a device synchronisation;
its figure is ms per call.  Prints one JSON line: median and min..max per caller, the rounds, on minus off, off minus parent and
the parent's own round-to-round spread (the only noise figure the setup gives: the margin for "flag off costs nothing").

    python tools/bench_rx_follow_bits.py [--rounds N] [--window SECONDS] [--depth D] [--parent-lib FILE] [--out FILE]
    python tools/bench_rx_follow_bits.py --only sync_on --calls 20     one caller alone, a fixed number of calls behind the warm-up:
        for `rocprofv3 --kernel-trace --stats -- python tools/...` (counters in a run of their own)"""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_rx_follow_meta as bm  # noqa: E402  (puts the repository and tests/ on the path)

S, F, R_IN, LOST = bm.S, bm.F, bm.R_IN, bm.LOST
HEAD_BITS = [8, 12, 16, 8, 12, 16, 8, 12]
ENTRIES = bm.ENTRIES


def meta_block(fc, rate, bits, f):
    """block 0 behind its header: the 24-byte MetaDataFEC of an undecimated stream of that sample size, then zeros"""
    m = struct.pack("<IIBBBBII", fc, rate, (bits - 1) // 8 + 1, bits, 128, R_IN, 1000 + f, 0)
    return np.frombuffer(m + struct.pack("<I", zlib.crc32(m)) + bytes(508 - 24), np.uint8)


def batch(orc, rs):
    """bench_rx_follow_meta.batch with each stream's head saying its own size"""
    rows, counts = [], []
    for s in range(S):
        n = 0
        for f in range(F):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            fr[0, 4:] = meta_block(435000 + 1000 * s, 10000000 - 100000 * s, HEAD_BITS[s], f)
            allb = np.concatenate([fr, orc.frame_encode(fr, R_IN)])
            keep = sorted(set(range(128 + R_IN)) - set(rs.choice(128 + R_IN, LOST, replace=False).tolist()))
            rows.append(allb[keep])
            n += len(keep)
        counts.append(n)
    return np.concatenate(rows), counts


class Handle(bm.Handle):
    """bench_rx_follow_meta.Handle with the other flag"""

    def __init__(self, lib, follow, dg, counts, depth):
        bm.Handle.__init__(self, lib, False, dg, counts, depth)
        if follow:
            self.check(lib.sdrhip_rx_set_follow_bits(self.rx, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libsdrhip.so built from the parent commit")
    ap.add_argument("--only", default=None, help="one caller alone (kernel-trace runs)")
    ap.add_argument("--calls", type=int, default=20, help="calls of the --only caller")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first: both libraries bind to it)

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle

    if sd.device_count() <= 0:
        raise SystemExit("bench_rx_follow_bits: no GPU")
    product = sd._lib.lib()
    dg, counts = batch(Oracle(), np.random.RandomState(1))
    spec = dict(sync_off=(product, False, "sync"), sync_on=(product, True, "sync"), async_off=(product, False, "async"),
                async_on=(product, True, "async"))
    if args.parent_lib:
        parent = bm.open_parent(args.parent_lib, product)
        spec.update(parent_sync=(parent, False, "sync"), parent_async=(parent, False, "async"))
    if args.only:
        spec = {args.only: spec[args.only]}
    handles, callers = {}, {}
    for name, (lib, follow, entry) in spec.items():
        h = handles[name] = Handle(lib, follow, dg, counts, args.depth)
        callers[name] = h.call_sync if entry == "sync" else h.call_async
    for name, fn in callers.items():  # steady state: every later call releases the batch's F frames per stream
        for _ in range(max(args.warmup, 2)):
            fn()
        handles[name].drain()
        assert list(handles[name].nr) == [F] * S, (name, list(handles[name].nr))
    frames_out = {k: [int(x) for x in h.nf] for k, h in handles.items()}

    def window(name):
        h, fn = handles[name], callers[name]
        h.sync()
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.window:
            fn()
            n += 1
        h.drain()
        return (time.perf_counter() - t0) / n * 1e3

    if args.only:
        for _ in range(args.calls):
            callers[args.only]()
        handles[args.only].drain()
        res = dict(bench="rx_follow_bits", only=args.only, calls=args.calls, frames_out_per_call=frames_out)
    else:
        ms = {k: [] for k in callers}
        for _ in range(args.rounds):
            for k in callers:  # (alternating)
                ms[k].append(round(window(k), 4))
        med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
        res = dict(bench="rx_follow_bits",
                   workload="rx datagrams: 8 streams x 64 released frames per call, fecblk 32 in, 24 erasures per frame, meta blocks in that say "
                            "8 / 12 / 16 bits by stream, decimate16_cen, nb_fec 32 out; sync: device memory, async: packed pinned host memory, "
                            "depth %d" % args.depth,
                   ms_per_call_median=med, ms_per_call_min={k: float(np.min(v)) for k, v in ms.items()},
                   ms_per_call_max={k: float(np.max(v)) for k, v in ms.items()}, rounds=ms,
                   on_minus_off_us={e: round((med[e + "_on"] - med[e + "_off"]) * 1e3, 2) for e in ("sync", "async")},
                   frames_out_per_call=frames_out)
        if args.parent_lib:
            res["off_minus_parent_us"] = {e: round((med[e + "_off"] - med["parent_" + e]) * 1e3, 2) for e in ("sync", "async")}
            res["parent_spread_us"] = {e: round((max(ms["parent_" + e]) - min(ms["parent_" + e])) * 1e3, 2) for e in ("sync", "async")}
    for h in handles.values():
        h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
