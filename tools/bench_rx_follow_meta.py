#!/usr/bin/env python3
"""The Rx pipe fed datagrams with the outgoing meta following the incoming meta blocks (sdrhip_rx_set_follow_meta) against the same
pipe with the flag off, on the hub's shape of tools/bench_rx_datagrams.py: 8 streams x 64 released frames per call, incoming fecblk
32 with 24 erasures per frame in a different pattern each, decimate16_cen, outgoing nb_fec 32.  Block 0 of every incoming frame is
a meta block (each stream its own frequency and rate), lost with the others' probability and then repaired.

Callers, each a handle of its own, in alternating rounds in one process:
  sync_off / sync_on     sdrhip_rx_process_datagrams, device memory
  async_off / async_on   sdrhip_rx_submit_datagrams / _collect_datagrams, packed pinned host memory in place, --depth batches in flight
  parent_sync / parent_async   (--parent-lib FILE) the same two entries of a library built from the parent commit, loaded beside
                         the product with a context of its own: the yardstick for flag off
A round is a window of at least --window seconds of back-to-back calls (batches), the clock stops behind a device synchronisation;
its figure is ms per call.  Prints one JSON line: median and min..max per caller, the rounds, on minus off.

    python tools/bench_rx_follow_meta.py [--rounds N] [--window SECONDS] [--depth D] [--parent-lib FILE] [--out FILE]
    python tools/bench_rx_follow_meta.py --only sync_on --calls 20     one caller alone, a fixed number of calls behind the warm-up:
        for `rocprofv3 --kernel-trace --stats -- python tools/...` (counters in a run of their own)"""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S, F, R_IN, LOST, L2, R_OUT = 8, 64, 32, 24, 4, 32
SPF = 16129
P = C.c_void_p
# the entries a caller uses: the parent library gets the product's prototypes for them
ENTRIES = ["sdrhip_last_error", "sdrhip_ctx_create", "sdrhip_ctx_destroy", "sdrhip_ctx_synchronize", "sdrhip_rx_create", "sdrhip_rx_destroy",
           "sdrhip_rx_max_frames", "sdrhip_rx_set_async", "sdrhip_rx_process_datagrams", "sdrhip_rx_submit_datagrams",
           "sdrhip_rx_collect_datagrams", "sdrhip_host_alloc", "sdrhip_host_free"]


def meta_block(fc, rate, f):
    """block 0 behind its header: the 24-byte MetaDataFEC of an undecimated 16-bit stream, then zeros"""
    m = struct.pack("<IIBBBBII", fc, rate, 2, 16, 128, R_IN, 1000 + f, 0)
    return np.frombuffer(m + struct.pack("<I", zlib.crc32(m)) + bytes(508 - 24), np.uint8)


def batch(orc, rs):
    """per stream F frames (frame indices 0 .. F - 1) with LOST random losses each, packed in arrival order: ([n][512], counts)"""
    rows, counts = [], []
    for s in range(S):
        n = 0
        for f in range(F):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            fr[0, 4:] = meta_block(435000 + 1000 * s, 10000000 - 100000 * s, f)
            allb = np.concatenate([fr, orc.frame_encode(fr, R_IN)])
            keep = sorted(set(range(128 + R_IN)) - set(rs.choice(128 + R_IN, LOST, replace=False).tolist()))
            rows.append(allb[keep])
            n += len(keep)
        counts.append(n)
    return np.concatenate(rows), counts


class Handle:
    """one library (the product's, or the parent's beside it), one context, one Rx bank, through the C entries alone"""

    def __init__(self, lib, follow, dg, counts, depth):
        from sdrdaemon_amd._lib import RxConfig

        self.lib, self.depth = lib, depth
        self.ctx, self.rx = P(), P()
        self.check(lib.sdrhip_ctx_create(0, P(0), C.byref(self.ctx)))
        cfg = RxConfig(L2, 2, 0, 16, R_OUT, 435000, 625000)
        self.check(lib.sdrhip_rx_create(self.ctx, S, C.byref(cfg), C.byref(self.rx)))
        if follow:
            self.check(lib.sdrhip_rx_set_follow_meta(self.rx, 1))
        self.nd = (C.c_size_t * S)(*counts)
        assert len(set(counts)) == 1  # (every frame loses LOST datagrams: the packed rows are also rows of one stride)
        self.stride = counts[0] * 512
        self.maxr = F + 1
        self.info = (C.c_int * (4 * S * self.maxr))()
        self.nr, self.nf = (C.c_size_t * S)(), (C.c_size_t * S)()
        self.sec, self.usec = (C.c_uint32 * S)(*[1] * S), (C.c_uint32 * S)()
        self.fb = (128 + R_OUT) * 512
        self.cap = max(int(lib.sdrhip_rx_max_frames(self.rx, SPF * self.maxr + 63)), 1)
        self.dg, self.in_flight = dg, 0
        self.pinned = self.dev = self.frames_dev = self.frames_host = None

    def check(self, rc):
        if rc:
            raise RuntimeError("sdrhip error %d: %s" % (rc, self.lib.sdrhip_last_error().decode("utf-8", "replace")))

    def sync(self):
        self.check(self.lib.sdrhip_ctx_synchronize(self.ctx))

    def call_sync(self):
        import torch

        if self.dev is None:
            self.dev = torch.from_numpy(self.dg).cuda()
            self.frames_dev = torch.empty((S, self.cap, 128 + R_OUT, 512), dtype=torch.uint8, device="cuda")
        self.check(self.lib.sdrhip_rx_process_datagrams(self.rx, P(self.dev.data_ptr()), self.nd, self.stride, self.sec, self.usec, self.maxr,
                                                        P(self.frames_dev.data_ptr()), self.cap * self.fb, self.info, self.nr, self.nf, 1))

    def collect(self):
        self.check(self.lib.sdrhip_rx_collect_datagrams(self.rx, self.frames_host.ctypes.data, self.cap * self.fb, self.cap, self.maxr, self.info,
                                                        self.nr, self.nf, 1))
        self.in_flight -= 1

    def call_async(self):
        if self.pinned is None:
            self.check(self.lib.sdrhip_rx_set_async(self.rx, self.depth, 1))
            self.pinned = self.lib.sdrhip_host_alloc(self.ctx, self.dg.nbytes)
            if not self.pinned:
                raise RuntimeError("sdrhip_host_alloc failed")
            C.memmove(self.pinned, self.dg.ctypes.data, self.dg.nbytes)
            self.frames_host = np.empty((S, self.cap, 128 + R_OUT, 512), np.uint8)
        if self.in_flight == self.depth:
            self.collect()
        self.check(self.lib.sdrhip_rx_submit_datagrams(self.rx, P(self.pinned), self.nd, 0, self.sec, self.usec))  # (0 = SDRHIP_PACKED)
        self.in_flight += 1

    def drain(self):
        while self.in_flight:
            self.collect()
        self.sync()

    def close(self):
        self.drain()
        self.dev = self.frames_dev = None
        if self.pinned:
            self.lib.sdrhip_host_free(self.ctx, P(self.pinned))
        self.lib.sdrhip_rx_destroy(self.rx)
        self.lib.sdrhip_ctx_destroy(self.ctx)


def open_parent(path, product):
    """the parent commit's library beside the product (a file of its own: its own code, kernels and state), the product's prototypes"""
    lib = C.CDLL(os.path.abspath(path))
    for n in ENTRIES:
        getattr(lib, n).argtypes = getattr(product, n).argtypes
        getattr(lib, n).restype = getattr(product, n).restype
    return lib


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
        raise SystemExit("bench_rx_follow_meta: no GPU")
    product = sd._lib.lib()
    dg, counts = batch(Oracle(), np.random.RandomState(1))
    spec = dict(sync_off=(product, False, "sync"), sync_on=(product, True, "sync"), async_off=(product, False, "async"),
                async_on=(product, True, "async"))
    if args.parent_lib:
        parent = open_parent(args.parent_lib, product)
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
        res = dict(bench="rx_follow_meta", only=args.only, calls=args.calls, frames_out_per_call=frames_out)
    else:
        ms = {k: [] for k in callers}
        for _ in range(args.rounds):
            for k in callers:  # (alternating)
                ms[k].append(round(window(k), 4))
        med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
        res = dict(bench="rx_follow_meta",
                   workload="rx datagrams: 8 streams x 64 released frames per call, fecblk 32 in, 24 erasures per frame, meta blocks in, "
                            "decimate16_cen, nb_fec 32 out; sync: device memory, async: packed pinned host memory, depth %d" % args.depth,
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
