#!/usr/bin/env python3
"""The Tx bank with an output format per stream (sdrhip_tx_set_stream_format: K5x / K6x) against the bank-wide formats, on the shape of
bench.py's configs[3] and tools/bench_tx_datagrams.py: S streams x F received frames per call (fecblk 32, 24 blocks of every frame
lost), decode + interpolate by 16, sdrhip_tx_process from device memory (`dev`) and to host memory (`host`).

Lines, each a handle of its own, in alternating rounds in one process:
  parent_s16 / parent_s8   (--parent-lib FILE) a library built from the parent commit, loaded beside the product: bank-wide S16 / S8
  never_s16 / never_s8     the product, the setter never called: the parent's kernels, to be found inside the parent's own spread
  equal_s16 / equal_s8     the product, an array of equal entries: K5x on one branch
  mixed                    the product, formats alternating s16, s8, s16, ...
What the results are held against: `never` against the parent's round-to-round spread; `equal` and `mixed` against the stream-weighted
mean of the parent's (without --parent-lib: the never-set) S16 and S8 lines -- a K5x launch adds one scalar load and one branch per
wave; the host lines against the byte ratio of their downloads ("d2h_bytes").
A round is a window of at least --window seconds of back-to-back calls, the clock stops behind a device synchronisation; its figure
is ms per call.  Prints one JSON line: median and min..max per line, the rounds, the ratios.

    python tools/bench_tx_stream_format.py [--rounds N] [--window SECONDS] [--streams S] [--frames F] [--parent-lib FILE] [--out FILE]
    python tools/bench_tx_stream_format.py --only mixed --mem dev --calls 20      one line alone, a fixed number of calls behind the
        warm-up: for `rocprofv3 --kernel-trace --stats -- python tools/...` (counters in a run of their own)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R, LOST, L2 = 32, 24, 4
SPF = 16129
P = C.c_void_p
S16, S8 = 0, 2
# the entries a line uses: the parent library gets the product's prototypes for them
ENTRIES = ["sdrhip_last_error", "sdrhip_ctx_create", "sdrhip_ctx_destroy", "sdrhip_ctx_synchronize", "sdrhip_ctx_get_counter", "sdrhip_tx_create",
           "sdrhip_tx_destroy", "sdrhip_tx_process", "sdrhip_tx_set_output_format"]


def batch(orc, rs, S, F):
    """S streams x F frames of received super blocks: 128 of the 128 + R sent, LOST originals of every frame lost"""
    import signals

    rx = np.zeros((S, F, 128, 512), np.uint8)
    for s in range(S):
        frames = orc.framer(nb_fec_blocks=R).write(signals.mixed(F * SPF + 1, 7 + s))
        for f in range(F):
            full = np.concatenate([frames[f], orc.frame_encode(frames[f], R)])
            lost = set(rs.choice(np.arange(1, 128), LOST, replace=False).tolist())
            rx[s, f] = full[[i for i in range(128 + R) if i not in lost][:128]]
    return rx


class Handle:
    """one library (the product's, or the parent's beside it), one context, one Tx bank, through the C entries alone.
    bank: the bank-wide format; fmts: the array (None: the setter is never called)"""

    def __init__(self, lib, rx, bank, fmts, mem):
        import torch

        self.lib, self.mem = lib, mem
        self.S, self.F = rx.shape[0], rx.shape[1]
        self.ctx, self.tx = P(), P()
        self.check(lib.sdrhip_ctx_create(0, P(0), C.byref(self.ctx)))
        self.check(lib.sdrhip_tx_create(self.ctx, self.S, L2, C.byref(self.tx)))
        if bank != S16:
            self.check(lib.sdrhip_tx_set_output_format(self.tx, bank))
        if fmts is not None:
            self.check(lib.sdrhip_tx_set_stream_format(self.tx, (C.c_int * self.S)(*fmts)))
        n = (self.F * SPF) << L2
        # rows of 4 * stride bytes serve every line: bank-wide S16 counts them as `stride` samples, bank-wide S8 as 2 * stride
        self.stride = (n + 3) & ~3
        self.out_stride = 2 * self.stride if (fmts is None and bank == S8) else self.stride
        if mem == "dev":
            self.rx = torch.from_numpy(rx).cuda()
            self.out = torch.empty((self.S, 4 * self.stride), dtype=torch.uint8, device="cuda")
            self.rxp, self.outp = P(self.rx.data_ptr()), P(self.out.data_ptr())
        else:
            self.rx = np.ascontiguousarray(rx)
            self.out = np.empty((self.S, 4 * self.stride), np.uint8)
            self.rxp, self.outp = P(self.rx.ctypes.data), P(self.out.ctypes.data)
        self.n_out = C.c_size_t(0)

    def check(self, rc):
        if rc:
            raise RuntimeError("sdrhip error %d: %s" % (rc, self.lib.sdrhip_last_error().decode("utf-8", "replace")))

    def sync(self):
        self.check(self.lib.sdrhip_ctx_synchronize(self.ctx))

    def call(self):
        self.check(self.lib.sdrhip_tx_process(self.tx, self.rxp, None, self.F, self.F * 128 * 512, self.outp, self.out_stride, C.byref(self.n_out),
                                              1 if self.mem == "dev" else 0))

    def d2h(self):
        v = C.c_uint64(0)
        self.check(self.lib.sdrhip_ctx_get_counter(self.ctx, b"d2h_bytes", C.byref(v)))
        return v.value

    def close(self):
        self.sync()
        self.rx = self.out = None
        self.lib.sdrhip_tx_destroy(self.tx)
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
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--parent-lib", default=None, help="libsdrhip.so built from the parent commit")
    ap.add_argument("--only", default=None, help="one line alone (kernel-trace runs)")
    ap.add_argument("--mem", default=None, choices=["dev", "host"], help="one memory kind alone")
    ap.add_argument("--calls", type=int, default=20, help="calls of the --only line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first: both libraries bind to it)

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle

    if sd.device_count() <= 0:
        raise SystemExit("bench_tx_stream_format: no GPU")
    product = sd._lib.lib()
    S, F = args.streams, args.frames
    rx = batch(Oracle(), np.random.RandomState(1), S, F)
    alt = [S8 if s % 2 else S16 for s in range(S)]
    spec = dict(never_s16=(product, S16, None), never_s8=(product, S8, None), equal_s16=(product, S16, [S16] * S),
                equal_s8=(product, S16, [S8] * S), mixed=(product, S16, alt))
    if args.parent_lib:
        parent = open_parent(args.parent_lib, product)
        spec.update(parent_s16=(parent, S16, None), parent_s8=(parent, S8, None))
    if args.only:
        spec = {args.only: spec[args.only]}
    handles = {}
    for mem in ([args.mem] if args.mem else ["dev", "host"]):
        for name, (lib, bank, fmts) in spec.items():
            handles[name + "_" + mem] = Handle(lib, rx, bank, fmts, mem)
    d2h = {}
    for name, h in handles.items():
        for _ in range(max(args.warmup, 2)):
            h.call()
        h.sync()
        b0 = h.d2h()
        h.call()
        h.sync()
        d2h[name] = h.d2h() - b0

    def window(h):
        h.sync()
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.window:
            h.call()
            n += 1
        h.sync()
        return (time.perf_counter() - t0) / n * 1e3

    if args.only:
        for h in handles.values():
            for _ in range(args.calls):
                h.call()
            h.sync()
        res = dict(bench="tx_stream_format", only=args.only, calls=args.calls, d2h_bytes_per_call=d2h)
    else:
        ms = {k: [] for k in handles}
        for _ in range(args.rounds):
            for k, h in handles.items():  # (alternating)
                ms[k].append(round(window(h), 4))
        med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
        n8 = sum(1 for f in alt if f == S8)
        ratios = {}
        for mem in ([args.mem] if args.mem else ["dev", "host"]):
            base = "parent" if args.parent_lib else "never"
            a, b = med["%s_s16_%s" % (base, mem)], med["%s_s8_%s" % (base, mem)]
            ratios[mem] = dict(yardstick=base, equal_s16_over_s16=round(med["equal_s16_" + mem] / a, 4), equal_s8_over_s8=round(med["equal_s8_" + mem] / b, 4),
                               mixed_over_weighted_mean=round(med["mixed_" + mem] / (((S - n8) * a + n8 * b) / S), 4))
            if args.parent_lib:
                for f in ("s16", "s8"):
                    p = ms["parent_%s_%s" % (f, mem)]
                    ratios[mem]["never_%s_minus_parent_us" % f] = round((med["never_%s_%s" % (f, mem)] - med["parent_%s_%s" % (f, mem)]) * 1e3, 2)
                    ratios[mem]["parent_%s_spread_us" % f] = round((max(p) - min(p)) * 1e3, 2)
        res = dict(bench="tx_stream_format",
                   workload="tx: %d streams x %d frames per call, decode 128+32 with %d lost + interpolate16_cen, sdrhip_tx_process; dev: device "
                            "memory, host: host memory" % (S, F, LOST),
                   ms_per_call_median=med, ms_per_call_min={k: float(np.min(v)) for k, v in ms.items()},
                   ms_per_call_max={k: float(np.max(v)) for k, v in ms.items()}, rounds=ms, ratios=ratios, d2h_bytes_per_call=d2h)
    for h in handles.values():
        h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
