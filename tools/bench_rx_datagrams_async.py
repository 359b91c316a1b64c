"""Asynchronous datagram-fed Rx batches (sdrhip_rx_submit_datagrams / sdrhip_rx_collect_datagrams) against back-to-back
synchronous host-memory calls (sdrhip_rx_process_datagrams), on the shape of tools/bench_tx_datagrams_async.py: 64 streams x 16
frames x 136 datagrams per batch (incoming fecblk 32, 24 random losses per frame), then decimate16_cen, nb_fec 32: every batch
releases 16 payloads and completes one frame per stream.  Variants:
  sync            back-to-back sdrhip_rx_process_datagrams calls, pageable strided input (the yardstick)
  sync_parent     the same calls through a library built from the parent commit (--parent-lib), in the same alternating rounds
  async_pinned    depth 4, packed sdrhip_host_alloc input uploaded in place
  async_pageable  depth 4, the same strided pageable input as the synchronous call, staged
Host clock around a run of --batches batches (async: the ring kept full, every batch collected into the caller's rows), median
over --rounds rounds, the variants alternating.  Also: the link rate a batch achieves against plain pinned copies of the same
sizes in each direction, the delivery kernel's time and rate (kernel timers), and the host time of a submit with in-place input
(the shadow's run over the headers, the tables and the launches), alone and behind batches that are still in flight.  Prints one JSON line.

    python tools/bench_rx_datagrams_async.py [--rounds N] [--batches B] [--parent-lib libsdrhip.so] [--out FILE]
Kernel times and launches per batch: `rocprofv3 --kernel-trace --stats -- python tools/bench_rx_datagrams_async.py --only
async_pinned`, a run of its own that holds that variant alone (3 + rounds x batches batches)."""
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

S, F, R_IN, LOST = 64, 16, 32, 24
L, R_OUT, DEPTH = 4, 32, 4
SPF = 16129
HBM = 8.0e12


def batch(orc, rs):
    """per stream F frames (frame indices 0 .. F - 1) of 128 + R_IN blocks with LOST random losses each, arrival order"""
    per = []
    for s in range(S):
        row = []
        for f in range(F):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            allb = np.concatenate([fr, orc.frame_encode(fr, R_IN)])
            keep = sorted(set(range(128 + R_IN)) - set(rs.choice(128 + R_IN, LOST, replace=False).tolist()))
            row += [allb[i] for i in keep]
        per.append(np.asarray(row, np.uint8))
    return per


class ParentRx:
    """sdrhip_rx_process_datagrams of another build of the library (the parent commit's), through its C ABI alone"""

    def __init__(self, path, cfg):
        P, sz, u32 = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        self.lib = lib = C.CDLL(path)
        lib.sdrhip_last_error.restype = C.c_char_p
        lib.sdrhip_ctx_create.argtypes = [C.c_int, P, C.POINTER(P)]
        lib.sdrhip_rx_create.argtypes = [P, C.c_int, P, C.POINTER(P)]
        lib.sdrhip_rx_process_datagrams.argtypes = [P, P, C.POINTER(sz), sz, u32, u32, sz, P, sz, P, C.POINTER(sz), C.POINTER(sz), C.c_int]
        self.ctx, self.h = P(), P()
        self.check(lib.sdrhip_ctx_create(0, P(0), C.byref(self.ctx)))
        self.check(lib.sdrhip_rx_create(self.ctx, S, C.cast(C.byref(cfg), P), C.byref(self.h)))

    def check(self, rc):
        if rc:
            raise RuntimeError("parent library: %d %s" % (rc, self.lib.sdrhip_last_error().decode()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, help="run this variant alone, for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_rx_datagrams_async: no GPU")
    orc = Oracle()
    rs = np.random.RandomState(1)
    ctx = sd.Context(0)
    lib = ctx.lib
    P = C.c_void_p
    per = batch(orc, rs)
    nd = [p.shape[0] for p in per]
    ndc = (C.c_size_t * S)(*nd)
    nmax = max(nd)
    strided = np.zeros((S, nmax, 512), np.uint8)
    for s, p in enumerate(per):
        strided[s, :p.shape[0]] = p
    pinned = ctx.host_alloc((sum(nd), 512), np.uint8)
    pinned[:] = np.concatenate(per)
    fbytes = (128 + R_OUT) * 512
    maxf, maxr = 3, F + 1
    out = np.empty((S, maxf * fbytes), np.uint8)
    info = (sd.engine.FECBufferFrame * (S * maxr))()
    nr, nf = (C.c_size_t * S)(), (C.c_size_t * S)()
    st = (C.c_uint32 * S)(*[7] * S)
    rxs = {v: sd.RxPipe(ctx, S, log2decim=L, nb_fec=R_OUT) for v in ("sync", "async_pinned", "async_pageable")}
    for v in ("async_pinned", "async_pageable"):
        rxs[v].set_async(depth=DEPTH)
    parent = ParentRx(args.parent_lib, rxs["sync"].cfg) if args.parent_lib else None

    def run_sync(n, lib=lib, h=rxs["sync"].h, chk=check):
        for _ in range(n):
            chk(lib.sdrhip_rx_process_datagrams(h, P(strided.ctypes.data), ndc, nmax * 512, st, st, maxr, P(out.ctypes.data), maxf * fbytes, info,
                                                nr, nf, sd.MEM_HOST))

    behind = []  # host time of every submit that went out while earlier batches were in flight

    def run_async(n, rx, src, stride):
        sub = col = 0
        while col < n:
            if sub < n:
                t0 = time.perf_counter()
                rc = lib.sdrhip_rx_submit_datagrams(rx.h, P(src), ndc, stride, st, st)
                if rc == 0:
                    if sub > col and stride == 0:
                        behind.append(time.perf_counter() - t0)
                    sub += 1
                    continue
                if rc != -6:
                    check(rc)
            check(lib.sdrhip_rx_collect_datagrams(rx.h, P(out.ctypes.data), maxf * fbytes, maxf, maxr, info, nr, nf, 1))
            col += 1

    fns = dict(sync=run_sync)
    if parent:
        fns["sync_parent"] = lambda n: run_sync(n, parent.lib, parent.h, parent.check)
    fns["async_pinned"] = lambda n: run_async(n, rxs["async_pinned"], pinned.ctypes.data, 0)
    fns["async_pageable"] = lambda n: run_async(n, rxs["async_pageable"], strided.ctypes.data, nmax * 512)
    if args.only:
        fns = {args.only: fns[args.only]}
    for fn in fns.values():  # steady state: every later batch releases the batch's frames and completes one frame per stream
        fn(3)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn(args.batches)
            times[k].append((time.perf_counter() - t0) / args.batches)
            assert [int(x) for x in nr] == [F] * S and [int(x) for x in nf] == [1] * S, (k, list(nr), list(nf))
    if args.only:
        med = float(np.median(times[args.only]))
        print(json.dumps(dict(variant=args.only, batches=3 + args.rounds * args.batches, batch_ms_median=med * 1e3,
                              submit_behind_batches_host_ms=dict(median=float(np.median(behind)) * 1e3, max=float(np.max(behind)) * 1e3)
                              if behind else None,
                              shadow_mismatch=ctx.counter("fecbuf_shadow_mismatch"))))
        return
    frames, recs = S, S * F
    up, down = sum(nd) * 512, frames * fbytes + recs * 16
    behind_run = list(behind)
    # the delivery kernel on its own (kernel timers, class K_CONVERT: nothing else of these batches runs in it)
    ctx.synchronize()
    ctx.kernel_timing(True)
    ctx.kernel_timing_read(sd.engine.K_CONVERT)
    fns["async_pinned"](args.batches)
    gms, gn = ctx.kernel_timing_read(sd.engine.K_CONVERT)
    ctx.kernel_timing(False)
    g_s = gms / max(gn, 1) * 1e-3
    # the host side of a submit with in-place input: shadow + tables + launches (no staging copy)
    rxp = rxs["async_pinned"]
    ts = []
    for _ in range(args.batches):
        t0 = time.perf_counter()
        check(lib.sdrhip_rx_submit_datagrams(rxp.h, P(pinned.ctypes.data), ndc, 0, st, st))
        ts.append(time.perf_counter() - t0)
        check(lib.sdrhip_rx_collect_datagrams(rxp.h, P(out.ctypes.data), maxf * fbytes, maxf, maxr, info, nr, nf, 1))
    # plain pinned copies of the same sizes
    hu = torch.empty(up, dtype=torch.uint8).pin_memory()
    hd = torch.empty(down, dtype=torch.uint8).pin_memory()
    du = torch.empty(up, dtype=torch.uint8, device="cuda")
    dd = torch.empty(down, dtype=torch.uint8, device="cuda")
    cu, cd = [], []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        du.copy_(hu, non_blocking=True)
        torch.cuda.synchronize()
        cu.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        hd.copy_(dd, non_blocking=True)
        torch.cuda.synchronize()
        cd.append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    dgs = sum(nd)
    link_s = float(np.median(cu)) + float(np.median(cd))
    res = dict(workload="rx datagram batches: 64 streams x 16 frames x 136 datagrams (fecblk 32, 24 losses) -> decimate16_cen, nb_fec 32, "
                        "host memory, depth %d" % DEPTH,
               batches_per_run=args.batches, rounds=args.rounds, datagrams=dgs, frames=frames, records=recs, up_bytes=up, down_bytes=down,
               batch_ms_median={k: v * 1e3 for k, v in med.items()},
               batch_ms_rounds={k: [x * 1e3 for x in v] for k, v in times.items()},
               datagrams_per_s={k: dgs / v for k, v in med.items()},
               async_pinned_over_sync=med["sync"] / med["async_pinned"],
               async_pageable_over_sync=med["sync"] / med["async_pageable"],
               link_GBps_async_pinned=(up + down) / med["async_pinned"] / 1e9,
               plain_pinned_copy_ms=dict(h2d=float(np.median(cu)) * 1e3, d2h=float(np.median(cd)) * 1e3),
               plain_pinned_copy_GBps=dict(h2d=up / float(np.median(cu)) / 1e9, d2h=down / float(np.median(cd)) / 1e9),
               async_pinned_over_plain_copies=link_s / med["async_pinned"],
               delivery_us=g_s * 1e6, delivery_launches_per_batch=gn / args.batches, delivery_GBps=2 * down / g_s / 1e9 if g_s else 0.0,
               delivery_of_hbm=2 * down / g_s / HBM if g_s else 0.0,
               submit_inplace_host_ms_median=float(np.median(ts)) * 1e3,
               # (a submit that waited for the batch before it would take about a batch's time)
               submit_behind_batches_host_ms=dict(median=float(np.median(behind_run)) * 1e3, max=float(np.max(behind_run)) * 1e3,
                                                  n=len(behind_run)))
    if parent:
        res["sync_parent_over_sync"] = med["sync_parent"] / med["sync"]
        res["async_pinned_over_sync_parent"] = med["sync_parent"] / med["async_pinned"]
        res["async_pageable_over_sync_parent"] = med["sync_parent"] / med["async_pageable"]
    res["shadow_mismatch"] = ctx.counter("fecbuf_shadow_mismatch")
    ctx.host_free(pinned)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
