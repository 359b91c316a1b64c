"""Asynchronous datagram-fed Tx batches (sdrhip_tx_submit_datagrams / sdrhip_tx_collect_datagrams) against back-to-back
synchronous host-memory calls (sdrhip_tx_process_datagrams), on the shape of tools/bench_tx_datagrams.py: 64 streams x 16 frames x
160 datagrams per batch (fecblk 32, 24 random losses per frame: 136 datagrams per frame).  Variants:
  a  x1, int16 output
  b  x16, 8-bit output (the HackRF sink)
  c  ragged counts: 8..16 frames per stream, x1, int16
each as  sync (pageable strided input, one call per batch), async_pinned (depth 4, packed sdrhip_host_alloc input uploaded in
place) and async_pageable (depth 4, the same strided pageable input as the synchronous call, staged).  Host clock around a run of
--batches batches (async: the ring kept full, every batch collected into the caller's rows), median over --rounds rounds, the
variants alternating.  Also: the link rate a batch achieves against a plain pinned copy of the same size in each direction, the
delivery gather's rate (kernel timers) against 8 TB/s, and the host time of a submit with in-place input (the shadow's run over
the headers, the tables and the launches).  Prints one JSON line.

    python tools/bench_tx_datagrams_async.py [--rounds N] [--batches B] [--out FILE]
Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own."""
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

S, F, R, LOST = 64, 16, 32, 24
SPF = 16129
HBM = 8.0e12


def batch(orc, rs, counts):
    """per stream counts[s] frames (frame indices 0 .. counts[s] - 1) with LOST random losses each, arrival order"""
    per = []
    for s in range(S):
        row = []
        for f in range(counts[s]):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            allb = np.concatenate([fr, orc.frame_encode(fr, R)])
            keep = sorted(set(range(128 + R)) - set(rs.choice(128 + R, LOST, replace=False).tolist()))
            row += [allb[i] for i in keep]
        per.append(np.asarray(row, np.uint8))
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_tx_datagrams_async: no GPU")
    orc = Oracle()
    rs = np.random.RandomState(1)
    ctx = sd.Context(0)
    lib = ctx.lib
    P = C.c_void_p
    eq = batch(orc, rs, [F] * S)
    rcounts = [int(x) for x in rs.randint(8, F + 1, S)]
    rg = batch(orc, rs, rcounts)
    shapes = dict(a=(eq, 0, "s16"), b=(eq, 4, "s8"), c=(rg, 0, "s16"))
    maxf = F + 1
    res = dict(workload="tx datagram batches: 64 streams x 16 frames x 136 datagrams (fecblk 32, 24 losses), host memory",
               ragged_counts_mean=float(np.mean(rcounts)), batches_per_run=args.batches, rounds=args.rounds)
    runs = {}
    for key, (per, L, fmt) in shapes.items():
        nd = [p.shape[0] for p in per]
        ndc = (C.c_size_t * S)(*nd)
        nmax = max(nd)
        strided = np.zeros((S, nmax, 512), np.uint8)
        for s, p in enumerate(per):
            strided[s, :p.shape[0]] = p
        pinned = ctx.host_alloc((sum(nd), 512), np.uint8)
        pinned[:] = np.concatenate(per)
        esz = 2 if fmt == "s8" else 4
        ostride = ((maxf * SPF) << L) + 7 & ~7
        out = np.empty((S, ostride * esz), np.uint8)
        b0 = np.empty((S, maxf, 508), np.uint8)
        info = (sd.engine.FECBufferFrame * (S * maxf))()
        nf = (C.c_size_t * S)()
        txs = {}
        for v in ("sync", "async_pinned", "async_pageable"):
            tx = sd.TxPipe(ctx, S, L, output_format=fmt)
            tx.set_async(4)
            txs[v] = tx

        def run_sync(n, tx=txs["sync"]):
            for _ in range(n):
                check(lib.sdrhip_tx_process_datagrams(tx.h, P(strided.ctypes.data), ndc, nmax * 512, P(out.ctypes.data), ostride, maxf,
                                                      P(b0.ctypes.data), info, nf, sd.MEM_HOST))

        def run_async(n, tx, src, stride):
            sub = col = 0
            while col < n:
                if sub < n:
                    rc = lib.sdrhip_tx_submit_datagrams(tx.h, P(src), ndc, stride)
                    if rc == 0:
                        sub += 1
                        continue
                    if rc != -6:
                        check(rc)
                check(lib.sdrhip_tx_collect_datagrams(tx.h, P(out.ctypes.data), ostride, maxf, P(b0.ctypes.data), info, nf, 1))
                col += 1

        fns = dict(sync=run_sync,
                   async_pinned=lambda n: run_async(n, txs["async_pinned"], pinned.ctypes.data, 0),
                   async_pageable=lambda n: run_async(n, txs["async_pageable"], strided.ctypes.data, nmax * 512))
        for fn in fns.values():  # steady state: every later batch releases the batch's frames
            fn(2)
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn(args.batches)
                times[k].append((time.perf_counter() - t0) / args.batches)
        assert [int(x) for x in nf] == ([F] * S if key != "c" else rcounts), [int(x) for x in nf]
        frames = sum(int(x) for x in nf)
        up = sum(nd) * 512
        down = frames * ((SPF << L) * esz + 16 + 508)
        # the gather on its own (kernel timers, class K_CONVERT: nothing else of these batches runs in it)
        ctx.synchronize()
        ctx.kernel_timing(True)
        ctx.kernel_timing_read(sd.engine.K_CONVERT)
        fns["async_pinned"](args.batches)
        gms, gn = ctx.kernel_timing_read(sd.engine.K_CONVERT)
        ctx.kernel_timing(False)
        g_s = gms / max(gn, 1) * 1e-3
        # the host side of a submit with in-place input: shadow + tables + launches (no staging copy)
        txp = txs["async_pinned"]
        ts = []
        for _ in range(args.batches):
            t0 = time.perf_counter()
            check(lib.sdrhip_tx_submit_datagrams(txp.h, P(pinned.ctypes.data), ndc, 0))
            ts.append(time.perf_counter() - t0)
            check(lib.sdrhip_tx_collect_datagrams(txp.h, P(out.ctypes.data), ostride, maxf, P(b0.ctypes.data), info, nf, 1))
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
        del hu, hd, du, dd
        med = {k: float(np.median(v)) for k, v in times.items()}
        dgs = sum(nd)
        link_s = float(np.median(cu)) + float(np.median(cd))
        runs[key] = dict(log2interp=L, output=fmt, datagrams=dgs, frames=frames, up_bytes=up, down_bytes=down,
                         batch_ms_median={k: v * 1e3 for k, v in med.items()},
                         datagrams_per_s={k: dgs / v for k, v in med.items()},
                         async_pinned_over_sync=med["sync"] / med["async_pinned"],
                         async_pageable_over_sync=med["sync"] / med["async_pageable"],
                         link_GBps_async_pinned=(up + down) / med["async_pinned"] / 1e9,
                         plain_pinned_copy_ms=dict(h2d=float(np.median(cu)) * 1e3, d2h=float(np.median(cd)) * 1e3),
                         plain_pinned_copy_GBps=dict(h2d=up / float(np.median(cu)) / 1e9, d2h=down / float(np.median(cd)) / 1e9),
                         async_pinned_over_plain_copies=link_s / med["async_pinned"],
                         gather_us=g_s * 1e6, gather_TBps=2 * down / g_s / 1e12 if g_s else 0.0,
                         gather_of_hbm=2 * down / g_s / HBM if g_s else 0.0,
                         submit_inplace_host_ms_median=float(np.median(ts)) * 1e3)
        ctx.host_free(pinned)
        for tx in txs.values():
            tx.close()
    res["variants"] = runs
    ra = runs["a"]["async_pinned_over_sync"]
    res["aim_a_async_pinned_over_sync"] = dict(value=ra, aim=">= 1.5", met=bool(ra >= 1.5))
    ga = max(r["gather_of_hbm"] for r in runs.values())
    res["aim_gather_of_hbm"] = dict(value=ga, per_variant={k: r["gather_of_hbm"] for k, r in runs.items()}, aim=">= 0.5", met=bool(ga >= 0.5))
    res["shadow_mismatch"] = ctx.counter("fecbuf_shadow_mismatch")
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
