"""Asynchronous ragged Rx entry (sdrhip_rx_submit_ragged / sdrhip_rx_collect_ragged), host clock, medians of --iters runs:
  g  64 streams x counts in [1, 4] x 65 536 per block, int16, ring depth 4, 8 blocks per batch: samples/s of the whole
     submit / collect stream (pinned packed blocks used in place; pageable strided rows) against the synchronous ragged host call
     (one sdrhip_rx_process_ragged per block, DESIGN.md's line e)
  h  16 x 65 536 per block, equal counts, 16 blocks per batch, pinned: ragged against sdrhip_rx_submit / collect
  i  K0p alone on one large batch (kernel-class timer of the widening / unpacking pass), against 8 TB/s of HBM
decimate16_cen, fecblk 32.  Link bytes per batch come from the context counters.  Kernel and copy counts come from a rocprofv3 run
of their own (--quick: fewer iterations).  Prints one JSON line (--out: also to a file).

    python tools/bench_rx_ragged_async.py [--iters N] [--out FILE] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.iters, args.batches = 2, 2
    import sdrdaemon_amd as sd

    ctx = sd.Context(0)
    rs = np.random.RandomState(1)
    L, R, B = 4, 32, 65536
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    fb = (128 + R) * 512

    # ---- g
    HS, blocks, depth = 64, 8, 4
    nblk = blocks * args.batches
    counts = [[int(v) * B for v in rs.randint(1, 5, size=HS)] for _ in range(blocks)]  # (batch after batch: the same 8 blocks)
    hx = rs.randint(-32768, 32768, size=(HS, 4 * B, 2)).astype(np.int16)  # strided rows (stride 4 x 65 536)
    packed = []
    for c in counts:
        p = ctx.host_alloc((sum(c) * 2,), np.int16)
        o = 0
        for s in range(HS):
            p[2 * o:2 * (o + c[s])] = hx[s, :c[s]].reshape(-1)
            o += c[s]
        packed.append(p)
    samples = args.batches * sum(sum(c) for c in counts)

    def run_async(form, rx):
        t0 = time.perf_counter()
        for b in range(nblk):
            while True:
                try:
                    rx.submit_ragged(packed[b % blocks] if form == "pinned" else hx, counts[b % blocks], b, 0)
                    break
                except sd.SdrHipError as e:
                    assert e.code == -6
                    rx.collect_ragged()
        while rx.collect_ragged() is not None:
            pass
        return time.perf_counter() - t0

    def run_sync(rx):
        t0 = time.perf_counter()
        for b in range(nblk):
            rx.process_ragged(hx, counts[b % blocks], b, 0)
        return time.perf_counter() - t0

    pipes = {k: sd.RxPipe(ctx, HS, **cfg) for k in ("pinned", "strided", "sync")}
    for k in ("pinned", "strided"):
        pipes[k].set_async(depth=depth, blocks=blocks)
    tg = {k: [] for k in pipes}
    link = {}
    for it in range(args.iters + 1):
        for k, rx in pipes.items():
            h0, d0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
            t = run_sync(rx) if k == "sync" else run_async(k, rx)
            if it:
                tg[k].append(t)
            link[k] = {"h2d_per_batch": (ctx.counter("h2d_bytes") - h0) / args.batches, "d2h_per_batch": (ctx.counter("d2h_bytes") - d0) / args.batches}
    gs = {k: samples / float(np.median(v)) for k, v in tg.items()}
    packed_bytes = samples * 4 / args.batches
    for p in packed:
        ctx.host_free(p)

    # ---- h
    S2, bl2 = 16, 16
    nb2 = bl2 * args.batches
    ux = [ctx.host_alloc((S2, B, 2), np.int16) for _ in range(bl2)]  # (the same 16 blocks batch after batch)
    for a in ux:
        a[:] = rs.randint(-32768, 32768, size=a.shape)
    uni, rg = sd.RxPipe(ctx, S2, **cfg), sd.RxPipe(ctx, S2, **cfg)
    uni.set_async(depth=4, blocks=bl2)
    rg.set_async(depth=4, blocks=bl2)
    flat = [a.reshape(-1) for a in ux]  # (the same pinned memory, packed: equal counts make rows back to back)

    def h_uni():
        t0 = time.perf_counter()
        for b in range(nb2):
            while True:
                try:
                    uni.submit(ux[b % bl2], b, 0)
                    break
                except sd.SdrHipError:
                    uni.collect()
        while uni.collect() is not None:
            pass
        return time.perf_counter() - t0

    def h_rg():
        t0 = time.perf_counter()
        for b in range(nb2):
            while True:
                try:
                    rg.submit_ragged(flat[b % bl2], [B] * S2, b, 0)
                    break
                except sd.SdrHipError:
                    rg.collect_ragged()
        while rg.collect_ragged() is not None:
            pass
        return time.perf_counter() - t0

    th = {"uniform": [], "ragged": []}
    for it in range(args.iters + 1):
        tu, tr = h_uni(), h_rg()
        if it:
            th["uniform"].append(tu)
            th["ragged"].append(tr)
    hm = {k: float(np.median(v)) * 1e3 / args.batches for k, v in th.items()}
    for a in ux:
        ctx.host_free(a)

    # ---- i: K0p alone (kernel-class timer) on one batch of 64 x 8 blocks of up to 4 x 65 536
    big = sd.RxPipe(ctx, HS, **cfg)
    big.set_async(depth=2, blocks=blocks)
    ctx.kernel_timing(True)
    kms = []
    for it in range(args.iters + 1):
        ctx.kernel_timing_read(sd.engine.K_CONVERT)
        for b in range(blocks):
            big.submit_ragged(hx, counts[b], b, 0)
        big.collect_ragged()
        ms, n = ctx.kernel_timing_read(sd.engine.K_CONVERT)
        assert n == 1, n
        if it:
            kms.append(ms)
    ctx.kernel_timing(False)
    isamp = sum(sum(c) for c in counts)
    k0p_ms = float(np.median(kms))
    k0p_tbs = 2 * isamp * 4 / (k0p_ms * 1e-3) / 1e12

    res = {"metric": "asynchronous ragged Rx, host clock, medians", "iters": args.iters, "batches": args.batches,
           "g": {"shape": "64 streams x [1, 4] x 65536 per block, S16, depth 4, 8 blocks per batch, decimate16_cen, fecblk 32",
                 "msamples_per_s": {k: round(v / 1e6, 1) for k, v in gs.items()},
                 "pinned_over_sync": round(gs["pinned"] / gs["sync"], 3), "strided_over_sync": round(gs["strided"] / gs["sync"], 3),
                 "link": link, "packed_bytes_per_batch": packed_bytes},
           "h": {"shape": "16 x 65536 per block, 16 blocks per batch, pinned, equal counts", "ms_per_batch": {k: round(v, 4) for k, v in hm.items()},
                 "ragged_over_uniform": round(hm["ragged"] / hm["uniform"], 3)},
           "i": {"samples": isamp, "k0p_ms": round(k0p_ms, 4), "bytes": 2 * isamp * 4, "tb_per_s": round(k0p_tbs, 3),
                 "of_8_tb_per_s": round(k0p_tbs / 8.0, 3)},
           "frame_bytes": fb}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
