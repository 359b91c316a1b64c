"""8-bit IQ at the edges of the pipes against int16, each pair alternating in one process, host clock around the work + a
synchronise, medians of --iters (default 50) for every line:
  rx_sync_{s16,u8}            host-fed Rx, 16 streams x 65 536-sample blocks, decimate16_cen, fecblk 32: one sdrhip_rx_process per block
  rx_async_{pinned,pageable}_{s16,u8}   the same blocks through sdrhip_rx_submit / _collect, depth 4, 16 blocks per batch: each
                              configuration on its own, windows of 4 batches drained inside the clock (time per batch)
  rx_dev_{s16,u8}             the whole Rx step on device input, 8 streams x 2^25 samples (the 8-bit one includes the widening pass K0)
  tx_dev_{s16,s8}             Tx on the configs[3] shape: 8 streams x 128 frames, 24 random erasures per frame, x16, device output
  tx_host_{s16,s8}            the same with host input and output
Kernel times per call come from the context's kernel-class timers (K_CONVERT, K_INTERPOLATE); a rocprofv3 --kernel-trace --stats run
of its own gives the per-kernel table.  Prints one JSON line (--out: also to a file).

    python tools/bench_iq8.py [--iters N] [--warmup W] [--out FILE] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (bench.py)
PCIE_PEAK_GBS = 63.0   # host link, PCIe Gen5 x16 per direction (bench.py)
SPF = 16129


def median_ms(xs):
    return float(np.median(xs)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="smaller shapes (a profiler run)")
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle

    if sd.device_count() <= 0:
        raise SystemExit("bench_iq8: no GPU")
    ctx = sd.Context(0)
    rs = np.random.RandomState(1)
    res = {}

    def alternate(pairs, iters, kclasses=()):
        """pairs: name -> fn; -> (median ms per call, kernel ms per call by class)"""
        for fn in pairs.values():
            for _ in range(args.warmup):
                fn()
        ctx.synchronize()
        ctx.kernel_timing(True)
        t = {k: [] for k in pairs}
        kt = {k: {c: 0.0 for c in kclasses} for k in pairs}
        for _ in range(iters):
            for k, fn in pairs.items():
                for c in kclasses:
                    ctx.kernel_timing_read(c)
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                t[k].append(time.perf_counter() - t0)
                for c in kclasses:
                    kt[k][c] += ctx.kernel_timing_read(c)[0]
        ctx.kernel_timing(False)
        return {k: median_ms(v) for k, v in t.items()}, {k: {c: v / iters for c, v in d.items()} for k, d in kt.items()}

    # ---- Rx host-fed: 16 streams x 65 536-sample blocks, decimate16_cen, fecblk 32
    S, n, NB = 16, 65536, 16
    blocks8 = rs.randint(0, 256, (NB, S, n, 2)).astype(np.uint8)
    blocks16 = (blocks8.astype(np.int16) - 128).astype(np.int16)
    cfg = dict(log2decim=4, fcpos=sd.FC_CEN, sample_bits=8, nb_fec=32)
    pipes = {f: sd.RxPipe(ctx, S, input_format=f, **cfg) for f in ("s16", "u8")}
    it = {"i": 0}

    def sync_call(f, data):
        def call():
            pipes[f].process(data[it["i"] % NB])
            it["i"] += 1
        return call
    med, _ = alternate({"s16": sync_call("s16", blocks16), "u8": sync_call("u8", blocks8)}, args.iters)
    for f in ("s16", "u8"):
        sps = S * n / (med[f] * 1e-3)
        res["rx_sync_" + f] = dict(ms_per_block=med[f], msamples_per_s=sps / 1e6, link_fraction=sps * (4 if f == "s16" else 2) / (PCIE_PEAK_GBS * 1e9))
    res["rx_sync_u8_over_s16_samples_per_s"] = med["s16"] / med["u8"]

    # async, depth 4, 16 blocks per batch.  Each configuration runs on its own (a pipe of its own, nothing else on the context's
    # stream): a timed window submits WIN batches, collecting the oldest whenever 3 are in flight, and drains the ring before the
    # clock stops -- every copy, launch and download of the window's batches lies inside it.  Time per batch = window / WIN.
    WIN = 4
    pinned = {"s16": ctx.host_alloc((NB, S, n, 2), np.int16), "u8": ctx.host_alloc((NB, S, n, 2), np.uint8)}
    pinned["s16"][:] = blocks16
    pinned["u8"][:] = blocks8
    for mode in ("pinned", "pageable"):
        for f in ("s16", "u8"):
            src = pinned[f] if mode == "pinned" else (blocks16 if f == "s16" else blocks8)
            p = sd.RxPipe(ctx, S, input_format=f, **cfg)
            p.set_async(depth=4, blocks=NB)

            def window():
                inflight = 0
                for _ in range(WIN):
                    for b in range(NB):
                        p.submit(src[b], tv_sec=0, tv_usec=0)
                    inflight += 1
                    if inflight >= 3:
                        p.collect(wait=True)
                        inflight -= 1
                while inflight:
                    p.collect(wait=True)
                    inflight -= 1
            for _ in range(max(args.warmup // 2, 1)):
                window()
            t = []
            for _ in range(args.iters):
                t0 = time.perf_counter()
                window()
                ctx.synchronize()
                t.append(time.perf_counter() - t0)
            p.close()
            ms = median_ms(t) / WIN
            sps = NB * S * n / (ms * 1e-3)
            res["rx_async_%s_%s" % (mode, f)] = dict(ms_per_batch=ms, msamples_per_s=sps / 1e6, windows=args.iters, batches_per_window=WIN,
                                                     link_fraction=sps * (4 if f == "s16" else 2) / (PCIE_PEAK_GBS * 1e9))
    r = res["rx_async_pinned_u8"]["msamples_per_s"] / res["rx_async_pinned_s16"]["msamples_per_s"]
    res["aim_rx_async_pinned_u8_over_s16"] = dict(value=r, aim=">= 1.4", met=bool(r >= 1.4))
    res["rx_async_pageable_u8_over_s16"] = res["rx_async_pageable_u8"]["msamples_per_s"] / res["rx_async_pageable_s16"]["msamples_per_s"]
    for p in pipes.values():
        p.close()
    ctx.host_free(pinned["s16"])
    ctx.host_free(pinned["u8"])
    del blocks8, blocks16

    # ---- device input: 8 streams x 2^25 samples, the headline Rx step, with and without the widening pass
    S2, n2 = 8, (1 << 21) if args.quick else (1 << 25)
    x8 = torch.randint(0, 256, (S2, n2, 2), dtype=torch.uint8, device="cuda")
    x16 = (x8.to(torch.int16) - 128).contiguous()
    dp = {f: sd.RxPipe(ctx, S2, input_format=f, **cfg) for f in ("s16", "u8")}
    med, kt = alternate({"s16": lambda: dp["s16"].process_view(x16), "u8": lambda: dp["u8"].process_view(x8)}, args.iters,
                        (sd.engine.K_CONVERT, sd.engine.K_DECIMATE, sd.engine.K_FEC_ENCODE))
    conv_ms = kt["u8"][sd.engine.K_CONVERT]
    frac = 6.0 * S2 * n2 / (conv_ms * 1e-3) / (HBM_PEAK_GBS * 1e9)
    res["convert_kernel"] = dict(ms=conv_ms, samples=S2 * n2, hbm_fraction_6B_per_sample=frac)
    res["aim_convert_hbm_fraction"] = dict(value=frac, aim=">= 0.55", met=bool(frac >= 0.55))
    res["rx_dev_step_ms"] = med
    res["rx_dev_kernel_ms"] = {k: {str(c): v for c, v in d.items()} for k, d in kt.items()}
    res["rx_dev_u8_step_over_s16"] = med["u8"] / med["s16"]
    del x8, x16, dp

    # ---- Tx, configs[3] shape: 8 streams x 128 frames, 24 random erasures per frame, x16
    orc = Oracle()
    S3, F3, R3 = 8, (16 if args.quick else 128), 32
    one = []
    for f in range(8):  # (8 distinct encoded frames, reused with their own losses)
        fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
        fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
        one.append(np.concatenate([fr, orc.frame_encode(fr, R3)]))
    rx = np.zeros((S3, F3, 128, 512), np.uint8)
    for s in range(S3):
        for f in range(F3):
            lost = set(rs.choice(np.arange(1, 128), 24, replace=False).tolist())
            rx[s, f] = one[(s + f) % 8][[i for i in range(128 + R3) if i not in lost][:128]]
    drx = torch.from_numpy(rx).cuda()
    tp = {f: sd.TxPipe(ctx, S3, 4, output_format=f) for f in ("s16", "s8")}
    med, kt = alternate({"s16": lambda: tp["s16"].process(drx), "s8": lambda: tp["s8"].process(drx)}, args.iters, (sd.engine.K_INTERPOLATE,))
    kr = kt["s8"][sd.engine.K_INTERPOLATE] / kt["s16"][sd.engine.K_INTERPOLATE]
    sr = med["s8"] / med["s16"]
    res["tx_dev_step_ms"] = med
    res["tx_dev_k5w_ms"] = {k: d[sd.engine.K_INTERPOLATE] for k, d in kt.items()}
    res["aim_tx_k5w_s8_over_s16"] = dict(value=kr, aim="<= 0.85", met=bool(kr <= 0.85))
    res["aim_tx_step_s8_over_s16"] = dict(value=sr, aim="<= 0.92", met=bool(sr <= 0.92))
    th = {f: sd.TxPipe(ctx, S3, 4, output_format=f) for f in ("s16", "s8")}
    med, _ = alternate({"s16": lambda: th["s16"].process(rx), "s8": lambda: th["s8"].process(rx)}, args.iters)
    res["tx_host_call_ms"] = med
    res["tx_host_s8_over_s16"] = med["s8"] / med["s16"]
    res["shapes"] = dict(rx_host="16 x 65536 per block, decimate16_cen, fecblk 32", rx_dev="%d x %d" % (S2, n2), tx="%d x %d frames, x16" % (S3, F3))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
