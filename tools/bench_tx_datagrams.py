"""The Tx pipe fed datagrams (sdrhip_tx_process_datagrams, device memory, x16) on the shape of tools/bench_fecbuf.py: 64 streams x 16
frames x 160 datagrams (fecblk 32, 24 random losses per frame).  Host clock around call + synchronise, median of --iters, the
variants alternating in one process:
  a         the datagram call (one ragged interpolator launch on equal counts)
  b         sdrhip_fecbuf_write_and_read + ONE uniform sdrhip_interpolate of the same 1024 frames
  c         what a caller does without the entry when the counts differ: the bank + 64 one-stream sdrhip_interpolate calls
  a_ragged  the datagram call with 8..16 frames per stream (random, mean ~12)
The interpolator's own time per variant comes from the context's kernel timers (hipEvents around its launches).  Prints one JSON line.

    python tools/bench_tx_datagrams.py [--iters N] [--warmup W] [--out FILE]
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

S, F, R, LOST, L2 = 64, 16, 32, 24, 4
SPF = 16129


def batch(orc, rs, counts):
    """per stream counts[s] frames (frame indices 0 .. counts[s] - 1) with LOST random losses each, arrival order: [S][max][512]"""
    per = []
    for s in range(S):
        row = []
        for f in range(counts[s]):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            allb = np.concatenate([fr, orc.frame_encode(fr, R)])
            keep = sorted(set(range(128 + R)) - set(rs.choice(128 + R, LOST, replace=False).tolist()))
            row += [allb[i] for i in keep]
        per.append(np.asarray(row))
    n = max(p.shape[0] for p in per)
    dg = np.zeros((S, n, 512), np.uint8)
    for s, p in enumerate(per):
        dg[s, :p.shape[0]] = p
    return dg, [p.shape[0] for p in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_tx_datagrams: no GPU")
    orc = Oracle()
    rs = np.random.RandomState(1)
    dg, nd_eq = batch(orc, rs, [F] * S)
    rcounts = [int(x) for x in rs.randint(8, F + 1, S)]
    dgr, nd_rg = batch(orc, rs, rcounts)
    ctx = sd.Context(0)
    lib = ctx.lib
    maxf = F + 1
    pitch = (maxf * SPF + 3) & ~3                       # samples per stream of the bank's output (16-byte aligned streams)
    ostride = (((maxf * SPF) << L2) + 3) & ~3          # samples per stream of the interpolated output
    ddg, ddgr = torch.from_numpy(dg).cuda(), torch.from_numpy(dgr).cuda()
    out = torch.empty((S, ostride, 2), dtype=torch.int16, device="cuda")
    b0 = torch.empty((S, maxf, 508), dtype=torch.uint8, device="cuda")
    data = torch.empty((S, pitch, 2), dtype=torch.int16, device="cuda")
    info = (sd.engine.FECBufferFrame * (S * maxf))()
    nf = (C.c_size_t * S)()
    P = C.c_void_p

    def make_a(d, nd):
        tx = sd.TxPipe(ctx, S, L2)
        ndc = (C.c_size_t * S)(*nd)

        def call():
            check(lib.sdrhip_tx_process_datagrams(tx.h, P(d.data_ptr()), ndc, d.shape[1] * 512, P(out.data_ptr()), ostride, maxf,
                                                  P(b0.data_ptr()), info, nf, sd.MEM_DEVICE))
        return call, tx

    call_a, tx_a = make_a(ddg, nd_eq)
    call_ar, tx_ar = make_a(ddgr, nd_rg)
    bank_b, bank_c = sd.FECBufferBank(ctx, S), sd.FECBufferBank(ctx, S)
    itp_b = sd.Interpolators(ctx, S)
    itp_c = [sd.Interpolators(ctx, 1) for _ in range(S)]
    ndb = (C.c_size_t * S)(*nd_eq)
    ndr = (C.c_size_t * S)(*nd_rg)

    def bank(b, d, ndc):
        check(lib.sdrhip_fecbuf_write_and_read(b.h, P(d.data_ptr()), ndc, d.shape[1] * 512, P(data.data_ptr()), pitch * 4,
                                                  P(b0.data_ptr()), maxf, info, nf, sd.MEM_DEVICE))

    def call_b():
        bank(bank_b, ddg, ndb)
        n = max(nf) * SPF
        check(lib.sdrhip_interpolate(itp_b.h, L2, P(data.data_ptr()), n, pitch, P(out.data_ptr()), ostride, None, sd.MEM_DEVICE))

    def call_c():
        bank(bank_c, ddgr, ndr)
        for s in range(S):
            if nf[s]:
                check(lib.sdrhip_interpolate(itp_c[s].h, L2, P(data[s].data_ptr()), nf[s] * SPF, 0, P(out[s].data_ptr()), 0, None,
                                             sd.MEM_DEVICE))

    variants = dict(a=call_a, b=call_b, c=call_c, a_ragged=call_ar)
    for fn in variants.values():  # steady state: every later call releases the 16 (or counts[s]) frames of the batch
        for _ in range(max(args.warmup, 2)):
            fn()
    ctx.synchronize()
    ctx.kernel_timing(True)
    times = {k: [] for k in variants}
    ktime = {k: [0.0, 0] for k in variants}
    frames = {}
    for _ in range(args.iters):
        for k, fn in variants.items():  # (alternating)
            ctx.kernel_timing_read(sd.engine.K_INTERPOLATE)
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            times[k].append(time.perf_counter() - t0)
            ms, n = ctx.kernel_timing_read(sd.engine.K_INTERPOLATE)
            ktime[k][0] += ms
            ktime[k][1] += n
            frames[k] = [int(x) for x in nf]
    ctx.kernel_timing(False)
    assert frames["a"] == [F] * S and frames["b"] == [F] * S, (frames["a"], frames["b"])
    assert frames["a_ragged"] == rcounts and frames["c"] == rcounts
    med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    kavg = {k: ktime[k][0] / max(ktime[k][1], 1) * 1e3 for k in variants}  # us per launch
    kcall = {k: ktime[k][0] / args.iters * 1e3 for k in variants}            # us per call (c: 64 launches)
    r_ab = med["a"] / med["b"]
    r_k_eq = kavg["a"] / kavg["b"]
    r_k_rg = kavg["a_ragged"] / kavg["a"]
    res = dict(workload="tx datagrams 64 streams x 16 frames x 136 datagrams, fecblk 32, 24 losses, x16, device memory",
               ragged_counts_mean=float(np.mean(rcounts)), call_ms_median=med, call_ms_min={k: float(np.min(v)) * 1e3 for k, v in times.items()},
               interp_us_per_launch=kavg, interp_us_per_call=kcall,
               aim_a_over_b=dict(value=r_ab, aim="<= 1.05", met=bool(r_ab <= 1.05)),
               aim_ragged_equal_kernel_over_uniform=dict(value=r_k_eq, aim="within 2 %", met=bool(abs(r_k_eq - 1) <= 0.02)),
               aim_ragged12_kernel_over_equal16=dict(value=r_k_rg, samples_ratio=float(np.mean(rcounts)) / F, aim="<= 0.85", met=bool(r_k_rg <= 0.85)),
               c_over_a_ragged=med["c"] / med["a_ragged"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
