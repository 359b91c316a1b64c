"""Throughput of the FEC buffer bank (sdrhip_fecbuf_write_and_read, device memory): 64 streams x 16 frames x 160 datagrams
(fecblk 32, 24 random losses per frame), against sdrhip_fec_decode_frames on the same frames collected on the host, and the
oracle's per-datagram collector (orc_fecbuffer) on one host core.  Prints one JSON line.

    python tools/bench_fecbuf.py [--iters N] [--warmup W] [--out FILE]
Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own (fecbuf_classify / scatter / copy kernels)."""
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
PB = 127 * 508


def batch(orc, rs):
    """[S][F * 136][512] datagrams (arrival order) and the first 128 arrivals of every frame [S * F][128][512]"""
    dg = np.empty((S, F * (128 + R - LOST), 512), np.uint8)
    first = np.empty((S * F, 128, 512), np.uint8)
    for s in range(S):
        row = []
        for f in range(F):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            allb = np.concatenate([fr, orc.frame_encode(fr, R)])
            keep = sorted(set(range(128 + R)) - set(rs.choice(128 + R, LOST, replace=False).tolist()))
            row += [allb[i] for i in keep]
            first[s * F + f] = allb[keep[:128]]
        dg[s] = np.asarray(row)
    return dg, first


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
        raise SystemExit("bench_fecbuf: no GPU")
    orc = Oracle()
    dg, first = batch(orc, np.random.RandomState(1))
    ctx = sd.Context(0)
    lib = ctx.lib
    bank = sd.FECBufferBank(ctx, S)
    ddg = torch.from_numpy(dg).cuda()
    dfirst = torch.from_numpy(first).cuda()
    maxf = F + 1
    data = torch.empty((S, maxf, PB), dtype=torch.uint8, device="cuda")
    b0 = torch.empty((S, maxf, 508), dtype=torch.uint8, device="cuda")
    info = (sd.engine.FECBufferFrame * (S * maxf))()
    nd = (C.c_size_t * S)(*([dg.shape[1]] * S))
    nf = (C.c_size_t * S)()
    pay = torch.empty((S * F, PB), dtype=torch.uint8, device="cuda")
    pb0 = torch.empty((S * F, 508), dtype=torch.uint8, device="cuda")

    def call_bank():
        check(lib.sdrhip_fecbuf_write_and_read(bank.h, C.c_void_p(ddg.data_ptr()), nd, dg.shape[1] * 512, C.c_void_p(data.data_ptr()),
                                                  maxf * PB, C.c_void_p(b0.data_ptr()), maxf, info, nf, sd.MEM_DEVICE))

    def call_decode():
        check(lib.sdrhip_fec_decode_frames(ctx.h, C.c_void_p(dfirst.data_ptr()), None, S * F, C.c_void_p(pay.data_ptr()),
                                              C.c_void_p(pb0.data_ptr()), sd.MEM_DEVICE))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.synchronize()
        t = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            t.append(time.perf_counter() - t0)
        return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3

    # alternate the two, twice, to see the spread
    bank_ms, dec_ms = [], []
    for _ in range(2):
        bank_ms.append(timed(call_bank))
        dec_ms.append(timed(call_decode))
    assert list(nf) == [F] * S, list(nf)
    # the decoded frames equal the bank's (frames 1..15 of a steady-state call are frames 0..14 of the batch)
    got = data[:, 1:F].cpu().numpy()
    exp = pay.view(S, F, PB)[:, :F - 1].cpu().numpy()
    same = bool(np.array_equal(got, exp))
    # oracle per-datagram collector, one host core, one stream
    ob = orc.fecbuffer()
    t0 = time.perf_counter()
    for d in dg[0]:
        ob.write_and_read(d)
    host_dps = dg.shape[1] / (time.perf_counter() - t0)
    ndg = S * dg.shape[1]
    stored = S * F * 128
    alg_bytes = ndg * 4 + stored * 512 * 2  # each header once, each stored datagram read and written once
    med = min(b[0] for b in bank_ms)
    res = dict(workload="fecbuf 64 streams x 16 frames x 160 datagrams, fecblk 32, 24 losses", datagrams_per_call=ndg,
               call_ms_median=[b[0] for b in bank_ms], call_ms_min=[b[1] for b in bank_ms],
               decode_precollected_ms_median=[d[0] for d in dec_ms], decode_precollected_ms_min=[d[1] for d in dec_ms],
               datagrams_per_s=ndg / (med * 1e-3), ratio_call_over_decode=med / min(d[0] for d in dec_ms),
               collection_alg_bytes=alg_bytes, collection_alg_bytes_at_8TBps_us=alg_bytes / 8e12 * 1e6,
               oracle_host_core_datagrams_per_s=host_dps, outputs_equal_precollected_decode=same)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
