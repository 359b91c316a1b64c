"""The Rx pipe fed datagrams (sdrhip_rx_process_datagrams, device memory) on the hub's shape: 8 streams x 64 released frames per
call, incoming fecblk 32 with 24 erasures per frame in a different pattern each (the Tx benchmark's loss model), decimate16_cen,
outgoing nb_fec 32.  Two callers in one process, in alternating rounds:
  entry      the datagram call
  yardstick  sdrhip_fecbuf_write_and_read into device rows + sdrhip_rx_process_ragged on floor(n / 16) * 16 samples of each: the
             entries a caller had before, which drop the remainder of every call -- a time yardstick, not a correctness partner
A round is a window of at least --window seconds of back-to-back calls, the clock stops behind a device synchronisation; the
figure of a round is ms per call.  Afterwards a few rounds of the entry with the context's kernel timers on give the per-class
kernel times (they cost the stream a little, so the timed rounds above run without them).  Prints one JSON line.

    python tools/bench_rx_datagrams.py [--rounds N] [--window SECONDS] [--warmup W] [--out FILE]
Launches per call: run it under `rocprofv3 --kernel-trace --stats` in a run of its own (--rounds 1)."""
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

S, F, R_IN, LOST, L2, R_OUT = 8, 64, 32, 24, 4, 32
SPF = 16129


def batch(orc, rs):
    """per stream F frames (frame indices 0 .. F - 1) with LOST random losses each, arrival order: [S][n][512]"""
    per = []
    for s in range(S):
        row = []
        for f in range(F):
            fr = rs.randint(0, 256, (128, 512)).astype(np.uint8)
            fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3] = f, 0, np.arange(128), 0
            allb = np.concatenate([fr, orc.frame_encode(fr, R_IN)])
            keep = sorted(set(range(128 + R_IN)) - set(rs.choice(128 + R_IN, LOST, replace=False).tolist()))
            row += [allb[i] for i in keep]
        per.append(np.asarray(row))
    return np.stack(per), [p.shape[0] for p in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_rx_datagrams: no GPU")
    dg, nd = batch(Oracle(), np.random.RandomState(1))
    ctx = sd.Context(0)
    lib = ctx.lib
    P = C.c_void_p
    ddg = torch.from_numpy(dg).cuda()
    ndc = (C.c_size_t * S)(*nd)
    maxr = F + 1
    info = (sd.engine.FECBufferFrame * (S * maxr))()
    nr, nf = (C.c_size_t * S)(), (C.c_size_t * S)()
    sec, usec = (C.c_uint32 * S)(*[1] * S), (C.c_uint32 * S)()
    fb = (128 + R_OUT) * 512

    rx_a = sd.RxPipe(ctx, S, log2decim=L2, nb_fec=R_OUT)
    cap = max(rx_a.max_frames(SPF * maxr + 63), 1)
    frames = torch.empty((S, cap, 128 + R_OUT, 512), dtype=torch.uint8, device="cuda")

    def entry():
        check(lib.sdrhip_rx_process_datagrams(rx_a.h, P(ddg.data_ptr()), ndc, ddg.shape[1] * 512, sec, usec, maxr, P(frames.data_ptr()),
                                              cap * fb, info, nr, nf, sd.MEM_DEVICE))

    rx_b = sd.RxPipe(ctx, S, log2decim=L2, nb_fec=R_OUT)
    bank = sd.FECBufferBank(ctx, S)
    pitch = (maxr * SPF + 3) & ~3
    rows = torch.empty((S, pitch, 2), dtype=torch.int16, device="cuda")
    cnt = (C.c_size_t * S)()

    def yardstick():
        check(lib.sdrhip_fecbuf_write_and_read(bank.h, P(ddg.data_ptr()), ndc, ddg.shape[1] * 512, P(rows.data_ptr()), pitch * 4, None, maxr,
                                               info, nr, sd.MEM_DEVICE))
        for s in range(S):
            cnt[s] = (nr[s] * SPF) >> L2 << L2
        check(lib.sdrhip_rx_process_ragged(rx_b.h, P(rows.data_ptr()), cnt, pitch, sec, usec, P(frames.data_ptr()), cap * fb, nf, sd.MEM_DEVICE))

    callers = dict(entry=entry, yardstick=yardstick)
    for fn in callers.values():  # steady state: every later call releases the batch's F frames per stream
        for _ in range(max(args.warmup, 2)):
            fn()
        ctx.synchronize()
        assert list(nr) == [F] * S, list(nr)

    def window(fn):
        ctx.synchronize()
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.window:
            fn()
            n += 1
        ctx.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    ms = {k: [] for k in callers}
    for _ in range(args.rounds):
        for k, fn in callers.items():  # (alternating)
            ms[k].append(window(fn))
    classes = dict(decimate=sd.engine.K_DECIMATE, fec_encode=sd.engine.K_FEC_ENCODE, fec_decode=sd.engine.K_FEC_DECODE, convert=sd.engine.K_CONVERT)
    ctx.kernel_timing(True)
    for c in classes.values():
        ctx.kernel_timing_read(c)
    calls = 20
    for _ in range(calls):
        entry()
    ctx.synchronize()
    kt = {}
    for name, c in classes.items():
        t, n = ctx.kernel_timing_read(c)
        kt[name] = dict(ms_per_call=t / calls, launches_per_call=n / calls)
    ctx.kernel_timing(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(workload="rx datagrams: 8 streams x 64 released frames per call, fecblk 32 in, 24 erasures per frame, decimate16_cen, nb_fec 32 out, device memory",
               ms_per_call_median=med, ms_per_call_min={k: float(np.min(v)) for k, v in ms.items()},
               ms_per_call_max={k: float(np.max(v)) for k, v in ms.items()}, rounds=ms,
               entry_minus_yardstick_ms=med["entry"] - med["yardstick"],
               yardstick_spread_ms=float(np.max(ms["yardstick"]) - np.min(ms["yardstick"])),
               frames_out_per_call=[int(x) for x in nf], carry=[int(x) for x in rx_a.carry()], plan=rx_a.last_plan(),
               entry_kernel_classes=kt)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
