"""Ragged Rx bank (sdrhip_rx_process_ragged) against the uniform call and against one-stream pipes, variants alternating in one
process, host clock around call + synchronise, medians of --iters (default 50):
  a  ragged call, equal counts, headline bank 8 x 2^25, device memory (the ragged kernels: K1mr with frame-direct stores)
  b  sdrhip_rx_process on the same input
  c  ragged, counts uniform in [0.5, 1] x 2^25 (mean 0.75), device memory
  d  8 one-stream pipes fed the variant-c counts
  e  64 streams x 1..4 TestSource-sized blocks (65 536 samples) each, host memory, one ragged call
  f  64 one-stream host calls for variant e
decimate16_cen, fecblk 32.  a-d call the C ABI in its zero-copy form (frames_out = NULL), e / f the Python host-memory entries.  Kernel times come from a rocprofv3 --kernel-trace --stats run of its own (--quick: fewer iterations).
Prints one JSON line (--out: also to a file).

    python tools/bench_rx_ragged.py [--iters N] [--warmup W] [--out FILE] [--quick]"""
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.iters, args.warmup = 5, 1
    import torch

    import sdrdaemon_amd as sd

    ctx = sd.Context(0)
    rs = np.random.RandomState(1)
    S, N, L, R = 8, 1 << 25, 4, 32
    cfg = dict(log2decim=L, fcpos=sd.FC_CEN, nb_fec=R)
    x = torch.randint(-32768, 32768, (S, N, 2), dtype=torch.int16, device="cuda")
    ragged = sd.RxPipe(ctx, S, **cfg)
    uniform = sd.RxPipe(ctx, S, **cfg)
    diverse = sd.RxPipe(ctx, S, **cfg)
    singles = [sd.RxPipe(ctx, 1, **cfg) for _ in range(S)]
    rows = [x[s] for s in range(S)]
    HS, B = 64, 65536
    hx = rs.randint(-32768, 32768, size=(HS, 4 * B, 2)).astype(np.int16)
    hrows = [np.ascontiguousarray(hx[s]) for s in range(HS)]
    hbank = sd.RxPipe(ctx, HS, **cfg)
    hsingles = [sd.RxPipe(ctx, 1, **cfg) for _ in range(HS)]
    ccounts = [[int(v) for v in rs.randint(N // 2, N + 1, size=S) // 4 * 4] for _ in range(args.iters + args.warmup)]
    ecounts = [[int(v) * B for v in rs.randint(1, 5, size=HS)] for _ in range(args.iters + args.warmup)]

    # a-d call the C ABI with frames_out = NULL (the zero-copy form): the library's time, not the Python wrappers' (a wrapper view of S
    # streams makes S tensors)
    import ctypes as C

    lib = ctx.lib
    xp, stride = C.c_void_p(x.data_ptr()), x.stride(0) // 2
    nf = (C.c_size_t * S)()
    nf1 = C.c_size_t(0)
    zeros = (C.c_uint32 * S)(*[0] * S)

    def ragged_call(h, counts, i):
        secs = (C.c_uint32 * S)(*[i] * S)
        sd._lib.check(lib.sdrhip_rx_process_ragged(h, xp, (C.c_size_t * S)(*counts), stride, secs, zeros, None, 0, nf, sd.MEM_DEVICE))

    def va(i):  # every stream the same count and stamp: the ragged kernels (K1mr frame-direct, the frame-list encoder)
        ragged_call(ragged.h, [N] * S, i)

    def vb(i):
        sd._lib.check(lib.sdrhip_rx_process(uniform.h, xp, N, stride, i, 0, None, 0, C.byref(nf1), sd.MEM_DEVICE))

    def vc(i):
        ragged_call(diverse.h, ccounts[i], i)

    def vd(i):
        for s in range(S):
            sd._lib.check(lib.sdrhip_rx_process(singles[s].h, C.c_void_p(rows[s].data_ptr()), ccounts[i][s], ccounts[i][s], i, 0, None, 0,
                                                C.byref(nf1), sd.MEM_DEVICE))

    def ve(i):
        hbank.process_ragged(hx, ecounts[i], i, 0)

    def vf(i):
        for s in range(HS):
            hsingles[s].process(hrows[s][:ecounts[i][s]], i, 0)

    variants = dict(a=va, b=vb, c=vc, d=vd, e=ve, f=vf)
    times = {k: [] for k in variants}
    for i in range(args.iters + args.warmup):
        for k, fn in variants.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            fn(i)
            ctx.synchronize()
            if i >= args.warmup:
                times[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
    res = {"metric": "ragged Rx bank, host clock around call + synchronise, median ms", "iters": args.iters,
           "shape": "a-d: 8 x 2^25 device, c/d counts uniform in [0.5, 1] x 2^25; e/f: 64 streams x 1..4 x 65536 host; decimate16_cen, fecblk 32",
           "ms": {k: round(v, 4) for k, v in med.items()},
           "ratios": {"a/b": round(med["a"] / med["b"], 3), "c/a": round(med["c"] / med["a"], 3), "d/c": round(med["d"] / med["c"], 3),
                      "f/e": round(med["f"] / med["e"], 3)},
           "plan_c": diverse.last_plan(), "plan_a": ragged.last_plan()}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
