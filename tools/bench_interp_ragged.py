"""The sample-fed ragged interpolator entry (sdrhip_interpolate_ragged, K5c; device memory, x16) on the shape of
tools/bench_tx_datagrams.py: 64 streams x 16 frames of 16 129 samples.  Host clock around call + synchronise, the interpolator's own
time from the context's kernel timers (hipEvents around its launches); the variants alternate in one process, medians over --iters
rounds, and the first variant runs twice per round (a, a2) so that the spread between two runs of the same thing stands beside the
differences:
  a   the ragged entry at equal counts of 16 x 16129 (the compact grid on the uniform call's work)
  b   the uniform sdrhip_interpolate at the same size
  c   the ragged entry at counts of 8..16 frames' worth per stream (random, mean ~12)
  d   what a caller does today at those counts: 64 one-stream sdrhip_interpolate calls
Prints one JSON line.

    python tools/bench_interp_ragged.py [--iters N] [--warmup W] [--out FILE]"""
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

S, F, L2 = 64, 16, 4
SPF = 16129


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    import signals
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_interp_ragged: no GPU")
    rs = np.random.RandomState(1)
    frames = [int(x) for x in rs.randint(8, F + 1, S)]
    eq, rg = [F * SPF] * S, [f * SPF for f in frames]
    ctx = sd.Context(0)
    lib = ctx.lib
    n = F * SPF
    istride, ostride = (n + 3) & ~3, ((n << L2) + 3) & ~3
    x = torch.empty((S, istride, 2), dtype=torch.int16, device="cuda")
    x[:, :n] = signals.hash_noise_torch(S * n, 5, "cuda").reshape(S, n, 2)
    out = torch.empty((S, ostride, 2), dtype=torch.int16, device="cuda")
    P, sz = C.c_void_p, C.c_size_t
    n_out = (sz * S)()
    banks = {k: sd.Interpolators(ctx, S) for k in ("a", "a2", "b", "c")}
    ones = [sd.Interpolators(ctx, 1) for _ in range(S)]
    c_eq, c_rg = (sz * S)(*eq), (sz * S)(*rg)

    def ragged(bank, counts):
        def call():
            check(lib.sdrhip_interpolate_ragged(bank.h, L2, P(x.data_ptr()), counts, istride, P(out.data_ptr()), ostride, n_out, sd.MEM_DEVICE))
        return call

    def call_b():
        check(lib.sdrhip_interpolate(banks["b"].h, L2, P(x.data_ptr()), n, istride, P(out.data_ptr()), ostride, None, sd.MEM_DEVICE))

    def call_d():
        for s in range(S):
            check(lib.sdrhip_interpolate(ones[s].h, L2, P(x[s].data_ptr()), rg[s], 0, P(out[s].data_ptr()), 0, None, sd.MEM_DEVICE))

    variants = dict(a=ragged(banks["a"], c_eq), b=call_b, c=ragged(banks["c"], c_rg), d=call_d, a2=ragged(banks["a2"], c_eq))
    for fn in variants.values():
        for _ in range(max(args.warmup, 2)):
            fn()
    ctx.synchronize()
    plans = {k: banks[k].last_plan() for k in banks}
    ctx.kernel_timing(True)
    times = {k: [] for k in variants}
    ktime = {k: [] for k in variants}
    for _ in range(args.iters):
        for k, fn in variants.items():  # (alternating)
            ctx.kernel_timing_read(sd.engine.K_INTERPOLATE)
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            times[k].append(time.perf_counter() - t0)
            ktime[k].append(ctx.kernel_timing_read(sd.engine.K_INTERPOLATE)[0])  # ms of the call's launches (d: 64 of them)
    ctx.kernel_timing(False)
    med = {k: float(np.median(v)) * 1e6 for k, v in times.items()}       # us per call
    kmed = {k: float(np.median(v)) * 1e3 for k, v in ktime.items()}      # us of interpolator launches per call (the timers say ms)
    samples_ratio = float(sum(rg)) / float(sum(eq))
    res = dict(workload="interpolator bank, 64 streams, x16, device memory; equal counts 16 x 16129, ragged counts 8..16 x 16129",
               ragged_frames_mean=float(np.mean(frames)), samples_ratio_c_over_a=samples_ratio, plans=plans,
               call_us_median=med, call_us_min={k: float(np.min(v)) * 1e6 for k, v in times.items()}, launch_us_median=kmed,
               spread_a2_over_a=dict(call=med["a2"] / med["a"], launch=kmed["a2"] / kmed["a"]),
               a_over_b=dict(call=med["a"] / med["b"], launch=kmed["a"] / kmed["b"]),
               c_over_a_launch=dict(value=kmed["c"] / kmed["a"], samples_ratio=samples_ratio, call=med["c"] / med["a"]),
               d_over_c=dict(call=med["d"] / med["c"], launch=kmed["d"] / kmed["c"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
