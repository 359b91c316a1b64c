"""The decimator taps (sdrhip_decimate_taps, K1t) against what serves the same outputs without them, on 8 streams of 2^22 and of
2^25 samples of `hash` noise in device memory, for the masks {2,4,6}, {3,4} and {1,2,3,4,5,6}:
  a   one sdrhip_decimate_taps call
  b   one bank per tap, one sdrhip_decimate(k, CEN) each, default decim_path (the matrix-core cascade where it is admitted)
  c   sdrhip_decimate_ragged(L, CEN) with decim_path = valu: K1r, the cascade K1t is built on -- a over c is the price of the taps
  a2  a again (the A/A pair: the spread between two runs of the same thing)
Host clock around call(s) + synchronise, the cascades' own time from the context's kernel timers (hipEvents around the launches); the
variants alternate in every round of one process, medians and min / max over --iters rounds after --warmup rounds.  Prints one JSON
line per (size, mask).

    python tools/bench_decim_taps.py [--iters N] [--warmup W] [--log2n 22 25] [--out FILE]"""
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

S = 8
MASKS = [(2, 4, 6), (3, 4), (1, 2, 3, 4, 5, 6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2n", type=int, nargs="+", default=[22, 25])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    import signals
    from sdrdaemon_amd import _lib
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_decim_taps: no GPU")
    ctx = sd.Context(0)
    lib = ctx.lib
    P, sz = C.c_void_p, C.c_size_t
    lines = []
    for log2n in args.log2n:
        n = 1 << log2n
        x = signals.hash_noise_torch(S * n, 5, "cuda").reshape(S, n, 2)
        out = {k: torch.empty((S, n >> k, 2), dtype=torch.int16, device="cuda") for k in range(1, 7)}
        counts, n_out = (sz * S)(*[n] * S), (sz * S)()
        for mask in MASKS:
            L, bits = max(mask), sum(1 << k for k in mask)
            taps = _lib.DecimTaps()
            for k in mask:
                taps.iq_out[k], taps.out_stride[k] = out[k].data_ptr(), n >> k
            bank = {v: sd.Decimators(ctx, S) for v in ("a", "a2", "c")}
            per_tap = {k: sd.Decimators(ctx, S) for k in mask}

            def call_taps(b):
                def call():
                    check(lib.sdrhip_decimate_taps(b.h, bits, 16, P(x.data_ptr()), counts, n, C.byref(taps), n_out, sd.MEM_DEVICE))
                return call

            def call_b():
                for k in mask:
                    ss = C.c_uint(16)
                    check(lib.sdrhip_decimate(per_tap[k].h, k, sd.FC_CEN, C.byref(ss), P(x.data_ptr()), n, n, P(out[k].data_ptr()), n >> k, None,
                                              sd.MEM_DEVICE))

            def call_c():
                ss = C.c_uint(16)
                check(lib.sdrhip_decimate_ragged(bank["c"].h, L, sd.FC_CEN, C.byref(ss), P(x.data_ptr()), counts, n, P(out[L].data_ptr()), n >> L,
                                                 n_out, sd.MEM_DEVICE))

            variants = dict(a=call_taps(bank["a"]), b=call_b, c=call_c, a2=call_taps(bank["a2"]))
            path = dict(a="auto", b="auto", c="valu", a2="auto")  # (a context option: set outside the timed region)
            times, ktime, plans = {v: [] for v in variants}, {v: [] for v in variants}, {}
            ctx.kernel_timing(True)
            for it in range(args.warmup + args.iters):
                for v, fn in variants.items():  # (alternating)
                    ctx.set_option("decim_path", path[v])
                    ctx.kernel_timing_read(sd.engine.K_DECIMATE)
                    t0 = time.perf_counter()
                    fn()
                    ctx.synchronize()
                    dt = time.perf_counter() - t0
                    kt = ctx.kernel_timing_read(sd.engine.K_DECIMATE)[0]
                    if it >= args.warmup:
                        times[v].append(dt * 1e6)
                        ktime[v].append(kt * 1e3)
            ctx.kernel_timing(False)
            ctx.set_option("decim_path", "auto")
            plans = {"a": bank["a"].last_plan(), "c": bank["c"].last_plan(), "b": {str(k): per_tap[k].last_plan()["path"] for k in mask}}

            def stats(d):
                return {v: dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))) for v, t in d.items()}
            call, launch = stats(times), stats(ktime)
            in_bytes, out_bytes = 4 * S * n, sum(4 * S * (n >> k) for k in mask)
            res = dict(workload="decimator bank, %d streams x 2^%d samples, device memory" % (S, log2n), mask=list(mask), iters=args.iters,
                       warmup=args.warmup, plans=plans, call_us=call, launch_us=launch,
                       a_over_b=dict(call=call["a"]["median"] / call["b"]["median"], launch=launch["a"]["median"] / launch["b"]["median"]),
                       a_over_c=dict(call=call["a"]["median"] / call["c"]["median"], launch=launch["a"]["median"] / launch["c"]["median"]),
                       spread_a2_over_a=dict(call=call["a2"]["median"] / call["a"]["median"], launch=launch["a2"]["median"] / launch["a"]["median"]),
                       a_bytes=in_bytes + out_bytes, a_gbps_launch=(in_bytes + out_bytes) / launch["a"]["median"] / 1e3)
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
            del bank, per_tap
        del x, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
