#!/usr/bin/env python3
"""Rx step of the headline shape (8 streams x 2^25 samples, decimate16_cen, 128 + 32) with per-stream centre frequencies and sample
rates set (sdrhip_rx_set_stream_meta) against the same bank with the shared record, in one process: the two handles take turns,
`rounds` times `steps` steps each behind a pre-roll, host clock between synchronisations.  One JSON line: the per-round step times
of both and their medians.
usage: python tools/bench_rx_stream_meta.py [--rounds 5] [--steps 100] [option=value ...]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import sdrdaemon_amd as sd  # noqa: E402
import signals  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--log2-samples", type=int, default=25)
    ap.add_argument("options", nargs="*", help="context options, key=value")
    a = ap.parse_args()
    ctx = sd.Context(0)
    for kv in a.options:
        k, v = kv.split("=")
        ctx.set_option(k, int(v) if v.lstrip("-").isdigit() else v)
    S, n = a.streams, 1 << a.log2_samples
    x = torch.stack([signals.hash_noise_torch(n, 1000 + s, "cuda") for s in range(S)])
    cfg = dict(log2decim=4, fcpos=sd.FC_CEN, hb_variant=sd.HB_EO1, sample_bits=16, nb_fec=32, center_frequency_khz=435000, sample_rate=625000)
    pipes = {"shared": sd.RxPipe(ctx, S, **cfg), "per_stream": sd.RxPipe(ctx, S, **cfg)}
    pipes["per_stream"].set_stream_meta([435000 + 1000 * s for s in range(S)], [625000 - 25000 * s for s in range(S)])
    times = {k: [] for k in pipes}
    frames = 0
    for r in range(a.rounds):
        for name, rx in pipes.items():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.25:  # (the clocks ramp over the first ~60 ms of load)
                for _ in range(5):
                    rx.process_view(x, 1, 0)
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                v = rx.process_view(x, 1, 0)
            torch.cuda.synchronize()
            times[name].append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
            frames = v.shape[1] * S
    res = {"bench": "rx_stream_meta", "streams": S, "log2_samples": a.log2_samples, "steps": a.steps, "frames_per_step": frames,
           "plan": pipes["per_stream"].last_plan()["path"], "ms_per_step": times,
           "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()}}
    res["per_stream_over_shared"] = round(res["median_ms"]["per_stream"] / res["median_ms"]["shared"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
