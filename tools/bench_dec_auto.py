#!/usr/bin/env python3
"""Batched CM256 decode under dec_max_rows = 32 | 128 | auto: the decode chain's time per call (sdrhip_ctx_kernel_timing class
SDRHIP_K_FEC_DECODE, whose timer brackets every launch of the chain) on 1024 device-resident frames, for three kinds of input:
  a  24 erasures per frame, recovery rows < 32 (the Tx benchmark's pattern): nothing is deferred
  b  like a, but every 16th frame comes from a fecblk-64 sender: 24 erasures repaired with rows 40..63
  c  every frame 40 erasures, rows 0..63: everything is deferred
The variants alternate inside every round; the figure of a variant is the median over the rounds of the round's mean per call.
dec_max_rows = 32 is a legal promise on input a only.  Every (input, variant) pair is checked once against the originals.
usage: python tools/bench_dec_auto.py [--variants 32,128,auto] [--inputs a,b,c] [--frames 1024] [--rounds 9] [--steps 100]
                                      [--label NAME] [--out FILE]      (SDRHIP_LIB_PATH=... selects another build of the library)"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sdrdaemon_amd as sd  # noqa: E402
from sdrdaemon_amd.engine import K_FEC_DECODE, MEM_DEVICE, _ptr, check  # noqa: E402


def make_inputs(ctx, F, which):
    """-> {name: (rx (F, 128, 512) on the device, originals' payload (F, 127 * 508), frames deferred under auto)}"""
    g = torch.Generator(device="cuda")
    g.manual_seed(2024)
    frames = torch.randint(0, 256, (F, 128, 512), dtype=torch.uint8, device="cuda", generator=g)
    fi = torch.arange(F, device="cuda")
    frames[:, :, 0] = (fi & 0xff).to(torch.uint8)[:, None]
    frames[:, :, 1] = ((fi >> 8) & 0xff).to(torch.uint8)[:, None]
    frames[:, :, 2] = torch.arange(128, device="cuda", dtype=torch.uint8)[None]
    frames[:, :, 3] = 0
    rec = sd.fec_encode_frames(ctx, frames, 64)
    allb = torch.cat([frames, rec], dim=1)
    want = frames[:, 1:, 4:].reshape(F, 127 * 508).contiguous()
    rs = np.random.RandomState(7)
    out = {}
    for name in which:
        order = np.zeros((F, 128), np.int64)
        ndef = 0
        for f in range(F):
            if name == "c":
                lost, rows = rs.choice(128, 40, replace=False), rs.choice(64, 40, replace=False)
            elif name == "b" and f % 16 == 15:
                lost, rows = rs.choice(128, 24, replace=False), 40 + rs.choice(24, 24, replace=False)
            else:
                lost, rows = rs.choice(128, 24, replace=False), rs.choice(32, 24, replace=False)
            ndef += int(len(rows) > 32 or rows.max() >= 32)
            order[f] = np.concatenate([np.setdiff1d(np.arange(128), lost), 128 + np.sort(rows)])
        idx = torch.from_numpy(order).cuda()
        out[name] = (allb[fi[:, None], idx].contiguous(), want, ndef)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="32,128,auto")
    ap.add_argument("--inputs", default="a,b,c")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--label", default="lib")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sd.Context(0)
    F = a.frames
    inputs = make_inputs(ctx, F, a.inputs.split(","))
    payload = torch.empty((F, 127 * 508), dtype=torch.uint8, device="cuda")
    b0 = torch.empty((F, 508), dtype=torch.uint8, device="cuda")

    def decode(rx):
        check(ctx.lib.sdrhip_fec_decode_frames(ctx.h, _ptr(rx), C.c_void_p(0), F, _ptr(payload), _ptr(b0), MEM_DEVICE))

    pairs = [(i, v) for i in inputs for v in a.variants.split(",") if not (v == "32" and i != "a")]
    for i, v in pairs:  # every pair once against the originals
        ctx.set_option("dec_max_rows", v)
        payload.zero_()
        d0 = ctx.counter("dec_deferred") if v == "auto" else 0
        decode(inputs[i][0])
        ctx.synchronize()
        assert torch.equal(payload, inputs[i][1]), (i, v)
        if v == "auto":
            assert ctx.counter("dec_deferred") - d0 == inputs[i][2], (i, inputs[i][2])
    ms = {p: [] for p in pairs}
    ctx.set_option("ktime_stride", 1)
    for _ in range(a.rounds):
        for i, v in pairs:
            ctx.set_option("dec_max_rows", v)
            for _ in range(10):
                decode(inputs[i][0])
            ctx.synchronize()
            ctx.kernel_timing(True)
            for _ in range(a.steps):
                decode(inputs[i][0])
            ctx.synchronize()
            t, k = ctx.kernel_timing_read(K_FEC_DECODE)
            ctx.kernel_timing(False)
            ms[(i, v)].append(t / max(k, 1))
    lines = ["# %s: %d frames per call, %d rounds x %d calls, median (min .. max) of the rounds' means, ms per call" % (a.label, F, a.rounds, a.steps)]
    for i, v in pairs:
        r = ms[(i, v)]
        lines.append("%-16s input %s (%4d deferred)  dec_max_rows = %-4s  %.4f  (%.4f .. %.4f)" %
                     (a.label, i, inputs[i][2] if v == "auto" else 0, v, statistics.median(r), min(r), max(r)))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
