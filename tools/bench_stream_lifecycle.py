#!/usr/bin/env python3
"""Per-stream lifecycle numbers -> profiles/stream_lifecycle.txt (DESIGN.md "Per-stream lifecycle").

1. The bank8 headline step (8 streams x 2^25 samples, decimate16 centred, fecblk 32, frames left in the frame area) of this
   build against the parent commit's libsdrhip.so, in interleaved processes (one process per repeat and library, A B A B ...):
   the feature adds nothing to that path, so this build must sit inside the run-to-run spread of the parent's own repeats.
2. The cost of sdrhip_rx_reset_streams between two headline steps: the host time of the call, and step + reset against the
   step alone on the same build.  8 of 8 keeps the bank aligned (the uniform step); 1 of 8 leaves it unaligned, so its partner
   is the ragged step sdrhip_rx_process falls back to, measured alone on the same unaligned bank.
3. sdrhip_rx_export_stream / sdrhip_rx_import_stream and the Tx pair: microseconds per stream and bytes moved.

usage: python tools/bench_stream_lifecycle.py --parent-lib PATH [--repeats 5] [--steps 100] [--log2-samples 25]
       (PATH: the parent commit's library, e.g. from `git worktree add ../parent HEAD~1` and
        `make -C ../parent/sdrdaemon_amd/csrc OUT=$PWD/../parent/libsdrhip.so`)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
S = 8


def bank(args):
    """the headline bank through the C ABI itself (plain ctypes: the parent commit's library lacks the entries the package binds)"""
    import torch

    import signals
    from sdrdaemon_amd import _lib

    lib = C.CDLL(_lib.LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    lib.sdrhip_last_error.restype = C.c_char_p
    lib.sdrhip_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.sdrhip_rx_create.argtypes = [vp, C.c_int, C.POINTER(_lib.RxConfig), C.POINTER(vp)]
    lib.sdrhip_rx_process.argtypes = [vp, vp, sz, sz, C.c_uint32, C.c_uint32, vp, sz, C.POINTER(sz), C.c_int]
    if hasattr(lib, "sdrhip_rx_reset_streams"):
        lib.sdrhip_rx_reset_streams.argtypes = [vp, C.POINTER(C.c_uint8)]
    n = 1 << args.log2_samples
    x = torch.stack([signals.hash_noise_torch(n, 1000 + s, "cuda") for s in range(S)])
    ctx, rx = vp(), vp()
    assert lib.sdrhip_ctx_create(0, None, C.byref(ctx)) == 0, lib.sdrhip_last_error()
    cfg = _lib.RxConfig(4, _lib.FC_CEN, _lib.HB_EO1, 16, 32, 435000, 625000)
    assert lib.sdrhip_rx_create(ctx, S, C.byref(cfg), C.byref(rx)) == 0, lib.sdrhip_last_error()
    nf = sz(0)
    ptr, stride = x.data_ptr(), x.stride(0) // 2

    def step():  # (the frames stay in the frame area, uniform and ragged step alike)
        rc = lib.sdrhip_rx_process(rx, ptr, n, stride, 1, 0, None, 0, C.byref(nf), _lib.MEM_DEVICE)
        assert rc == 0, lib.sdrhip_last_error()

    step.keep = x
    return lib, rx, step, torch


def loop_ms(torch, fn, steps):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def worker_headline(args):
    lib, rx, step, torch = bank(args)
    print(json.dumps({"step_ms": loop_ms(torch, step, args.steps)}))


def worker_reset(args):
    lib, rx, step, torch = bank(args)
    one, full = (C.c_uint8 * S)(0, 0, 0, 1, 0, 0, 0, 0), None
    call_us = {}

    def with_reset(mask, key):
        def fn():
            step()
            t = time.perf_counter()
            rc = lib.sdrhip_rx_reset_streams(rx, mask)
            call_us.setdefault(key, []).append((time.perf_counter() - t) * 1e6)
            assert rc == 0
        return fn

    out = {}
    for r in range(args.repeats):  # (interleaved on one bank; the partial reset comes last: it leaves the bank unaligned for good)
        out.setdefault("uniform_step_ms", []).append(loop_ms(torch, step, args.steps))
        out.setdefault("uniform_step_reset8_ms", []).append(loop_ms(torch, with_reset(full, "reset8_call_us"), args.steps))
    assert lib.sdrhip_rx_reset_streams(rx, one) == 0
    # (the ragged step alone, loop after loop from the moment the bank became unaligned: does its time settle?)
    out["ragged_step_series_ms"] = [loop_ms(torch, step, args.steps) for _ in range(8)]
    for r in range(args.repeats):
        out.setdefault("ragged_step_ms", []).append(loop_ms(torch, step, args.steps))
        out.setdefault("ragged_step_reset1_ms", []).append(loop_ms(torch, with_reset(one, "reset1_call_us"), args.steps))
    for k, v in call_us.items():
        out[k] = [statistics.median(v), min(v), max(v)]
    print(json.dumps(out))


def worker_move(args):
    import numpy as np
    import torch

    import sdrdaemon_amd as sd

    ctx = sd.Context(0)
    out = {}
    x = np.random.RandomState(1).randint(-32768, 32768, size=(S, 40000, 2)).astype(np.int16)
    rx = sd.RxPipe(ctx, S, log2decim=1, nb_fec=32)
    rx.process(x)  # (an open frame in every stream)
    tx = sd.TxPipe(ctx, S, 4)
    tx.process(np.zeros((S, 1, 128, 512), np.uint8))
    for kind, pipe in (("rx", rx), ("tx", tx)):
        blob = pipe.export_stream(0)
        te, ti = [], []
        for r in range(args.steps):
            s = r % S
            ctx.synchronize()
            t = time.perf_counter()
            blob = pipe.export_stream(s)
            te.append((time.perf_counter() - t) * 1e6)
            t = time.perf_counter()
            pipe.import_stream((s + 1) % S, blob)
            ti.append((time.perf_counter() - t) * 1e6)  # (the call returns without a synchronisation)
            ctx.synchronize()
        out[kind] = {"bytes": len(blob), "export_us": [statistics.median(te), min(te), max(te)],
                     "import_call_us": [statistics.median(ti), min(ti), max(ti)]}
    print(json.dumps(out))


def spawn(mode, args, lib=None):
    env = dict(os.environ)
    if lib:
        env["SDRHIP_LIB_PATH"] = lib
    else:
        env.pop("SDRHIP_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--steps", str(args.steps), "--repeats", str(args.repeats),
           "--log2-samples", str(args.log2_samples)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("worker %s failed (%d):\n%s" % (mode, r.returncode, r.stderr[-3000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--log2-samples", type=int, default=25)
    ap.add_argument("--worker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_lifecycle.txt"))
    args = ap.parse_args()
    if args.worker:
        return {"headline": worker_headline, "reset": worker_reset, "move": worker_move}[args.worker](args)
    lines = ["per-stream lifecycle (tools/bench_stream_lifecycle.py): MI355X, %d streams x 2^%d samples, decimate16 cen, fecblk 32, %d steps per figure"
             % (S, args.log2_samples, args.steps), ""]
    if args.parent_lib:
        a, b = [], []
        for r in range(args.repeats):  # (interleaved processes: parent, this build, parent, ...)
            a.append(spawn("headline", args, os.path.abspath(args.parent_lib))["step_ms"])
            b.append(spawn("headline", args)["step_ms"])
        inside = min(a) <= statistics.median(b) <= max(a)
        lines += ["1. headline step, interleaved processes",
                  "   parent commit  ms: " + " ".join("%.4f" % v for v in a) + "   (median %.4f, spread %.4f .. %.4f)" % (statistics.median(a), min(a), max(a)),
                  "   this build     ms: " + " ".join("%.4f" % v for v in b) + "   (median %.4f)" % statistics.median(b),
                  "   this build's median inside the parent's own spread: %s" % ("yes" if inside else "NO"), ""]
    else:
        lines += ["1. headline step against the parent commit: not measured (no --parent-lib)", ""]
    r = spawn("reset", args)
    med = {k: statistics.median(v) for k, v in r.items() if k.endswith("_ms")}
    series = r.pop("ragged_step_series_ms")
    lines += ["2. sdrhip_rx_reset_streams between two headline steps (one process, interleaved loops; ms per iteration, median of %d)" % args.repeats]
    for k in ("uniform_step_ms", "uniform_step_reset8_ms", "ragged_step_ms", "ragged_step_reset1_ms"):
        lines.append("   %-24s %.4f   (%s)" % (k, med[k], " ".join("%.4f" % v for v in r[k])))
    def added(with_key, alone_key):  # the medians' difference, and the spread the repeats leave open (us)
        w, al = r[with_key], r[alone_key]
        return ((med[with_key] - med[alone_key]) * 1e3, (min(w) - max(al)) * 1e3, (max(w) - min(al)) * 1e3)

    lines += ["   8 of 8: step + reset - step = %+.1f us (between %+.1f and %+.1f over the repeats);  the call itself %.1f us on the host (min %.1f, max %.1f)"
              % (added("uniform_step_reset8_ms", "uniform_step_ms") + tuple(r["reset8_call_us"])),
              "   1 of 8: step + reset - step = %+.1f us (between %+.1f and %+.1f over the repeats);  the call itself %.1f us on the host (min %.1f, max %.1f)"
              % (added("ragged_step_reset1_ms", "ragged_step_ms") + tuple(r["reset1_call_us"])),
              "           [partner: the ragged step of the unaligned bank.  That step has two levels: as fast as the uniform step behind ONE partial reset",
              "            (the series below, and the first ragged_step_ms repeat), slower once a loop with a partial reset per step has run (the later",
              "            repeats).  The spread above spans both; which state of the existing ragged step makes the difference was not isolated]",
              "   the ragged step alone, eight loops in a row from the first step behind the partial reset: " + " ".join("%.4f" % v for v in series), ""]
    m = spawn("move", args)
    lines += ["3. export / import of one stream (export: gather + one copy + one synchronisation; import: the call, no synchronisation)"]
    for kind in ("rx", "tx"):
        lines.append("   %s: %d bytes   export %.1f us (min %.1f, max %.1f)   import call %.1f us (min %.1f, max %.1f)"
                     % ((kind, m[kind]["bytes"]) + tuple(m[kind]["export_us"]) + tuple(m[kind]["import_call_us"])))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
