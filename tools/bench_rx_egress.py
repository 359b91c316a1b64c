"""Departure-order egress (sdrhip_rx_set_egress / sdrhip_rx_collect_egress) against the stream-order collect, on the shape of
tools/bench_rx_datagrams_async.py: 64 streams x 16 frames x 136 datagrams per batch (incoming fecblk 32, 24 random losses per
frame), decimate16_cen, nb_fec 32, depth 4, packed sdrhip_host_alloc input uploaded in place: every batch releases 16 payloads and
completes one frame per stream (64 x 160 datagrams delivered).  Variants, alternating rounds, medians on the host clock:
  off          order off: sdrhip_rx_collect_datagrams into the caller's rows (one memcpy per stream)
  off_parent   the same calls through a library built from the parent commit (--parent-lib): the yardstick
  on           SDRHIP_EGRESS_ROUND_ROBIN: sdrhip_rx_collect_egress lends the array, the next collect releases it
1. batch period of each variant; 2. KR against KD per batch (kernel timers, class K_CONVERT: nothing else of these batches runs in
it); 3. host time of the collect call on a batch that has finished: per-stream memcpy against lent.

    python tools/bench_rx_egress.py [--rounds N] [--batches B] [--parent-lib libsdrhip.so] [--out profiles/rx_egress_ab.txt]"""
import argparse
import ctypes as C
import datetime
import hashlib
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_rx_datagrams_async import DEPTH, F, L, R_OUT, S, batch  # noqa: E402  (the same input)


class ParentRx:
    """asynchronous datagram batches of another build of the library (the parent commit's), through its C ABI alone"""

    def __init__(self, path, cfg, dgrams):
        P, sz, u32 = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
        self.lib = lib = C.CDLL(path)
        lib.sdrhip_last_error.restype = C.c_char_p
        lib.sdrhip_ctx_create.argtypes = [C.c_int, P, C.POINTER(P)]
        lib.sdrhip_rx_create.argtypes = [P, C.c_int, P, C.POINTER(P)]
        lib.sdrhip_rx_set_async.argtypes = [P, C.c_int, C.c_int]
        lib.sdrhip_rx_submit_datagrams.argtypes = [P, P, C.POINTER(sz), sz, u32, u32]
        lib.sdrhip_rx_collect_datagrams.argtypes = [P, P, sz, sz, sz, P, C.POINTER(sz), C.POINTER(sz), C.c_int]
        self.ctx, self.h = P(), P()
        self.check(lib.sdrhip_ctx_create(0, P(0), C.byref(self.ctx)))
        self.check(lib.sdrhip_rx_create(self.ctx, S, C.cast(C.byref(cfg), P), C.byref(self.h)))
        self.check(lib.sdrhip_rx_set_async(self.h, DEPTH, 1))
        # the same datagrams in pinned memory of ITS allocator (a library uploads in place only what its own sdrhip_host_alloc gave)
        lib.sdrhip_host_alloc.argtypes = [P, sz]
        lib.sdrhip_host_alloc.restype = P
        self.pinned = lib.sdrhip_host_alloc(self.ctx, dgrams.nbytes)
        if not self.pinned:
            raise RuntimeError("parent library: sdrhip_host_alloc")
        C.memmove(self.pinned, dgrams.ctypes.data, dgrams.nbytes)

    def check(self, rc):
        if rc:
            raise RuntimeError("parent library: %d %s" % (rc, self.lib.sdrhip_last_error().decode()))


def head(path):
    with open(path, "rb") as fh:
        return "%s  sha256 %s  %d bytes" % (os.path.relpath(path, ROOT), hashlib.sha256(fh.read()).hexdigest()[:16], os.path.getsize(path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import sdrdaemon_amd as sd
    from oracle_lib import Oracle
    from sdrdaemon_amd import _lib
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_rx_egress: no GPU")
    ctx = sd.Context(0)
    lib = ctx.lib
    P = C.c_void_p
    per = batch(Oracle(), np.random.RandomState(1))
    nd = [p.shape[0] for p in per]
    ndc = (C.c_size_t * S)(*nd)
    pinned = ctx.host_alloc((sum(nd), 512), np.uint8)
    pinned[:] = np.concatenate(per)
    B = 128 + R_OUT
    fbytes = B * 512
    maxf, maxr = 3, F + 1
    out = np.empty((S, maxf * fbytes), np.uint8)
    info = (sd.engine.FECBufferFrame * (S * maxr))()
    nr, nf = (C.c_size_t * S)(), (C.c_size_t * S)()
    st = (C.c_uint32 * S)(*[7] * S)
    eg = _lib.RxEgress()
    rxs = {v: sd.RxPipe(ctx, S, log2decim=L, nb_fec=R_OUT) for v in ("off", "on")}
    for rx in rxs.values():
        rx.set_async(depth=DEPTH)
    rxs["on"].set_egress("round_robin")
    parent = ParentRx(args.parent_lib, rxs["off"].cfg, pinned) if args.parent_lib else None
    collect_s = {"off": [], "on": []}  # host time of a collect call whose batch had finished

    def collect(v, l, h, chk):
        if v == "on":
            chk(l.sdrhip_rx_collect_egress(h, C.byref(eg), nf, maxr, info, nr, 1))
        else:
            chk(l.sdrhip_rx_collect_datagrams(h, P(out.ctypes.data), maxf * fbytes, maxf, maxr, info, nr, nf, 1))

    def run(n, v, l=lib, h=None, chk=check, src=None):
        h = h or rxs[v].h
        src = src or pinned.ctypes.data
        sub = col = 0
        while col < n:
            if sub < n:
                rc = l.sdrhip_rx_submit_datagrams(h, P(src), ndc, 0, st, st)
                if rc == 0:
                    sub += 1
                    continue
                if rc != -6:
                    chk(rc)
            collect(v, l, h, chk)
            col += 1
        if v == "on":
            chk(l.sdrhip_rx_release_egress(h))

    fns = dict(off=lambda n: run(n, "off"))
    if parent:
        fns["off_parent"] = lambda n: run(n, "off", parent.lib, parent.h, parent.check, parent.pinned)
    fns["on"] = lambda n: run(n, "on")
    for fn in fns.values():  # steady state: every later batch releases 16 frames and completes one frame per stream
        fn(3)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn(args.batches)
            times[k].append((time.perf_counter() - t0) / args.batches)
            assert [int(x) for x in nr] == [F] * S and [int(x) for x in nf] == [1] * S, (k, list(nr), list(nf))
    assert eg.blocks_per_frame == B
    # 2. the delivery kernel on its own: KD (off) against KR (on)
    kern = {}
    for v in ("off", "on"):
        ctx.synchronize()
        ctx.kernel_timing(True)
        ctx.kernel_timing_read(sd.engine.K_CONVERT)
        fns[v](args.batches)
        ms, n = ctx.kernel_timing_read(sd.engine.K_CONVERT)
        ctx.kernel_timing(False)
        kern[v] = dict(us_per_launch=ms / max(n, 1) * 1e3, launches_per_batch=n / args.batches)
    # 3. the host time of the collect call alone: one batch, finished on the device before the call
    for _ in range(args.rounds * 2):
        for v in ("off", "on"):
            check(lib.sdrhip_rx_submit_datagrams(rxs[v].h, P(pinned.ctypes.data), ndc, 0, st, st))
            ctx.synchronize()
            t0 = time.perf_counter()
            collect(v, lib, rxs[v].h, check)
            collect_s[v].append(time.perf_counter() - t0)
    check(lib.sdrhip_rx_release_egress(rxs["on"].h))
    med = {k: float(np.median(v)) for k, v in times.items()}
    down = S * fbytes + S * F * 16
    res = dict(workload="rx datagram batches: 64 streams x 16 frames x 136 datagrams (fecblk 32, 24 losses) -> decimate16_cen, nb_fec 32, "
                        "pinned packed input in place, depth %d; %d datagrams delivered per batch" % (DEPTH, S * B),
               batches_per_run=args.batches, rounds=args.rounds, down_bytes=down,
               batch_ms_median={k: v * 1e3 for k, v in med.items()},
               batch_ms_rounds={k: [round(x * 1e3, 4) for x in v] for k, v in times.items()},
               on_over_off=med["on"] / med["off"],
               delivery_kernel=kern,
               delivery_GBps={v: 2 * down / (kern[v]["us_per_launch"] * 1e-6) / 1e9 if kern[v]["us_per_launch"] else 0.0 for v in kern},
               collect_call_host_us_median={v: float(np.median(t)) * 1e6 for v, t in collect_s.items()},
               collect_call_host_us_min={v: float(np.min(t)) * 1e6 for v, t in collect_s.items()},
               shadow_mismatch=ctx.counter("fecbuf_shadow_mismatch"))
    if parent:
        res["off_over_off_parent"] = med["off"] / med["off_parent"]
        res["on_over_off_parent"] = med["on"] / med["off_parent"]
    ctx.host_free(pinned)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("Departure-order egress (KR, sdrhip_rx_collect_egress) against the stream-order collect (KD, sdrhip_rx_collect_datagrams):\n"
                     "tools/bench_rx_egress.py, alternating rounds, medians on the host clock.\n")
            fh.write("box: %s, %s, torch %s\n" % (torch.cuda.get_device_name(0), platform.platform(), torch.__version__))
            fh.write("date: %s\n" % datetime.datetime.now().strftime("%Y-%m-%d %H:%M"))
            fh.write("library: %s\n" % head(_lib.LIB_PATH))
            if args.parent_lib:
                fh.write("parent library (off_parent): sha256 %s\n" % hashlib.sha256(open(args.parent_lib, "rb").read()).hexdigest()[:16])
            fh.write("\n%s\n\n" % res["workload"])
            fh.write("1. batch period, ms (median of %d rounds of %d batches)\n" % (args.rounds, args.batches))
            for k in times:
                fh.write("   %-11s %.4f   rounds: %s\n" % (k, med[k] * 1e3, " ".join("%.4f" % (x * 1e3) for x in times[k])))
            fh.write("   on / off = %.4f" % res["on_over_off"])
            if parent:
                fh.write("   off / off_parent = %.4f   on / off_parent = %.4f" % (res["off_over_off_parent"], res["on_over_off_parent"]))
            fh.write("\n2. delivery kernel per batch (kernel timers, K_CONVERT), %d bytes in and out\n" % down)
            for v, name in (("off", "KD"), ("on", "KR")):
                fh.write("   %s  %.2f us per launch, %.2f launches per batch, %.0f GB/s read + written\n"
                         % (name, kern[v]["us_per_launch"], kern[v]["launches_per_batch"], res["delivery_GBps"][v]))
            fh.write("3. host time of the collect call on a finished batch, us (median / min of %d)\n" % len(collect_s["off"]))
            fh.write("   off (one memcpy per stream into the caller's rows)  %.1f / %.1f\n"
                     % (res["collect_call_host_us_median"]["off"], res["collect_call_host_us_min"]["off"]))
            fh.write("   on  (lent: records copied, nothing else)            %.1f / %.1f\n"
                     % (res["collect_call_host_us_median"]["on"], res["collect_call_host_us_min"]["on"]))
            fh.write("shadow mismatches: %d\n\n%s\n" % (res["shadow_mismatch"], line))


if __name__ == "__main__":
    main()
