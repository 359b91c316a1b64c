"""Tagged datagram batches (sdrhip_{rx,tx}_submit_datagrams_tagged) against what a hub has to do without them, on the shape of
profiles/fecbuf_bench_64x16.json: 64 streams x 16 frames x 160 datagrams (fecblk 32) with 24 random losses per frame = 139 264
datagrams per batch.  The arrival order is a seeded random merge of the streams that keeps every stream's order.  Variants:
  A_host_sort        what a caller must do today: gather the arrival array into packed per-stream rows on a host core (a stable
                     argsort of the tags and numpy take along axis 0: this is the host sort measured), then the untagged
                     SDRHIP_PACKED submit from that pageable array
  B_tagged_pageable  the tagged submit from the pageable arrival array (one staging memcpy, demultiplexed on the device)
  C_tagged_inplace   the tagged submit in place from sdrhip_host_alloc memory (what recvmmsg into pinned memory gives)
Host clock around submit + collect(wait = 1) of one batch, median over --reps repetitions, the variants alternating.  Run for the
Rx pipe (decimate16_cen, nb_fec 32) and the Tx pipe (x1).  Prints one JSON line.

    python tools/bench_dgram_demux.py [--reps N] [--pipes rx,tx] [--out FILE]
KX's own time: `rocprofv3 --kernel-trace --stats -- python tools/bench_dgram_demux.py --reps 10`, a run of its own without
counters; dgram_demux_kernel stands next to the collector's copy pass (fecbuf_copy_*) in its kernel statistics."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_rx_datagrams_async import F, L, R_OUT, S, batch  # noqa: E402  (the same batch: 64 x 16 x 136 datagrams)

VARIANTS = ("A_host_sort", "B_tagged_pageable", "C_tagged_inplace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--pipes", default="rx,tx")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sdrdaemon_amd as sd
    from oracle_lib import Oracle
    from sdrdaemon_amd._lib import check

    if sd.device_count() <= 0:
        raise SystemExit("bench_dgram_demux: no GPU")
    ctx = sd.Context(0)
    lib = ctx.lib
    P, u16p = C.c_void_p, C.POINTER(C.c_uint16)
    per = batch(Oracle(), np.random.RandomState(1))
    nd = [p.shape[0] for p in per]
    n_total = sum(nd)
    tags = np.concatenate([np.full(n, s, np.uint16) for s, n in enumerate(nd)])
    np.random.RandomState(2).shuffle(tags)  # the arrival order: a random merge that keeps each stream's order
    arrival = np.empty((n_total, 512), np.uint8)
    for s, p in enumerate(per):
        arrival[tags == s] = p
    pinned = ctx.host_alloc((n_total, 512), np.uint8)
    pinned[:] = arrival
    ndc = (C.c_size_t * S)(*nd)
    tp = tags.ctypes.data_as(u16p)
    st = (C.c_uint32 * S)(*[7] * S)
    nr, nf = (C.c_size_t * S)(), (C.c_size_t * S)()
    maxr = F + 1
    info = (sd.engine.FECBufferFrame * (S * maxr))()
    res = dict(workload="tagged datagram batches: 64 streams x 16 frames x 136 of 160 datagrams (fecblk 32, 24 losses), arrival order = "
                        "seeded random merge; host clock around submit + collect(wait) of one batch; rx: decimate16_cen, nb_fec 32; tx: x1",
               datagrams=n_total, up_bytes_untagged=n_total * 512, up_bytes_tagged=n_total * 516, reps=args.reps, pipes={})

    for pipe in args.pipes.split(","):
        if pipe == "rx":
            fbytes, maxf = (128 + R_OUT) * 512, 3
            out = np.empty((S, maxf * fbytes), np.uint8)
            hs = {v: sd.RxPipe(ctx, S, log2decim=L, nb_fec=R_OUT) for v in VARIANTS}

            def submit(h, src, tagged):
                if tagged:
                    return lib.sdrhip_rx_submit_datagrams_tagged(h, P(src), tp, n_total, st, st)
                return lib.sdrhip_rx_submit_datagrams(h, P(src), ndc, 0, st, st)

            def collect(h):
                check(lib.sdrhip_rx_collect_datagrams(h, P(out.ctypes.data), maxf * fbytes, maxf, maxr, info, nr, nf, 1))
                return [int(x) for x in nr]
        else:
            ostride = (maxr * 16129 + 7) & ~7
            out = np.empty((S, ostride, 2), np.int16)
            b0 = np.empty((S, maxr, 508), np.uint8)
            hs = {v: sd.TxPipe(ctx, S, 0) for v in VARIANTS}

            def submit(h, src, tagged):
                if tagged:
                    return lib.sdrhip_tx_submit_datagrams_tagged(h, P(src), tp, n_total)
                return lib.sdrhip_tx_submit_datagrams(h, P(src), ndc, 0)

            def collect(h):
                check(lib.sdrhip_tx_collect_datagrams(h, P(out.ctypes.data), ostride, maxr, P(b0.ctypes.data), info, nf, 1))
                return [int(x) for x in nf]

        def run(v):
            h = hs[v].h
            t0 = time.perf_counter()
            if v == "A_host_sort":
                packed = np.take(arrival, np.argsort(tags, kind="stable"), axis=0)
                t1 = time.perf_counter()
                check(submit(h, packed.ctypes.data, False))
            else:
                t1 = t0
                check(submit(h, (arrival if v == "B_tagged_pageable" else pinned).ctypes.data, True))
            t2 = time.perf_counter()
            rel = collect(h)
            t3 = time.perf_counter()
            return t3 - t0, t1 - t0, t2 - t1, rel

        for v in VARIANTS:  # steady state: every later batch releases the batch's 16 frames per stream
            for _ in range(3):
                run(v)
        tot, sort, sub = ({v: [] for v in VARIANTS} for _ in range(3))
        for _ in range(args.reps):
            for v in VARIANTS:
                t, ts, tsub, rel = run(v)
                assert rel == [F] * S, (pipe, v, rel)
                tot[v].append(t)
                sort[v].append(ts)
                sub[v].append(tsub)
        med = {v: float(np.median(tot[v])) for v in VARIANTS}
        res["pipes"][pipe] = dict(
            batch_ms_median={v: med[v] * 1e3 for v in VARIANTS},
            batch_ms_min={v: float(np.min(tot[v])) * 1e3 for v in VARIANTS},
            host_sort_ms_median=float(np.median(sort["A_host_sort"])) * 1e3,
            submit_host_ms_median={v: float(np.median(sub[v])) * 1e3 for v in VARIANTS},
            datagrams_per_s={v: n_total / med[v] for v in VARIANTS},
            B_over_A=med["A_host_sort"] / med["B_tagged_pageable"], C_over_A=med["A_host_sort"] / med["C_tagged_inplace"])
        del hs
    res["shadow_mismatch"] = ctx.counter("fecbuf_shadow_mismatch")
    ctx.host_free(pinned)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
