"""The paced departure order (SDRHIP_EGRESS_PACED, KP) against round robin (KR), every bank driven through the C ABI alone so that a
library built from the parent commit (--parent-lib) runs the same calls.  Variants, alternating rounds, medians on the host clock:
  rr_parent   SDRHIP_EGRESS_ROUND_ROBIN through the parent commit's library: the yardstick
  rr          SDRHIP_EGRESS_ROUND_ROBIN through this library
  paced       SDRHIP_EGRESS_PACED through this library
Shapes:
  equal    the shape of tools/bench_rx_egress.py: datagram batches, 64 streams x 16 frames x 136 datagrams (incoming fecblk 32, 24
           random losses per frame), decimate16_cen, nb_fec 32, depth 4, packed sdrhip_host_alloc input uploaded in place; every
           batch completes one frame per stream, so the paced and the round-robin arrays are identical
  unequal  ragged sample batches, 64 streams, decimate2_cen, nb_fec 32, depth 4, packed sdrhip_host_alloc input in place: stream 0
           completes four frames per batch, every other stream one
Per shape: 1. batch period; 2. the delivery kernel (kernel timers, class K_CONVERT, per batch: nothing else of a datagram batch
runs in it; a ragged batch's input unpack does, the same launch in all three columns), one figure per round, so that the difference between KP and KR stands next to the spread of KR's own rounds; 3. host time of a submit
call that found a free slot (it builds the order's table and tags); 4. from the tags alone: the longest run of one stream's
datagrams, and the most datagrams of one stream among any 64 consecutive entries (one per stream is the even share), under both
orders.

    python tools/bench_rx_egress_paced.py [--rounds N] [--batches B] [--parent-lib libsdrhip.so] [--out profiles/rx_egress_paced_ab.txt]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_rx_datagrams_async import DEPTH, F, L, R_OUT, S, SPF, batch  # noqa: E402  (the same input)

K_CONVERT = 4
RR, PACED = 1, 2
P, SZ = C.c_void_p, C.c_size_t


class Egress(C.Structure):  # sdrhip_rx_egress
    _fields_ = [("dgrams", P), ("stream_of", P), ("n_dgrams", SZ), ("blocks_per_frame", SZ)]


class Library:
    """one build of the library and a context of it"""

    def __init__(self, path):
        u32 = C.POINTER(C.c_uint32)
        self.path = path
        self.lib = lib = C.CDLL(path)
        lib.sdrhip_last_error.restype = C.c_char_p
        lib.sdrhip_ctx_create.argtypes = [C.c_int, P, C.POINTER(P)]
        lib.sdrhip_ctx_synchronize.argtypes = [P]
        lib.sdrhip_ctx_kernel_timing.argtypes = [P, C.c_int]
        lib.sdrhip_ctx_kernel_timing_read.argtypes = [P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint)]
        lib.sdrhip_host_alloc.argtypes = [P, SZ]
        lib.sdrhip_host_alloc.restype = P
        lib.sdrhip_rx_create.argtypes = [P, C.c_int, P, C.POINTER(P)]
        lib.sdrhip_rx_set_async.argtypes = [P, C.c_int, C.c_int]
        lib.sdrhip_rx_set_egress.argtypes = [P, C.c_int]
        lib.sdrhip_rx_submit_datagrams.argtypes = [P, P, C.POINTER(SZ), SZ, u32, u32]
        lib.sdrhip_rx_submit_ragged.argtypes = [P, P, C.POINTER(SZ), SZ, u32, u32]
        lib.sdrhip_rx_collect_egress.argtypes = [P, C.POINTER(Egress), C.POINTER(SZ), SZ, P, C.POINTER(SZ), C.c_int]
        lib.sdrhip_rx_release_egress.argtypes = [P]
        self.ctx = P()
        self.check(lib.sdrhip_ctx_create(0, P(0), C.byref(self.ctx)))

    def check(self, rc):
        if rc:
            raise RuntimeError("%s: %d %s" % (os.path.basename(os.path.dirname(self.path)), rc, self.lib.sdrhip_last_error().decode()))

    def pinned(self, a):
        """a copy of `a` in this library's own pinned memory (a library uploads in place only what its sdrhip_host_alloc gave)"""
        p = self.lib.sdrhip_host_alloc(self.ctx, a.nbytes)
        if not p:
            raise RuntimeError("sdrhip_host_alloc")
        C.memmove(p, a.ctypes.data, a.nbytes)
        return p

    def kernel_us(self, fn):
        """K_CONVERT's time in us and its launches while fn runs"""
        ms, n = C.c_double(0), C.c_uint(0)
        self.check(self.lib.sdrhip_ctx_synchronize(self.ctx))
        self.check(self.lib.sdrhip_ctx_kernel_timing(self.ctx, 1))
        self.check(self.lib.sdrhip_ctx_kernel_timing_read(self.ctx, K_CONVERT, C.byref(ms), C.byref(n)))
        fn()
        self.check(self.lib.sdrhip_ctx_kernel_timing_read(self.ctx, K_CONVERT, C.byref(ms), C.byref(n)))
        self.check(self.lib.sdrhip_ctx_kernel_timing(self.ctx, 0))
        return ms.value * 1e3, n.value


class Bank:
    """one Rx pipe in an egress order, fed the same batch again and again"""

    def __init__(self, library, cfg, order, src, counts, datagrams, max_released):
        self.L, self.lib = library, library.lib
        self.h = P()
        self.L.check(self.lib.sdrhip_rx_create(library.ctx, S, C.cast(C.byref(cfg), P), C.byref(self.h)))
        self.L.check(self.lib.sdrhip_rx_set_async(self.h, DEPTH, 1))
        self.L.check(self.lib.sdrhip_rx_set_egress(self.h, order))
        self.src, self.counts = P(src), (SZ * S)(*counts)
        self.submit_fn = self.lib.sdrhip_rx_submit_datagrams if datagrams else self.lib.sdrhip_rx_submit_ragged
        self.st = (C.c_uint32 * S)(*[7] * S)
        self.eg, self.nf, self.nr = Egress(), (SZ * S)(), (SZ * S)()
        self.maxr = max_released
        self.info = (C.c_uint8 * (16 * S * max(max_released, 1)))()
        self.submit_s = []

    def run(self, n):
        sub = col = 0
        while col < n:
            if sub < n:
                t0 = time.perf_counter()
                rc = self.submit_fn(self.h, self.src, self.counts, 0, self.st, self.st)
                t1 = time.perf_counter()
                if rc == 0:
                    self.submit_s.append(t1 - t0)
                    sub += 1
                    continue
                if rc != -6:
                    self.L.check(rc)
            self.L.check(self.lib.sdrhip_rx_collect_egress(self.h, C.byref(self.eg), self.nf, self.maxr, C.cast(self.info, P), self.nr, 1))
            col += 1

    def tags(self):
        """the tags of the batch that is lent"""
        n = int(self.eg.n_dgrams)
        return np.ctypeslib.as_array((C.c_uint16 * n).from_address(self.eg.stream_of)).copy()

    def array_digest(self):
        n = int(self.eg.n_dgrams) * 512
        return hashlib.sha256(C.string_at(self.eg.dgrams, n)).hexdigest()[:16]

    def release(self):
        self.L.check(self.lib.sdrhip_rx_release_egress(self.h))


def longest_run(tags):
    if not tags.shape[0]:
        return 0
    edges = np.flatnonzero(np.diff(tags.astype(np.int64)) != 0)
    bounds = np.concatenate([[-1], edges, [tags.shape[0] - 1]])
    return int(np.diff(bounds).max())


def most_in_window(tags, width):
    """the most datagrams of one stream among any `width` consecutive entries"""
    best = 0
    for s in np.unique(tags):
        c = np.concatenate([[0], np.cumsum(tags == s)])
        w = min(width, tags.shape[0])
        best = max(best, int((c[w:] - c[:-w]).max()))
    return best


def measure(name, banks, rounds, batches, expect_nf):
    for b in banks.values():  # steady state
        b.run(3)
    times = {k: [] for k in banks}
    for _ in range(rounds):
        for k, b in banks.items():
            t0 = time.perf_counter()
            b.run(batches)
            times[k].append((time.perf_counter() - t0) / batches)
            assert [int(x) for x in b.nf] == expect_nf, (name, k, list(b.nf))
    for b in banks.values():
        b.submit_s = []
    kern = {k: [] for k in banks}
    launches = {}
    for _ in range(rounds):
        for k, b in banks.items():
            us, n = b.L.kernel_us(lambda: b.run(batches))
            kern[k].append(us / batches)
            launches[k] = n / batches
    res = dict(shape=name,
               batch_ms_median={k: float(np.median(v)) * 1e3 for k, v in times.items()},
               batch_ms_rounds={k: [round(x * 1e3, 4) for x in v] for k, v in times.items()},
               kernel_us_median={k: float(np.median(v)) for k, v in kern.items()},
               kernel_us_rounds={k: [round(x, 3) for x in v] for k, v in kern.items()},
               kernel_launches_per_batch=launches,
               submit_host_us_median={k: float(np.median(b.submit_s)) * 1e6 for k, b in banks.items()},
               submit_host_us_min={k: float(np.min(b.submit_s)) * 1e6 for k, b in banks.items()},
               n_dgrams={k: int(b.eg.n_dgrams) for k, b in banks.items()},
               longest_run={k: longest_run(b.tags()) for k, b in banks.items()},
               most_in_64={k: most_in_window(b.tags(), 64) for k, b in banks.items()},
               array_sha256={k: b.array_digest() for k, b in banks.items()})
    res["kernel_us_paced_minus_rr"] = res["kernel_us_median"]["paced"] - res["kernel_us_median"]["rr"]
    res["kernel_us_rr_spread"] = max(kern["rr"]) - min(kern["rr"])
    for b in banks.values():
        b.release()
    return res


def report(fh, r, rounds, batches):
    fh.write("%s\n" % r["workload"])
    fh.write("1. batch period, ms (median of %d rounds of %d batches)\n" % (rounds, batches))
    for k, v in r["batch_ms_median"].items():
        fh.write("   %-10s %.4f   rounds: %s\n" % (k, v, " ".join("%.4f" % x for x in r["batch_ms_rounds"][k])))
    fh.write("2. delivery kernel, us per batch (kernel timers, class K_CONVERT%s; one figure per round of %d batches)\n"
             % (": the input unpack and the delivery" if max(r["kernel_launches_per_batch"].values()) > 1 else "", batches))
    for k, v in r["kernel_us_median"].items():
        fh.write("   %-10s %.2f   rounds: %s   (%.2f launches per batch)\n"
                 % (k, v, " ".join("%.2f" % x for x in r["kernel_us_rounds"][k]), r["kernel_launches_per_batch"][k]))
    fh.write("   paced - rr = %+.2f us; spread of rr's own rounds (max - min) = %.2f us\n" % (r["kernel_us_paced_minus_rr"], r["kernel_us_rr_spread"]))
    fh.write("3. host time of a submit call that found a free slot, us (median / min)\n")
    for k in r["submit_host_us_median"]:
        fh.write("   %-10s %.1f / %.1f\n" % (k, r["submit_host_us_median"][k], r["submit_host_us_min"][k]))
    fh.write("4. the array of the last batch (%s datagrams), from its tags\n" % "/".join(str(v) for v in sorted(set(r["n_dgrams"].values()))))
    for k in r["longest_run"]:
        fh.write("   %-10s longest run of one stream %5d   most of one stream among 64 consecutive entries %3d   array sha256 %s\n"
                 % (k, r["longest_run"][k], r["most_in_64"][k], r["array_sha256"][k]))
    fh.write("\n")


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

    if sd.device_count() <= 0:
        raise SystemExit("bench_rx_egress_paced: no GPU")
    here = Library(_lib.LIB_PATH)
    parent = Library(args.parent_lib) if args.parent_lib else None
    ctx = sd.Context(0)  # (the engine's own context: the configuration structs come from its pipes)
    B = 128 + R_OUT
    results = []

    def banks(cfg, src, counts, datagrams, max_released):
        out = {}
        if parent:
            out["rr_parent"] = Bank(parent, cfg, RR, parent.pinned(src), counts, datagrams, max_released)
        p = here.pinned(src)
        out["rr"] = Bank(here, cfg, RR, p, counts, datagrams, max_released)
        out["paced"] = Bank(here, cfg, PACED, p, counts, datagrams, max_released)
        return out

    # ---- equal counts: the datagram batches of tools/bench_rx_egress.py
    per = batch(Oracle(), np.random.RandomState(1))
    cfg = sd.RxPipe(ctx, S, log2decim=L, nb_fec=R_OUT).cfg
    r = measure("equal", banks(cfg, np.concatenate(per), [p.shape[0] for p in per], True, F + 1), args.rounds, args.batches, [1] * S)
    r["workload"] = ("equal: rx datagram batches, 64 streams x 16 frames x 136 datagrams (fecblk 32, 24 losses) -> decimate16_cen, nb_fec 32, "
                     "pinned packed input in place, depth %d; one frame per stream, %d datagrams delivered per batch" % (DEPTH, S * B))
    assert len(set(r["array_sha256"].values())) == 1, r["array_sha256"]  # (equal counts: one array under both orders)
    results.append(r)
    # ---- unequal counts: ragged sample batches, stream 0 four frames, the others one
    frames = [4] + [1] * (S - 1)
    L2 = 1
    counts = [f * SPF << L2 for f in frames]
    iq = np.random.RandomState(2).randint(-32768, 32768, size=(sum(counts), 2)).astype(np.int16)
    cfg2 = sd.RxPipe(ctx, S, log2decim=L2, fcpos=sd.FC_CEN, nb_fec=R_OUT).cfg
    r = measure("unequal", banks(cfg2, iq, counts, False, 0), args.rounds, args.batches, frames)
    r["workload"] = ("unequal: rx ragged sample batches, 64 streams -> decimate2_cen, nb_fec 32, pinned packed input in place, depth %d; "
                     "stream 0 completes 4 frames per batch, the other 63 one: %d datagrams delivered per batch" % (DEPTH, sum(frames) * B))
    results.append(r)
    line = json.dumps(dict(results=results))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("Paced departure order (KP, SDRHIP_EGRESS_PACED) against round robin (KR), and against round robin through the parent\n"
                     "commit's library: tools/bench_rx_egress_paced.py, alternating rounds, medians on the host clock.\n")
            fh.write("box: %s, %s, torch %s\n" % (torch.cuda.get_device_name(0), platform.platform(), torch.__version__))
            fh.write("date: %s\n" % datetime.datetime.now().strftime("%Y-%m-%d %H:%M"))
            with open(_lib.LIB_PATH, "rb") as f:
                fh.write("library: sha256 %s  %d bytes\n" % (hashlib.sha256(f.read()).hexdigest()[:16], os.path.getsize(_lib.LIB_PATH)))
            if args.parent_lib:
                with open(args.parent_lib, "rb") as f:
                    fh.write("parent library (rr_parent): sha256 %s\n" % hashlib.sha256(f.read()).hexdigest()[:16])
            fh.write("\n")
            for r in results:
                report(fh, r, args.rounds, args.batches)
            fh.write("%s\n" % line)


if __name__ == "__main__":
    main()
