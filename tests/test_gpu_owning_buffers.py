"""Who owns what in the host layer, on a live GPU.

A pipe keeps its own context alive: an RxPipe / a TxPipe that is the ONLY handle on its context goes on working after
sdrhip_ctx_destroy on that context, gives what a twin pipe on a living context gives, and frees the context when it is closed.

Create / use / destroy on the paths test_gpu_errors.test_create_use_destroy_cycles_do_not_leak never touches -- the ragged step
with per-stream formats, the stream-meta table, ragged batches whose arena grows, the datagram entries (rows that grow, batches,
egress), a re-pitch, a pipelined pipe whose area grows while frames wait, reset / export / import of a stream, the Tx pipe's
pipelined, datagram and batch entries -- with that test's warm-up and limits."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPF = 16129  # samples per frame
L = 2        # the twins' and the cycle's log2decim / log2interp


def samples(n, seed, dtype=np.int16):
    rs = np.random.RandomState(seed)
    if dtype == np.uint8:
        return rs.randint(0, 256, (n, 2)).astype(np.uint8)
    return rs.randint(-20000, 20000, (n, 2)).astype(np.int16)


@pytest.fixture(scope="module")
def frames():
    """6 frames per stream of a 2-stream sender (128 + 8 super blocks each): their blocks are the datagrams the datagram entries take"""
    import sdrdaemon_amd as sd

    c = sd.Context(0)
    rx = sd.RxPipe(c, 2, log2decim=0, nb_fec=8)
    fr = rx.process(np.stack([samples(6 * SPF, 1), samples(6 * SPF, 2)]), 10, 20)
    rx.close()
    c.close()
    assert fr.shape == (2, 6, 136, 512)
    fr = np.ascontiguousarray(fr)
    fr.setflags(write=False)
    return fr


def dgrams(frames, lo, hi):
    return [np.ascontiguousarray(frames[s, lo:hi]).reshape(-1, 512) for s in range(2)]


def destroy_context_first(ctx):
    ctx.lib.sdrhip_ctx_destroy(ctx.h)
    ctx.h = C.c_void_p()


def twins(make):
    import sdrdaemon_amd as sd

    ca, cb = sd.Context(0), sd.Context(0)
    return ca, cb, make(ca), make(cb)


def same_datagram_result(a, b):
    assert len(a) == len(b) == 2
    for (fa, ra), (fb, rb) in zip(a, b):
        assert np.array_equal(fa, fb) and ra == rb


def test_rx_pipe_alone_keeps_its_context_alive():
    import sdrdaemon_amd as sd

    ca, cb, a, b = twins(lambda c: sd.RxPipe(c, 2, log2decim=L, nb_fec=8))
    x = np.stack([samples(2 * (SPF + 700) << L, 3), samples(2 * (SPF + 700) << L, 4)])
    half = x.shape[1] // 2
    assert np.array_equal(a.process(x[:, :half], 1, 2), b.process(x[:, :half], 1, 2))
    destroy_context_first(ca)
    ra, rb = a.process(x[:, half:], 3, 4), b.process(x[:, half:], 3, 4)
    assert ra.shape == (2, 1, 136, 512) and np.array_equal(ra, rb)
    a.close()  # (the last reference: frees the context)
    b.close()
    cb.close()


def test_rx_pipe_with_a_collector_keeps_its_context_alive(frames):
    import sdrdaemon_amd as sd

    ca, cb, a, b = twins(lambda c: sd.RxPipe(c, 2, log2decim=L, nb_fec=8))
    first, second = dgrams(frames, 0, 2), dgrams(frames, 2, 6)
    same_datagram_result(a.process_datagrams(first, 5, 6, max_released=8), b.process_datagrams(first, 5, 6, max_released=8))
    destroy_context_first(ca)
    ra, rb = a.process_datagrams(second, 7, 8, max_released=8), b.process_datagrams(second, 7, 8, max_released=8)
    # (5 of the 6 incoming frames are released by now: 5 * 16129 / 4 samples, one outgoing frame)
    assert a.last_n_released == b.last_n_released and sum(a.last_n_released) >= 2 and ra[0][0].shape[0] == ra[1][0].shape[0] == 1
    same_datagram_result(ra, rb)
    assert list(a.carry()) == list(b.carry())
    a.close()
    b.close()
    cb.close()


def test_tx_pipe_alone_keeps_its_context_alive(frames):
    import sdrdaemon_amd as sd

    ca, cb, a, b = twins(lambda c: sd.TxPipe(c, 2, L))
    rx = np.ascontiguousarray(frames[:, :, :128])
    assert np.array_equal(a.process(rx[:, :1]), b.process(rx[:, :1]))
    destroy_context_first(ca)
    ra, rb = a.process(rx[:, 1:2]), b.process(rx[:, 1:2])
    assert ra.shape == (2, SPF << L, 2) and np.array_equal(ra, rb) and ra.any()
    a.close()
    b.close()
    cb.close()


CYCLES = 120


def test_create_use_destroy_cycles_on_the_other_paths_do_not_leak(frames):
    """test_create_use_destroy_cycles_do_not_leak's measurement (8 warm-up cycles, device memory < 64 MiB, ru_maxrss < 96 MiB) over
    a cycle that reaches the buffers its cycle never allocates; 2 streams, the smallest shapes that reach each of them"""
    import gc
    import resource

    import torch

    import sdrdaemon_amd as sd

    x = np.stack([samples(6 * (SPF + 300) << L, 5), samples(6 * (SPF + 300) << L, 6)])
    one, five = (SPF + 300) << L, 5 * (SPF + 300) << L
    x8 = samples(one, 7, np.uint8)
    rx128 = np.ascontiguousarray(frames[:, :2, :128])

    def cycle():
        c = sd.Context(0)
        made = []

        def rx_pipe(**kw):
            made.append(sd.RxPipe(c, 2, log2decim=L, nb_fec=8, **kw))
            return made[-1]

        def tx_pipe(**kw):
            made.append(sd.TxPipe(c, 2, L, **kw))
            return made[-1]

        # the uniform step: the stream-meta table set twice (sm_tab), a fecblk change between calls (re-pitch), a partial reset,
        # export / import (x_blob, x_pin)
        u = rx_pipe()
        u.set_stream_meta([435000, 436000], [625000, 312500])
        n = u.process(x[:, :one], 1, 2).shape[1]
        u.set_stream_meta([437000, 438000], None)
        n += u.process(x[:, one:2 * one], 3, 4).shape[1]
        u.reconfigure(nb_fec=16)
        n += u.process(x[:, 2 * one:3 * one], 5, 6).shape[1]
        assert n == 3
        u.reset_streams([1])
        u.import_stream(1, u.export_stream(0))
        # a synchronous ragged call with per-stream formats (f_*)
        f = rx_pipe()
        f.set_stream_formats(["s16", "u8"])
        _, nf = f.process_ragged([x[0, :one], x8], None, 1, 2)
        assert list(nf) == [1, 1]
        # ragged batches whose second block is longer than the first: the arena grows (ring, a_*)
        r = rx_pipe()
        r.set_async(4, 2)
        r.submit_ragged(x[:, :1000], [1000, 900])
        r.submit_ragged(x[:, 1000:five], [five - 1000, five - 2000])
        assert [g.shape[0] for g in r.collect_ragged()] == [5, 5]
        # the datagram entries: a call, a larger one (j_rows grows), a batch (d_tabs, d_seg), an egress batch (e_tab)
        d = rx_pipe()
        d.process_datagrams(dgrams(frames, 0, 2), 1, 2, max_released=2)
        d.process_datagrams(dgrams(frames, 2, 4), 3, 4, max_released=6)
        d.submit_datagrams(dgrams(frames, 4, 5), 5, 6)
        assert d.collect_datagrams() is not None and sum(d.last_n_released) >= 2
        d.set_egress("round_robin")
        d.submit_datagrams(dgrams(frames, 5, 6), 7, 8)
        assert d.collect_egress() is not None and sum(d.last_n_released) >= 2
        # a pipelined pipe whose area grows while frames wait (old_work)
        p = rx_pipe(pipelined=True)
        assert p.process(x[:, :one], 1, 2).shape[1] == 0
        assert p.process(x[:, one:], 3, 4).shape[1] == 1
        assert p.flush().shape[1] == 5
        # Tx: a pipelined call, a datagram call, a datagram batch
        t = tx_pipe(pipelined=True)
        assert t.process(rx128).shape[1] == 0
        assert t.flush().shape[1] == 2 * SPF << L
        g = tx_pipe()
        assert g.process_datagrams(dgrams(frames, 0, 2), max_frames=8)[0][0].shape[0] >= SPF << L
        g.submit_datagrams(dgrams(frames, 2, 4))
        assert g.collect_datagrams()[1][0].shape[0] >= SPF << L
        c.synchronize()
        for obj in made:
            obj.close()
        c.close()

    for _ in range(8):
        cycle()
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    for _ in range(CYCLES):
        cycle()
    gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    assert free0 - free1 < 64 << 20, "device memory leaked: %.1f MiB over %d cycles" % ((free0 - free1) / 2**20, CYCLES)
    assert rss1 - rss0 < 96 << 10, "host memory grew by %.1f MiB over %d cycles (ru_maxrss)" % ((rss1 - rss0) / 1024, CYCLES)
