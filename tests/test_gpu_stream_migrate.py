"""Export and import of one stream (sdrhip_*_export_stream / _import_stream): a live stream moves from one bank to another --
another context, another nstreams, another fecblk -- and continues exactly where it stood; both banks' other streams run on.

The expected output is the UNINTERRUPTED reference chain of the stream (test_gpu_rx_datagrams.HubChain: the reference's
SDRdaemonFECBuffer, the compiled-reference decimators, the oracle framer and encoder; test_gpu_tx_datagrams.RefChain for Tx), which
never hears of the move; from the first frame completed in the destination it is encoded with the destination's fecblk (the open
frame keeps the meta block it was opened with).  Everything is byte-exact.

Shapes: decimate4 / interpolate4, 10 incoming frames per stream; the move happens 60 datagrams into incoming frame 2: an open
collector slot, 3 samples held back, an open outgoing frame."""
import numpy as np
import pytest

import test_gpu_rx_datagrams as tr
import test_gpu_stream_reset as ts
import test_gpu_tx_datagrams as tt

pytestmark = pytest.mark.gpu

ctx = tt.ctx  # (dec_strict = 1: the reference's copy-back holes)
reflib = tt.reflib
torch_first = ts.torch_first
L, FC = 2, 2
CUTS = [(2, 60), (3, 20)]


def second_context():
    import sdrdaemon_amd as sd

    c = sd.Context(0)
    c.set_option("dec_strict", 1)
    return c


def rx_calls(oracle, seed, S):
    return ts.dgram_calls(ts.follow_streams(oracle, seed, S, 10), CUTS)


def run_rx(rx, chains, chunk, R, sec, where, device=True):
    """one process_datagrams call against the chains (R: per chain, the fecblk its frames get from now on)"""
    got = tr.run_call(rx, chunk, sec, 5, device=device)
    for s, c in enumerate(chains):
        tr.check_frames(got[s][0], c.dgrams(chunk[s], L, FC, R[s], sec, 5), (where, s))
    assert list(rx.carry()) == [len(c.rem) for c in chains], where
    return sum(g[0].shape[0] for g in got)


def test_rx_stream_moves_to_another_bank(oracle, ctx, reflib):
    import sdrdaemon_amd as sd

    RA, RB = 8, 32
    ca, cb = rx_calls(oracle, 90, 3), rx_calls(oracle, 91, 2)
    A = sd.RxPipe(ctx, 3, log2decim=L, nb_fec=RA)
    ctx_b = second_context()
    B = sd.RxPipe(ctx_b, 2, log2decim=L, nb_fec=RB)
    chA = [tr.HubChain(reflib, oracle) for _ in range(3)]
    chB = [tr.HubChain(reflib, oracle) for _ in range(2)]
    run_rx(A, chA, ca[0], [RA] * 3, 300, "A0")
    run_rx(B, chB, cb[0], [RB] * 2, 400, "B0")
    assert chA[1].rem.shape[0] == 3 and chA[1].fr.s.sample_index + chA[1].fr.s.tx_block_index > 0  # (a carry, an open frame)
    blob = A.export_stream(1)
    assert len(blob) == ctx.lib.sdrhip_rx_stream_state_bytes(A.h) == ctx_b.lib.sdrhip_rx_stream_state_bytes(B.h)
    assert blob[:4] == b"SDRS" and int.from_bytes(blob[4:8], "little") == 1 and int.from_bytes(blob[12:16], "little") == len(blob)
    B.import_stream(0, blob)
    # B's stream 0 is A's stream 1 from here on: a second, uninterrupted chain of that stream, encoded with B's fecblk from now on
    moved = tr.HubChain(reflib, oracle)
    assert moved.dgrams(ca[0][1], L, FC, RA, 300, 5) == []
    chB[0] = moved
    total = 0
    for i in (1, 2):
        run_rx(A, chA, ca[i], [RA] * 3, 300 + i, ("A", i), device=i == 1)  # (all of A undisturbed, the exported stream included)
        total += run_rx(B, chB, [ca[i][1], cb[i][1]], [RB] * 2, 300 + i, ("B", i), device=i == 2)
    assert total >= 3
    for s, c in enumerate(chB):
        st = B.collector_stats(s)
        assert st["cur_nb_blocks"] > 0, s


def test_rx_round_trip_inside_one_bank(oracle, ctx, reflib):
    """export, feed the stream other data, import, continue: as if the other data had never been fed"""
    import sdrdaemon_amd as sd

    R = 8
    calls, other = rx_calls(oracle, 92, 3), rx_calls(oracle, 93, 1)
    rx = sd.RxPipe(ctx, 3, log2decim=L, nb_fec=R)
    chains = [tr.HubChain(reflib, oracle) for _ in range(3)]
    run_rx(rx, chains, calls[0], [R] * 3, 500, 0)
    blob = rx.export_stream(1)
    got = tr.run_call(rx, [ts.EMPTY, np.concatenate([other[0][0], other[1][0]]), ts.EMPTY], 777, 1)
    assert got[1][0].shape[0] >= 1 and got[0][0].shape[0] == got[2][0].shape[0] == 0
    rx.import_stream(1, blob)
    total = sum(run_rx(rx, chains, calls[i], [R] * 3, 500 + i, i, device=i == 1) for i in (1, 2))
    assert total >= 6


def test_tx_stream_moves_to_another_bank(oracle, ctx, reflib):
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(94)
    per = [tt.stream_dgrams(oracle, rs, 4, 32) for _ in range(5)]
    cut = [[np.asarray(p[:200], np.uint8).reshape(-1, 512), np.asarray(p[200:420], np.uint8).reshape(-1, 512),
            np.asarray(p[420:], np.uint8).reshape(-1, 512)] for p in per]
    ctx_b = second_context()
    A, B = sd.TxPipe(ctx, 3, L), sd.TxPipe(ctx_b, 2, L)
    chA = [tt.RefChain(reflib, oracle) for _ in range(3)]
    chB = [tt.RefChain(reflib, oracle) for _ in range(2)]

    def run(tx, chains, chunk, where):
        got, = tt.run_calls(tx, [chunk])
        for s, c in enumerate(chains):
            exp = c.feed(chunk[s], L)
            assert got[s][0].shape == exp.shape and np.array_equal(got[s][0], exp), (where, s)
        return sum(g[0].shape[0] for g in got)

    run(A, chA, [cut[s][0] for s in range(3)], "A0")
    run(B, chB, [cut[3][0], cut[4][0]], "B0")
    blob = A.export_stream(1)
    assert len(blob) == ctx.lib.sdrhip_tx_stream_state_bytes(A.h) and blob[:4] == b"SDRS" and int.from_bytes(blob[8:12], "little") == 2
    B.import_stream(0, blob)
    moved = tt.RefChain(reflib, oracle)
    moved.feed(cut[1][0], L)
    chB[0] = moved
    n = 0
    for i in (1, 2):
        run(A, chA, [cut[s][i] for s in range(3)], ("A", i))
        n += run(B, chB, [cut[1][i], cut[4][i]], ("B", i))
    assert n >= 4 * (16129 << L)
    # a round trip inside bank A: other data into stream 2, then back
    blob = A.export_stream(2)
    tt.run_calls(A, [[ts.EMPTY, ts.EMPTY, cut[3][1]]])
    A.import_stream(2, blob)
    tail = np.full((1, 512), 0xAB, np.uint8)  # (another frame index: releases what every stream holds)
    run(A, chA, [tail] * 3, "A tail")


def test_refusals_leave_the_state_unchanged(oracle, ctx, reflib):
    """a blob of the other hb_variant, a truncated blob, a flipped magic, a batch in flight: SDRHIP_EINVAL each; the calls that
    follow continue the uninterrupted chains"""
    import sdrdaemon_amd as sd

    R = 8
    calls = rx_calls(oracle, 95, 2)
    rx = sd.RxPipe(ctx, 2, log2decim=L, nb_fec=R)
    db = sd.RxPipe(ctx, 2, log2decim=L, nb_fec=R, hb_variant=sd.HB_DB)
    chains = [tr.HubChain(reflib, oracle) for _ in range(2)]
    run_rx(rx, chains, calls[0], [R] * 2, 600, 0)
    blob = rx.export_stream(0)
    other = bytes(len(blob))

    def refused(fn, *a):
        with pytest.raises(sd.SdrHipError) as e:
            fn(*a)
        assert e.value.code == -1, e.value

    refused(db.import_stream, 0, blob)
    refused(rx.import_stream, 1, blob[:-16])
    refused(rx.import_stream, 1, bytes([blob[0] ^ 0x40]) + blob[1:])
    refused(rx.import_stream, 1, blob[:4] + (2).to_bytes(4, "little") + blob[8:])  # (version)
    refused(rx.import_stream, 1, blob[:8] + (2).to_bytes(4, "little") + blob[12:])  # (a Tx blob's kind)
    refused(rx.import_stream, 2, blob)
    refused(rx.import_stream, 1, other)
    refused(rx.export_stream, -1)
    tx = sd.TxPipe(ctx, 2, L)
    refused(tx.import_stream, 0, blob)
    rx.submit_datagrams(calls[1], 601, 5)
    refused(rx.import_stream, 1, blob)
    refused(rx.export_stream, 0)
    got = rx.collect_datagrams()
    for s, c in enumerate(chains):
        tr.check_frames(got[s][0], c.dgrams(calls[1][s], L, FC, R, 601, 5), ("batch", s))
    assert run_rx(rx, chains, calls[2], [R] * 2, 602, 2) >= 2
    # the DB bank took nothing: it still behaves as a fresh one
    dchains = [tr.HubChain(reflib, oracle, 1) for _ in range(2)]
    assert sum(g[0].shape[0] for g in tr.run_call(db, calls[0], 1, 1)) == 0
    for s, c in enumerate(dchains):
        assert c.dgrams(calls[0][s], L, FC, R, 1, 1) == []
    got = tr.run_call(db, calls[1], 2, 1)
    for s, c in enumerate(dchains):
        tr.check_frames(got[s][0], c.dgrams(calls[1][s], L, FC, R, 2, 1), ("db", s))
