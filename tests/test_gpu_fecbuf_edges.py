"""The five entries that take raw FEC datagrams, on sequences that put the hostile events of the classify rule at the classify
kernel's 1024-datagram chunk edges (tests/fecbuf_edges.py builds them, tests/test_fecbuf_edges_model.py proves the placement
and pins the yardsticks): a frame start at B - 1 / B / B + 1, the 128th arrival at B - 1 / B, a repeated original and a repeated
block 0 with one copy per chunk, block 0 in one chunk and the release in the next, a frame longer than two chunks, a chunk in
which every datagram opens a frame, A-B-A around B, calls of exactly 1024 / 1025 / 2048 datagrams; each behind a carry of 0, 37
and 133 datagrams.  All streams go together in one bank, the long one first, so that the packed entries see large offsets that
are no multiple of 1024 datagrams.

Until now the suite reached the chunk loop by chance only: the hostile sequences were fed in calls below 1024 datagrams, and the
calls above 1024 were benign.  test_gpu_tx_datagrams.test_bench_shape and test_gpu_rx_datagrams.test_realistic_shape stay as
they are: their fixed 136-datagram frames are the benchmark's shape, which is why their boundaries at 1024 and 2048 never moved
from ranks 72 and 8 of a frame.

The bank above has 14 streams, and the other datagram tests reach a bank of 1, 3 or 5 streams at some entries only: the
test_table_* cases at the end put banks of 1, 3 and 5 streams through all five entries on the smallest input that fills every column of the
drivers' per-call table (fecbuf_edges.table_calls), whose 64-bit arrays lie behind a padded run of ints.

Yardsticks: the reference's own SDRdaemonFECBuffer fed datagram by datagram (RefChain / HubChain) and the oracle's restatement
(test_gpu_fecbuf.Model); every released frame of every stream is compared, byte for byte."""
import numpy as np
import pytest

import fecbuf_edges as fe
import test_gpu_fecbuf as tg
import test_gpu_rx_datagrams as tr
import test_gpu_rx_datagrams_async as tra
import test_gpu_tx_datagrams as tt
import test_gpu_tx_datagrams_async as ta
from test_gpu_rx_datagrams import torch_first  # noqa: F401  (fixture: torch's runtime before the reference's library)

pytestmark = pytest.mark.gpu

ctx = tg.ctx        # (dec_strict = 1; "dec_rows_exceeded" must not grow)
reflib = tt.reflib
CL = fe.CL


check_events = fe.check_events


def reference_frames(oracle, reflib, carry):
    """per stream the payloads the reference class releases (the initial slot zero, as the library gives it)"""
    return [tt.RefChain(reflib, oracle).collect(list(seq)) for seq in fe.sequences(oracle, carry)]


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("carry", fe.CARRIES)
def test_bank(oracle, ctx, reflib, carry, device):
    """FECBufferBank.write_and_read: records, frames, block 0, statistics and both metas against the restatement, frames against
    the reference class; before the main call the same call without room: SDRHIP_EINVAL, the counts, nothing consumed"""
    import torch

    import sdrdaemon_amd as sd

    calls = fe.calls(oracle, carry)
    models, counts = fe.models(oracle, carry)
    S, main = len(models), len(calls) - 2
    bank = sd.FECBufferBank(ctx, S)
    got0, n0 = fe.run_bank(bank, calls[:main], device)
    arg = [torch.from_numpy(c).cuda() for c in calls[main]] if device else calls[main]
    assert max(counts[main]) > 1000
    with pytest.raises(sd.SdrHipError) as e:
        bank.write_and_read(arg, max_frames=1000)
    assert e.value.code == -1 and bank.last_n_frames == counts[main]
    got1, n1 = fe.run_bank(bank, calls[main:], device, max_frames=max(counts[main]))
    got = [tuple(a + b for a, b in zip(got0[s], got1[s])) for s in range(S)]
    assert n0 + n1 == counts
    tg.check_against_model(bank, got, models)
    ref = reference_frames(oracle, reflib, carry)
    for s in range(S):
        assert len(got[s][0]) == len(ref[s]), s
        for k in range(len(ref[s])):
            assert np.array_equal(got[s][0][k], ref[s][k]), (s, k, got[s][2][k])
    check_events(oracle, [g[2] for g in got], counts, bank.stats)


@pytest.fixture(scope="module")
def tx_expected(oracle, reflib):
    """per (log2interp, carry): per call, per stream the reference chain's samples, computed once for both Tx entries"""
    kept = {}

    def get(L, carry):
        if (L, carry) not in kept:
            chains = [tt.RefChain(reflib, oracle) for _ in fe.streams(oracle)]
            kept[(L, carry)] = [[ch.feed(c, L) for ch, c in zip(chains, chunk)] for chunk in fe.calls(oracle, carry)]
        return kept[(L, carry)]

    yield get
    kept.clear()


TX_CASES = [(0, 0), (0, 37), (0, 133), (4, 37)]


def check_samples(got, exp):
    for i, call in enumerate(exp):
        for s, e in enumerate(call):
            iq = got[i][s][0]
            assert iq.shape == e.shape, (i, s, iq.shape, e.shape)
            assert np.array_equal(iq, e), (i, s)


@pytest.mark.parametrize("L,carry", TX_CASES)
def test_tx_process_datagrams(oracle, ctx, reflib, tx_expected, L, carry):
    """TxPipe.process_datagrams against the reference chain; records and block 0 against a bank on the same calls"""
    import sdrdaemon_amd as sd

    calls = fe.calls(oracle, carry)
    _, counts = fe.models(oracle, carry)
    S = len(calls[0])
    tx, bank = sd.TxPipe(ctx, S, L), sd.FECBufferBank(ctx, S)
    got = tt.run_calls(tx, calls, bank=bank, max_frames=max(max(c) for c in counts))
    assert [[len(g[2]) for g in call] for call in got] == counts
    check_samples(got, tx_expected(L, carry))
    check_events(oracle, [sum((call[s][2] for call in got), []) for s in range(S)], counts, tx.collector_stats)


@pytest.mark.parametrize("L,carry", TX_CASES)
def test_tx_submit_collect_datagrams(oracle, ctx, reflib, tx_expected, L, carry):
    """TxPipe.submit_datagrams / collect_datagrams at depth 2: the same checks; the host's shadow never disagreed with the
    device, and the frame counts are the bank's read-back"""
    import sdrdaemon_amd as sd

    calls = fe.calls(oracle, carry)
    _, counts = fe.models(oracle, carry)
    S = len(calls[0])
    tx, bank = sd.TxPipe(ctx, S, L), sd.FECBufferBank(ctx, S)
    got = ta.run_async(tx, calls, 2)
    for i, chunk in enumerate(calls):
        ref = bank.write_and_read(chunk)
        assert [len(g[2]) for g in got[i]] == bank.last_n_frames == counts[i], i
        for s in range(S):
            assert got[i][s][2] == ref[s][2], (i, s)
            assert np.array_equal(got[i][s][1], ref[s][1]), (i, s)
    check_samples(got, tx_expected(L, carry))
    check_events(oracle, [sum((call[s][2] for call in got), []) for s in range(S)], counts, tx.collector_stats)
    assert ta.mismatches(ctx) == 0


RX = dict(L=2, fcpos=2, R=8)


@pytest.fixture(scope="module")
def rx_expected(oracle, reflib):
    """per carry: per call, per stream the hub chain's frames, and the remainders after every call; once for both Rx entries"""
    kept = {}

    def get(carry):
        if carry not in kept:
            calls = fe.calls(oracle, carry)
            S = len(calls[0])
            chains = [tr.HubChain(reflib, oracle) for _ in range(S)]
            frames, rems = [], []
            for i, chunk in enumerate(calls):
                sec, usec = tra.stamps(i, S)
                frames.append([chains[s].dgrams(chunk[s], RX["L"], RX["fcpos"], RX["R"], sec[s], usec[s]) for s in range(S)])
                rems.append([len(c.rem) for c in chains])
            kept[carry] = (frames, rems)
        return kept[carry]

    yield get
    kept.clear()


@pytest.mark.parametrize("carry", fe.CARRIES)
def test_rx_process_datagrams(oracle, ctx, reflib, rx_expected, carry):
    """RxPipe.process_datagrams at decimate4_cen, nb_fec 8, against the hub chain: frames, recovery blocks, carry(); records
    against a bank on the same calls"""
    import sdrdaemon_amd as sd

    calls = fe.calls(oracle, carry)
    _, counts = fe.models(oracle, carry)
    S = len(calls[0])
    exp, rems = rx_expected(carry)
    rx = sd.RxPipe(ctx, S, log2decim=RX["L"], fcpos=RX["fcpos"], nb_fec=RX["R"])
    bank = sd.FECBufferBank(ctx, S)
    recs = [[] for _ in range(S)]
    for i, chunk in enumerate(calls):
        sec, usec = tra.stamps(i, S)
        got = tr.run_call(rx, chunk, sec, usec, bank=bank, max_released=max(counts[i]))
        assert rx.last_n_released == counts[i], i
        for s in range(S):
            tr.check_frames(got[s][0], exp[i][s], (carry, i, s))
            recs[s] += got[s][1]
        assert list(rx.carry()) == rems[i], i
    assert sum(len(f) for call in exp for f in call) > 250
    check_events(oracle, recs, counts, rx.collector_stats)


@pytest.mark.parametrize("carry", fe.CARRIES)
def test_rx_submit_collect_datagrams(oracle, ctx, reflib, rx_expected, carry):
    """RxPipe.submit_datagrams / collect_datagrams at depth 2: the same checks, the carry after every submit, and the host's shadow
    never disagreed with the device"""
    import sdrdaemon_amd as sd

    calls = fe.calls(oracle, carry)
    _, counts = fe.models(oracle, carry)
    S = len(calls[0])
    exp, rems = rx_expected(carry)
    rx = sd.RxPipe(ctx, S, log2decim=RX["L"], fcpos=RX["fcpos"], nb_fec=RX["R"])

    def carry_is_the_chains(i):
        assert list(rx.carry()) == rems[i], i

    got = tra.run_async(rx, calls, 2, after_submit=carry_is_the_chains)
    bank = sd.FECBufferBank(ctx, S)
    recs = [[] for _ in range(S)]
    for i, chunk in enumerate(calls):
        ref = bank.write_and_read(chunk)
        assert [len(g[1]) for g in got[i]] == bank.last_n_frames == counts[i], i
        for s in range(S):
            assert got[i][s][1] == ref[s][2], (i, s)
            tr.check_frames(got[i][s][0], exp[i][s], (carry, i, s))
            recs[s] += got[i][s][1]
    check_events(oracle, recs, counts, rx.collector_stats)
    assert tra.mismatches(ctx) == 0


# ---- banks of 1, 3 and 5 streams: every column of the per-call table, whose offsets move with the bank size mod 4
@pytest.fixture(scope="module")
def table_expected(oracle, reflib):
    """per bank size: the calls, the frame counts per call, and per call, per stream the reference chains' results: the Tx
    chain's samples at TABLE_L, the hub chain's frames and remainders; computed once for the entries that share them"""
    kept = {}

    def get(S):
        if S not in kept:
            calls = fe.table_calls(oracle, S)
            _, counts = fe.models_of(oracle, calls)
            txc, hub = [tt.RefChain(reflib, oracle) for _ in range(S)], [tr.HubChain(reflib, oracle) for _ in range(S)]
            samples, frames, rems = [], [], []
            for i, chunk in enumerate(calls):
                sec, usec = tra.stamps(i, S)
                samples.append([txc[s].feed(chunk[s], TABLE_L) for s in range(S)])
                frames.append([hub[s].dgrams(chunk[s], TABLE_RX["L"], TABLE_RX["fcpos"], TABLE_RX["R"], sec[s], usec[s]) for s in range(S)])
                rems.append([len(c.rem) for c in hub])
            kept[S] = (calls, counts, samples, frames, rems)
        return kept[S]

    yield get
    kept.clear()


TABLE_L = 1                           # interpolate2
TABLE_RX = dict(L=1, fcpos=2, R=8)    # decimate2_cen: three frames of 16129 samples leave one behind in every row


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("S", fe.TABLE_SIZES)
def test_table_bank(oracle, ctx, reflib, table_expected, S, device):
    """FECBufferBank.write_and_read, device and host memory: as test_bank"""
    import sdrdaemon_amd as sd

    calls, counts = table_expected(S)[:2]
    models, _ = fe.models_of(oracle, calls)
    bank = sd.FECBufferBank(ctx, S)
    got, n = fe.run_bank(bank, calls, device)
    assert n == counts
    tg.check_against_model(bank, got, models)
    for s in range(S):
        ref = tt.RefChain(reflib, oracle).collect(list(np.concatenate([c[s] for c in calls])))
        assert len(got[s][0]) == len(ref), s
        for k in range(len(ref)):
            assert np.array_equal(got[s][0][k], ref[k]), (s, k, got[s][2][k])
    fe.check_table_events([g[2] for g in got], counts)


@pytest.mark.parametrize("S", fe.TABLE_SIZES)
def test_table_tx_process_datagrams(oracle, ctx, table_expected, S):
    """TxPipe.process_datagrams: as test_tx_process_datagrams"""
    import sdrdaemon_amd as sd

    calls, counts, samples = table_expected(S)[:3]
    tx, bank = sd.TxPipe(ctx, S, TABLE_L), sd.FECBufferBank(ctx, S)
    got = tt.run_calls(tx, calls, bank=bank)
    assert [[len(g[2]) for g in call] for call in got] == counts
    check_samples(got, samples)
    fe.check_table_events([sum((call[s][2] for call in got), []) for s in range(S)], counts)


@pytest.mark.parametrize("S", fe.TABLE_SIZES)
def test_table_tx_submit_collect_datagrams(oracle, ctx, table_expected, S):
    """TxPipe.submit_datagrams / collect_datagrams at depth 2: as test_tx_submit_collect_datagrams"""
    import sdrdaemon_amd as sd

    calls, counts, samples = table_expected(S)[:3]
    tx = sd.TxPipe(ctx, S, TABLE_L)
    got = ta.run_async(tx, calls, 2)
    assert [[len(g[2]) for g in call] for call in got] == counts
    ta.check_bank(ctx, got, calls)
    check_samples(got, samples)
    fe.check_table_events([sum((call[s][2] for call in got), []) for s in range(S)], counts)
    assert ta.mismatches(ctx) == 0


@pytest.mark.parametrize("S", fe.TABLE_SIZES)
def test_table_rx_process_datagrams(oracle, ctx, table_expected, S):
    """RxPipe.process_datagrams: as test_rx_process_datagrams"""
    import sdrdaemon_amd as sd

    calls, counts, _, exp, rems = table_expected(S)
    rx = sd.RxPipe(ctx, S, log2decim=TABLE_RX["L"], fcpos=TABLE_RX["fcpos"], nb_fec=TABLE_RX["R"])
    bank = sd.FECBufferBank(ctx, S)
    recs = [[] for _ in range(S)]
    for i, chunk in enumerate(calls):
        sec, usec = tra.stamps(i, S)
        got = tr.run_call(rx, chunk, sec, usec, bank=bank)
        assert rx.last_n_released == counts[i], i
        for s in range(S):
            tr.check_frames(got[s][0], exp[i][s], (S, i, s))
            recs[s] += got[s][1]
        assert list(rx.carry()) == rems[i], i
    assert sum(len(f) for call in exp for f in call) == S and rems[-1] == [1] * S
    fe.check_table_events(recs, counts)


@pytest.mark.parametrize("S", fe.TABLE_SIZES)
def test_table_rx_submit_collect_datagrams(oracle, ctx, table_expected, S):
    """RxPipe.submit_datagrams / collect_datagrams at depth 2: as test_rx_submit_collect_datagrams"""
    import sdrdaemon_amd as sd

    calls, counts, _, exp, rems = table_expected(S)
    rx = sd.RxPipe(ctx, S, log2decim=TABLE_RX["L"], fcpos=TABLE_RX["fcpos"], nb_fec=TABLE_RX["R"])

    def carry_is_the_chains(i):
        assert list(rx.carry()) == rems[i], i

    got = tra.run_async(rx, calls, 2, after_submit=carry_is_the_chains)
    bank = sd.FECBufferBank(ctx, S)
    recs = [[] for _ in range(S)]
    for i, chunk in enumerate(calls):
        ref = bank.write_and_read(chunk)
        assert [len(g[1]) for g in got[i]] == bank.last_n_frames == counts[i], i
        for s in range(S):
            assert got[i][s][1] == ref[s][2], (i, s)
            tr.check_frames(got[i][s][0], exp[i][s], (S, i, s))
            recs[s] += got[i][s][1]
    fe.check_table_events(recs, counts)
    assert tra.mismatches(ctx) == 0
