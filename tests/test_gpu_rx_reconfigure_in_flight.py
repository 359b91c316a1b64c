"""sdrhip_rx_reconfigure between the submit and the collect of an asynchronous Rx batch: "batches in flight keep the configuration
(and frame size) they were submitted with" (include/sdrhip.h), so RxPipe.collect / collect_ragged must shape what they deliver
with the nb_fec of the batch, not with the pipe's nb_fec at the collect.

Two streams, no decimation, blocks of 16129 + 64 samples: every block completes exactly one frame per stream and leaves one open
(ragged: the second stream gets 16129 + 32).  Block 1 goes in under R_before, the pipe is reconfigured to R_after, block 2 goes in,
then both batches are collected.  Expected: what a twin pipe delivers for the same samples through the synchronous call with the
same reconfigure between its two calls, byte for byte -- batch 1 in frames of 128 + R_before blocks, batch 2 of 128 + R_after.

Before the batch log kept each batch's nb_fec, the pipe shaped both collects with R_after, and batch 1 came back mis-shaped in
all four cases: (4, 8) as (1, 136, 512) cut out of a frame of 132 blocks, (8, 4) as (1, 132, 512) cut out of one of 136 (the
buffer has room for 3 frames per stream here, so the library's "frame stride too small" did not trigger)."""
import numpy as np
import pytest

import sdrdaemon_amd as sd

pytestmark = pytest.mark.gpu

F = 16129
S = 2
N = F + 64
COUNTS = [F + 64, F + 32]


@pytest.mark.parametrize("entry", ["uniform", "ragged"])
@pytest.mark.parametrize("r_before,r_after", [(4, 8), (8, 4)])
def test_a_batch_in_flight_keeps_its_frame_size(r_before, r_after, entry):
    assert sd.device_count() > 0
    ctx = sd.Context(0)
    rs = np.random.RandomState(100 * r_before + r_after)
    blocks = [rs.randint(-32768, 32768, size=(S, N, 2)).astype(np.int16) for _ in range(2)]
    a = sd.RxPipe(ctx, S, log2decim=0, fcpos=sd.FC_CEN, nb_fec=r_before)
    b = sd.RxPipe(ctx, S, log2decim=0, fcpos=sd.FC_CEN, nb_fec=r_before)
    a.set_async(depth=2, blocks=1)
    exp = []
    for i, x in enumerate(blocks):
        if i == 1:
            a.reconfigure(nb_fec=r_after)
            b.reconfigure(nb_fec=r_after)
        if entry == "uniform":
            a.submit(x, 7 + i, 9)
            exp.append(list(b.process(x, 7 + i, 9)))
        else:
            a.submit_ragged(x, COUNTS, 7 + i, 9)
            frames, n = b.process_ragged(x, COUNTS, 7 + i, 9)
            exp.append([frames[s, :n[s]] for s in range(S)])
    for i, r in enumerate((r_before, r_after)):
        got = a.collect() if entry == "uniform" else a.collect_ragged()
        assert got is not None, i
        for s in range(S):
            assert exp[i][s].shape == (1, 128 + r, 512), (i, s, exp[i][s].shape)
            assert got[s].shape == (1, 128 + r, 512), (i, s, got[s].shape)
            assert np.array_equal(got[s], exp[i][s]), (i, s)
    assert (a.collect(wait=False) if entry == "uniform" else a.collect_ragged(wait=False)) is None
