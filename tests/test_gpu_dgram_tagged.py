"""Tagged datagram batches (sdrhip_fecbuf_write_and_read_tagged, sdrhip_tx_submit_datagrams_tagged,
sdrhip_rx_submit_datagrams_tagged): one arrival-order array with a stream tag per datagram, demultiplexed on the device (KX).  A
tagged call means the untagged call on the per-stream subsequences, byte for byte.  The bank is tied to test_gpu_fecbuf's reference
SDRdaemonFECBuffer directly, fed every stream's subsequence datagram by datagram; the pipes to their untagged entries on a twin
handle, which the existing tests tie to the reference chains.  Every test checks that the host's shadow of the classification never
disagreed with the device ("fecbuf_shadow_mismatch" stays 0)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_fecbuf as tg
import test_gpu_rx_datagrams as tr
import test_gpu_tx_datagrams as tt
from test_gpu_rx_datagrams import torch_first  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F = 16129
EBUSY, EINVAL = -6, -1
SKIP = 0xFFFF
EMPTY = np.zeros((0, 512), np.uint8)


@pytest.fixture
def ctx():
    import sdrdaemon_amd as sd

    assert sd.device_count() > 0
    c = sd.Context(0)
    c.set_option("dec_strict", 1)  # (the reference's copy-back holes)
    yield c
    assert c.counter("fecbuf_shadow_mismatch") == 0


def mismatches(ctx):
    return ctx.counter("fecbuf_shadow_mismatch")


def interleave(chunk, tags, seed=0):
    """the arrival array of a tag sequence: position i takes the next datagram of stream tags[i], random bytes for SDRHIP_DGRAM_SKIP"""
    rs = np.random.RandomState(1000 + seed)
    tags = np.asarray(tags, np.uint16)
    arr = np.empty((len(tags), 512), np.uint8)
    for s, c in enumerate(chunk):
        at = np.flatnonzero(tags == s)
        assert len(at) == len(c), (s, len(at), len(c))
        if len(c):
            arr[at] = np.asarray(c, np.uint8).reshape(-1, 512)
    junk = np.flatnonzero(tags == SKIP)
    arr[junk] = rs.randint(0, 256, (len(junk), 512)).astype(np.uint8)
    return arr, tags


def merge(chunk, seed, skip=0):
    """one arrival array + tags from a per-stream list: a seeded random merge that keeps each stream's order, with `skip` junk
    datagrams (random bytes) inserted, tagged SDRHIP_DGRAM_SKIP"""
    tags = np.concatenate([np.full(len(c), s, np.uint16) for s, c in enumerate(chunk)] + [np.full(skip, SKIP, np.uint16)])
    np.random.RandomState(seed).shuffle(tags)
    return interleave(chunk, tags, seed)


def cut(arr, tags, S, at):
    """the arrival array cut at position `at`: two (array, tags, per-stream subsequences)"""
    out = []
    for a, t in ((arr[:at], tags[:at]), (arr[at:], tags[at:])):
        out.append((a, t, [a[t == s] for s in range(S)]))
    return out


def lossy_stream(oracle, rs, n, fi0):
    """n datagrams of one stream: frames of fecblk 4 with two originals lost (130 datagrams each), the last one cut short"""
    dg = []
    for fr in tg.make_frames(oracle, rs, n // 130 + 1, 4, fi0):
        lost = set(rs.choice(np.arange(1, 128), 2, replace=False).tolist())
        dg += [fr[i] for i in range(132) if i not in lost]
    return np.asarray(dg[:n], np.uint8).reshape(-1, 512)


# ------------------------------------------------------------------------------------------------ 1. the bank
_BANK = {}


def bank_case(oracle):
    """3 streams with 133, 0 and 267 datagrams (kept: every order and memory shares it)"""
    if "per" not in _BANK:
        rs = np.random.RandomState(11)
        _BANK["per"] = [lossy_stream(oracle, rs, 133, 65534), EMPTY, lossy_stream(oracle, rs, 267, 7)]
    return _BANK["per"]


def bank_order(per, order):
    n = [len(p) for p in per]
    if order == "random":
        return per, merge(per, 3, skip=1)
    if order == "one":  # every datagram tagged to one stream: it collects the concatenation
        per = [EMPTY, np.concatenate([per[0], per[2]]), EMPTY]
        return per, interleave(per, [1] * 200 + [SKIP] + [1] * 200)
    if order == "round_robin":  # strictly alternating while both streams last
        tags = [0, 2] * n[0] + [SKIP] + [2] * (n[2] - n[0])
        return per, interleave(per, tags)
    assert order == "bursts"  # whole streams one after the other
    return per, interleave(per, [2] * n[2] + [SKIP] + [0] * n[0])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("order", ["random", "one", "round_robin", "bursts"])
def test_bank_against_the_reference_collector(oracle, ctx, order, device):
    """n_total = 400 + 1 skipped = 401 (odd), one stream empty, cut into two calls in the middle of a frame: payloads, block 0,
    records and the statistics equal one reference collector per stream fed its subsequence datagram by datagram"""
    import sdrdaemon_amd as sd
    import torch

    per, (arr, tags) = bank_order(bank_case(oracle), order)
    assert arr.shape[0] == 401 and int((tags == SKIP).sum()) == 1
    models = [tg.Model(oracle).run(list(p)) for p in per]
    bank = sd.FECBufferBank(ctx, 3)
    got = [([], [], []) for _ in range(3)]
    pieces = cut(arr, tags, 3, 190)
    assert any(len(x) % 130 for x in pieces[0][2])  # (a frame of 130 datagrams begins in the first call and ends in the second)
    for a, t, _ in pieces:
        out = bank.write_and_read_tagged(torch.from_numpy(a).cuda() if device else a, t)
        for s in range(3):
            got[s][0].extend(list(tt.as_np(out[s][0])))
            got[s][1].extend(list(tt.as_np(out[s][1])))
            got[s][2].extend(out[s][2])
    assert sum(len(g[2]) for g in got) >= 4  # (initial slots and whole frames were released)
    assert any(r["flags"] & sd.engine.FECBUF_REPAIRED for g in got for r in g[2])
    tg.check_against_model(bank, got, models)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 2. chunk and grid edges
_EDGE = {}


@pytest.mark.parametrize("n_total", [1, 2, 3, 255, 256, 257, 511, 513, 1025])
def test_chunk_and_grid_edges(oracle, ctx, n_total):
    """a tagged bank call against an untagged one on a twin bank at the sizes where KX's half-waves, workgroups and the classify
    pass's chunks end"""
    import sdrdaemon_amd as sd

    if "pool" not in _EDGE:
        rs = np.random.RandomState(12)
        _EDGE["pool"] = [lossy_stream(oracle, rs, 700, 100), lossy_stream(oracle, rs, 700, 9000)]
    n0 = n_total // 3
    per = [_EDGE["pool"][0][:n0], _EDGE["pool"][1][:n_total - n0]]
    arr, tags = merge(per, n_total)
    assert arr.shape[0] == n_total
    a, b = sd.FECBufferBank(ctx, 2), sd.FECBufferBank(ctx, 2)
    got, exp = a.write_and_read_tagged(arr, tags), b.write_and_read(per)
    for s in range(2):
        assert got[s][2] == exp[s][2], s
        assert np.array_equal(got[s][0], exp[s][0]) and np.array_equal(got[s][1], exp[s][1]), s
        assert a.stats(s) == b.stats(s), s
    assert len(got[1][2]) == 1 + (n_total - n0 - 1) // 130
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 3. the Rx hub
def hub_calls(oracle):
    """8 streams, fecblk 1 / 32 / 64 / 127, hostile losses, 3 calls; each merged with 5 skipped datagrams"""
    calls = tr.bank_calls(oracle, 300, ncalls=3)
    return calls, [merge(chunk, 40 + i, skip=5) for i, chunk in enumerate(calls)]


def stamps(i, S):
    return [1000 + 10 * i + s for s in range(S)], [37 * i + s for s in range(S)]


def rx_pair(ctx, S, L, fcpos, R=32):
    import sdrdaemon_amd as sd

    a = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, nb_fec=R)
    b = sd.RxPipe(ctx, S, log2decim=L, fcpos=fcpos, nb_fec=R)
    if L >= 3:  # (as test_gpu_rx_datagrams.prime: the open frames 300 decimated samples from full, so that few payloads complete frames)
        n = (F - 300) << L
        x = np.random.RandomState(5).randint(-32768, 32768, size=(S, n, 2)).astype(np.int16)
        for p in (a, b):
            assert not p.process_ragged(x, [n] * S, 999, 1)[1].any()
    return a, b


def same_rx_batch(got, exp, where):
    for s in range(len(exp)):
        assert got[s][1] == exp[s][1], (where, s)
        g, e = np.asarray(got[s][0]), np.asarray(exp[s][0])
        assert g.shape == e.shape and g.tobytes() == e.tobytes(), (where, s)


def same_rx_state(a, b, S, where):
    assert list(a.carry()) == list(b.carry()), where
    for s in range(S):
        assert a.collector_stats(s) == b.collector_stats(s), (where, s)


@pytest.mark.parametrize("pinned", [True, False])
@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("L,fcpos", [(0, 2), (4, 2), (1, 0)])
def test_rx_hub(oracle, ctx, L, fcpos, depth, pinned):
    """submit_datagrams_tagged against submit_datagrams of the same calls on a twin RxPipe: frames, records, the carry after every
    submit and the collector's statistics; then one untagged synchronous call on both handles: the state left behind is the same"""
    S = 8
    calls, merged = hub_calls(oracle)
    a, b = rx_pair(ctx, S, L, fcpos)
    a.set_async(depth=depth)
    b.set_async(depth=depth)
    keep, got, exp, frames = [], [], [], 0
    for i, (chunk, (arr, tags)) in enumerate(zip(calls, merged)):
        sec, usec = stamps(i, S)
        if pinned:  # (in place: the array stays untouched until the batch is collected)
            buf = ctx.host_alloc(arr.shape, np.uint8)
            buf[...] = arr
            keep.append(buf)
            arr = buf
        a.submit_datagrams_tagged(arr, tags, sec, usec)
        b.submit_datagrams(chunk, sec, usec)
        assert list(a.carry()) == list(b.carry()), i
        if depth == 1:
            got.append(a.collect_datagrams())
            exp.append(b.collect_datagrams())
    while len(got) < len(calls):
        got.append(a.collect_datagrams())
        exp.append(b.collect_datagrams())
    for i in range(len(calls)):
        same_rx_batch(got[i], exp[i], i)
        frames += sum(np.asarray(g[0]).shape[0] for g in got[i])
    assert frames >= 1 and sum(len(g[1]) for call in got for g in call) > S
    same_rx_state(a, b, S, "after the batches")
    last = tr.bank_calls(oracle, 301, ncalls=1)[0]
    same_rx_batch(a.process_datagrams(last, 7, 8), b.process_datagrams(last, 7, 8), "synchronous")
    same_rx_state(a, b, S, "after the synchronous call")
    for buf in keep:
        ctx.host_free(buf)
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 4. Tx
def same_tx_batch(got, exp, where):
    for s in range(len(exp)):
        assert got[s][2] == exp[s][2], (where, s)
        assert got[s][0].shape == exp[s][0].shape and got[s][0].tobytes() == exp[s][0].tobytes(), (where, s)
        assert np.array_equal(got[s][1], exp[s][1]), (where, s)


@pytest.mark.parametrize("log2interp", [0, 4])
def test_tx(oracle, ctx, log2interp):
    """the same calls, submit_datagrams_tagged against submit_datagrams on a twin TxPipe at x1 and x16: samples, block 0, records"""
    import sdrdaemon_amd as sd

    S = 8
    calls, merged = hub_calls(oracle)
    a, b = sd.TxPipe(ctx, S, log2interp), sd.TxPipe(ctx, S, log2interp)
    for p in (a, b):
        p.set_async(4)
    for chunk, (arr, tags) in zip(calls, merged):
        a.submit_datagrams_tagged(arr, tags)
        b.submit_datagrams(chunk)
    released = 0
    for i in range(len(calls)):
        got, exp = a.collect_datagrams(), b.collect_datagrams()
        same_tx_batch(got, exp, i)
        released += sum(len(g[2]) for g in got)
    assert released > S
    for s in range(S):
        assert a.collector_stats(s) == b.collector_stats(s), s
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 5. alternation
@pytest.mark.parametrize("pipe", ["rx", "tx"])
def test_tagged_and_untagged_submits_alternate(oracle, ctx, pipe):
    """tagged and untagged submits in turn on one handle against the all-untagged twin"""
    import sdrdaemon_amd as sd

    S = 8
    calls, merged = hub_calls(oracle)
    if pipe == "rx":
        a, b = rx_pair(ctx, S, 1, 2)
    else:
        a, b = sd.TxPipe(ctx, S, 2), sd.TxPipe(ctx, S, 2)
    for i, (chunk, (arr, tags)) in enumerate(zip(calls, merged)):
        extra = stamps(i, S) if pipe == "rx" else ()
        if i % 2 == 0:
            a.submit_datagrams_tagged(arr, tags, *extra)
        else:
            a.submit_datagrams(chunk, *extra)
        b.submit_datagrams(chunk, *extra)
    for i in range(len(calls)):
        (same_rx_batch if pipe == "rx" else same_tx_batch)(a.collect_datagrams(), b.collect_datagrams(), i)
    for s in range(S):
        assert a.collector_stats(s) == b.collector_stats(s), s
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_consume_nothing(oracle, ctx):
    """a tag equal to nstreams, NULL tags, a full ring, ragged batches in flight: all refused on the host, before any launch, and
    the next correct call gives what it would have given"""
    import sdrdaemon_amd as sd

    S = 8
    calls, merged = hub_calls(oracle)
    a, b = rx_pair(ctx, S, 0, 2)
    a.set_async(depth=1)
    b.set_async(depth=1)
    arr, tags = merged[0]
    bad = tags.copy()
    bad[len(bad) // 2] = S
    lib = ctx.lib
    st = (C.c_uint32 * S)()
    with pytest.raises(sd.SdrHipError) as e:
        a.submit_datagrams_tagged(arr, bad)
    assert e.value.code == EINVAL
    assert lib.sdrhip_rx_submit_datagrams_tagged(a.h, arr.ctypes.data, None, arr.shape[0], st, st) == EINVAL
    assert lib.sdrhip_rx_submit_datagrams_tagged(a.h, None, tags.ctypes.data_as(C.POINTER(C.c_uint16)), arr.shape[0], st, st) == EINVAL
    # the bank and the Tx pipe refuse the same tags
    bank, twin = sd.FECBufferBank(ctx, S), sd.FECBufferBank(ctx, S)
    with pytest.raises(sd.SdrHipError) as e:
        bank.write_and_read_tagged(arr, bad)
    assert e.value.code == EINVAL
    got, exp = bank.write_and_read_tagged(arr, tags), twin.write_and_read(calls[0])
    for s in range(S):
        assert got[s][2] == exp[s][2] and np.array_equal(got[s][0], exp[s][0]) and np.array_equal(got[s][1], exp[s][1]), s
    tx = sd.TxPipe(ctx, S, 0)
    with pytest.raises(sd.SdrHipError) as e:
        tx.submit_datagrams_tagged(arr, bad)
    assert e.value.code == EINVAL
    assert tx.collect_datagrams(wait=False) is None
    # nothing was consumed: the first correct batch
    assert a.collect_datagrams(wait=False) is None
    sec, usec = stamps(0, S)
    a.submit_datagrams_tagged(arr, tags, sec, usec)
    b.submit_datagrams(calls[0], sec, usec)
    # a full ring: SDRHIP_EBUSY, nothing consumed
    held = list(a.carry())
    with pytest.raises(sd.SdrHipError) as e:
        a.submit_datagrams_tagged(*merged[1], 1, 2)
    assert e.value.code == EBUSY and list(a.carry()) == held
    same_rx_batch(a.collect_datagrams(), b.collect_datagrams(), 0)
    # ragged batches in flight: SDRHIP_EINVAL
    x = np.random.RandomState(3).randint(-32768, 32768, size=(S, 64, 2)).astype(np.int16)
    for p in (a, b):
        p.submit_ragged(x, [64] * S, 1, 2)
    with pytest.raises(sd.SdrHipError) as e:
        a.submit_datagrams_tagged(*merged[1], 1, 2)
    assert e.value.code == EINVAL
    ra, rb = a.collect_ragged(wait=True), b.collect_ragged(wait=True)
    for s in range(S):
        assert np.asarray(ra[s]).tobytes() == np.asarray(rb[s]).tobytes(), s
    # and on: the remaining batches continue the streams
    for i in (1, 2):
        sec, usec = stamps(i, S)
        a.submit_datagrams_tagged(*merged[i], sec, usec)
        b.submit_datagrams(calls[i], sec, usec)
        same_rx_batch(a.collect_datagrams(), b.collect_datagrams(), i)
    same_rx_state(a, b, S, "end")
    assert mismatches(ctx) == 0


# ------------------------------------------------------------------------------------------------ 7. link counters
def test_link_bytes(oracle, ctx):
    """up: 512 bytes per datagram, skipped ones included, and 4 per datagram for the table of places; down: the untagged twin's"""
    S = 8
    calls, merged = hub_calls(oracle)
    a, b = rx_pair(ctx, S, 0, 2, R=8)
    for p in (a, b):
        p.carry()
        p._collector()  # (created on first use: its initial state goes up once)
        p.set_async(depth=1)
    ctx.synchronize()
    for i, (chunk, (arr, tags)) in enumerate(zip(calls, merged)):
        c0 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        a.submit_datagrams_tagged(arr, tags, i, 0)
        got = a.collect_datagrams()
        c1 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        b.submit_datagrams(chunk, i, 0)
        exp = b.collect_datagrams()
        c2 = ctx.counter("h2d_bytes"), ctx.counter("d2h_bytes")
        print("batch %d: n_total %d h2d %d d2h %d | untagged h2d %d d2h %d" % (i, len(tags), c1[0] - c0[0], c1[1] - c0[1], c2[0] - c1[0], c2[1] - c1[1]))
        assert len(tags) == sum(len(c) for c in chunk) + 5
        assert c1[0] - c0[0] == 516 * len(tags)
        assert c1[1] - c0[1] == c2[1] - c1[1]
        same_rx_batch(got, exp, i)
    assert mismatches(ctx) == 0
