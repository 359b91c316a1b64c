"""enc_form = bitslice (gf_encode128_bs.h: the FFT encoder's middle stages as compile-time XOR trees on bit planes) against
enc_form = table and the oracle, byte for byte: row counts the FFT path serves, frame counts around the launch's residency steps and the Rx pipe's ways into the encoder (frames in memory, the fused framing copy with a straddling frame,
the encoder + K2 launch, the pipelined pipe)."""
import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sdrdaemon_amd as sd

    assert sd.device_count() > 0
    c = sd.Context(0)
    yield c
    c.set_option("enc_form", "bitslice")
    c.set_option("enc_units", "frame")
    c.set_option("rx_direct", 1)


def _both(ctx, fn):
    out = []
    for form in ("table", "bitslice"):
        ctx.set_option("enc_form", form)
        out.append(fn())
    ctx.set_option("enc_form", "bitslice")
    return out


@pytest.mark.parametrize("R", [1, 7, 16, 31, 32])
def test_bitslice_equals_table_and_oracle(ctx, oracle, R):
    import sdrdaemon_amd as sd

    F = 9
    x = signals.noise(F * 16129, 900 + R)
    frames = oracle.framer(nb_fec_blocks=R).write(x)
    frames[:, :, 3] = 0
    frames[F - 1, 1:] = 0xFF  # an all-0xFF payload
    a, b = _both(ctx, lambda: sd.fec_encode_frames(ctx, frames, R))
    assert np.array_equal(a, b), R
    for f in range(F):
        assert np.array_equal(b[f], oracle.frame_encode(frames[f], R)), (R, f)


@pytest.mark.parametrize("F", [1, 255, 256, 257, 1040, 1296])
def test_bitslice_frame_counts(ctx, F):
    import sdrdaemon_amd as sd

    rs = np.random.RandomState(F)
    frames = rs.randint(0, 256, size=(F, 128, 512)).astype(np.uint8)
    a, b = _both(ctx, lambda: sd.fec_encode_frames(ctx, frames, 32))
    assert np.array_equal(a, b), F


def test_bitslice_rx_pipe_paths(ctx):
    """ragged calls through the Rx pipe: rx_direct 1 / 0 (fused framing copy, straddling frame, meta blocks derived in the
    encoder + K2 launch), plain and pipelined"""
    import torch

    import sdrdaemon_amd as sd

    S, n = 3, (1 << 22) + 4 * 777
    xs = torch.from_numpy(np.stack([signals.noise(n, 80 + s) for s in range(S)])).cuda()
    cut = (n // 3 + 40) & ~3
    for R in (7, 32):
        for direct, pipelined in ((1, False), (0, False), (1, True), (0, True)):
            res = []
            for form in ("table", "bitslice"):
                ctx.set_option("enc_form", form)
                ctx.set_option("rx_direct", direct)
                rx = sd.RxPipe(ctx, S, log2decim=4, nb_fec=R, pipelined=pipelined)
                parts = [rx.process(xs[:, :cut], 1, 2), rx.process(xs[:, cut:], 3, 4)]
                if pipelined:
                    parts.append(torch.from_numpy(rx.flush()).cuda())
                res.append(torch.cat([p for p in parts if p.shape[1]], dim=1).clone())
            ctx.synchronize()
            assert torch.equal(res[0], res[1]), (R, direct, pipelined)
    ctx.set_option("enc_form", "bitslice")
    ctx.set_option("rx_direct", 1)


def test_half_units_run_the_table_form(ctx, oracle):
    """enc_units = half has no bit-sliced kernel: with enc_form = bitslice it runs the table form, same bytes"""
    import sdrdaemon_amd as sd

    F, R = 5, 32
    x = signals.noise(F * 16129, 31)
    frames = oracle.framer(nb_fec_blocks=R).write(x)
    frames[:, :, 3] = 0
    ctx.set_option("enc_units", "half")
    try:
        a, b = _both(ctx, lambda: sd.fec_encode_frames(ctx, frames, R))
    finally:
        ctx.set_option("enc_units", "frame")
    assert np.array_equal(a, b)
    for f in range(F):
        assert np.array_equal(b[f], oracle.frame_encode(frames[f], R)), f


def test_enc_form_rejects_unknown_values(ctx):
    with pytest.raises(Exception):
        ctx.set_option("enc_form", "planes")
