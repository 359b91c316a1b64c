"""The UDPSourceFEC drop-in adapter fed by a sender with 64 FEC blocks (the `rx` form of test_gpu_udp_adapters.py::
test_udpsourcefec_frames: Python sends the datagrams over loopback to tests/cxx/udp_adapter_test.cpp).  The adapter promises the
library nothing about the sender (dec_max_rows = auto, set once): a frame whose first 128 arrivals hold FEW recovery blocks but a row
>= 32 among them must decode like any other -- a count of the recovery blocks collected says nothing about their rows."""
import socket
import time

import numpy as np
import pytest

import signals
from test_gpu_udp_adapters import _free_port, exe  # noqa: F401  (the fixture compiles the adapter program)
from test_ref_fecbuffer import _run_oracle

R = 64


def _datagrams(oracle):
    """four frames of a fecblk-64 sender in wire order (originals first, then the recovery blocks) + a datagram that flushes the last"""
    rs = np.random.RandomState(64)
    x = signals.mixed(4 * 16129, 64)
    frames = oracle.framer(nb_fec_blocks=R).write(x)
    lost = [
        set(rs.choice(np.arange(1, 128), 20, replace=False).tolist()) | {128 + r for r in range(20)},  # A: the first 128 arrivals end with rows 20..39
        set(rs.choice(128, 40, replace=False).tolist()),                                               # B: 40 recovery blocks used
        set(range(1, 121, 5)),                                                                         # C: 24, rows 0..23
        set(),                                                                                         # D
    ]
    out, first128 = [], []
    for f in range(4):
        allb = np.concatenate([frames[f], oracle.frame_encode(frames[f], R)])
        sent = [i for i in range(128 + R) if i not in lost[f]]
        first128.append(sent[:128])
        out += [allb[i] for i in sent]
    out.append(np.full(512, 0xEE, np.uint8))
    return x, out, first128


@pytest.mark.gpu
def test_udpsourcefec_decodes_a_fecblk64_sender(exe, oracle, tmp_path):  # noqa: F811
    x, dgrams, first128 = _datagrams(oracle)
    rec = [[i - 128 for i in a if i >= 128] for a in first128]
    assert len(rec[0]) == 20 and max(rec[0]) == 39 and min(rec[0]) == 20  # few recovery blocks, rows >= 32 among them
    assert len(rec[1]) == 40 and len(rec[2]) == 24 and max(rec[2]) < 32 and not rec[3]
    exp, _, _ = _run_oracle(oracle, dgrams)
    assert len(exp) == 5
    port = _free_port()
    fout = str(tmp_path / "out.bin")
    import subprocess

    p = subprocess.Popen([exe, "rx", str(port), "5", fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        assert p.stdout.readline().strip() == "ready"
        tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        for d in dgrams:
            tx.sendto(np.ascontiguousarray(d).tobytes(), ("127.0.0.1", port))
            time.sleep(0.0005)  # the loopback receive buffer is small; the adapter decodes between datagrams
        out, err = p.communicate(timeout=60)
    finally:
        if p.poll() is None:
            p.kill()
    assert p.returncode == 0, err
    got = np.fromfile(fout, np.uint8).reshape(5, 127 * 508)
    assert not got[0].any()  # the collector's initial slot
    bad = [i for i in range(1, 5) if not np.array_equal(got[i], exp[i])]
    assert not bad, ("frames that differ from the oracle collector's (1 = A ... 4 = D)", bad)
    for f in range(4):  # all four are decodable: they carry the stream
        assert np.array_equal(got[f + 1].view(np.int16).reshape(-1, 2), x[f * 16129:(f + 1) * 16129]), f
    lines = [ln for ln in out.splitlines() if ln.startswith("frame ")]
    assert len(lines) == 5 and all("samples 16129" in ln for ln in lines)
