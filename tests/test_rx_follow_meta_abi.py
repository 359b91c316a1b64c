"""CPU-side checks of the outgoing meta that follows the incoming meta blocks (sdrhip_rx_set_follow_meta): declared in
include/sdrhip.h with the documented prototype and its citations, exported by libsdrhip.so and reachable from Python, a NULL handle
refused, and KF (rx_follow_kernels.hip, a translation unit of its own: one kernel, one lane per stream) compiles for gfx950 with no
scratch and no LDS, its stores plain vector stores of the lane."""
import inspect
import os
import re
import subprocess

import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = "int sdrhip_rx_set_follow_meta(sdrhip_rx *rx, int on);"
SRC = "rx_follow_kernels.hip"
built = iq8.built


def _norm(s):
    return re.sub(r"\s+", " ", s).replace("( ", "(").strip()


def _header():
    return open(os.path.join(ROOT, "include", "sdrhip.h")).read()


def test_declared_with_the_documented_prototype_and_exported(built):
    src = _norm(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    assert _norm(PROTO) in src
    assert hasattr(built.lib(), "sdrhip_rx_set_follow_meta")
    assert "sdrhip_rx_set_follow_meta" in built.EXPORTS


def test_header_states_the_contract_and_cites_the_reference():
    h = _header()
    at = h.index("int sdrhip_rx_set_follow_meta")
    comment = h[h.rindex("/*", 0, at):at]
    for cite in ("SDRdaemonFECBuffer.cpp:72-85", "SDRdaemonFECBuffer.cpp:150-153", "sdrdaemonrx.cpp:622-631,644", "UDPSinkFEC.cpp:160-165"):
        assert cite in comment, cite
    for word in ("host-side flag only", "a batch in flight keeps the mode", "ignore the flag", ">> log2decim",
                 "sdrhip_rx_get_stream_meta keeps reporting the host's values", "on = 0 is"):
        assert word in _norm(comment), word
    # (the getter's own comment says where the followed values are read)
    at = h.index("int sdrhip_rx_get_stream_meta")
    assert "sdrhip_fecbuf_stats" in h[h.rindex("/*", 0, at):at]


def test_null_handle_is_refused(built):
    lib = built.lib()
    assert lib.sdrhip_rx_set_follow_meta(None, 1) == -1  # SDRHIP_EINVAL
    assert lib.sdrhip_rx_set_follow_meta(None, 0) == -1
    assert b"NULL" in lib.sdrhip_last_error()


def test_python_surface(built):
    import sdrdaemon_amd as sd

    p = inspect.signature(sd.RxPipe.set_follow_meta).parameters
    assert list(p)[1:] == ["on"] and p["on"].default is True


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 2).set_follow_meta()


def test_kernel_compiles_without_scratch_and_lds(tmp_path):
    """one kernel in the new file; no scratch, no LDS, full occupancy (the figures DESIGN.md records: 13 VGPRs, 14 SGPRs)"""
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(iq8.CSRC, SRC), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = iq8._resources(r.stderr)
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(res) == len(lds) == 1, sorted(res)
    (name, (vg, sc, occ)), = res.items()
    print(name, "VGPRs", vg, "scratch", sc, "occupancy", occ, "LDS", lds[0])
    assert "21rx_follow_meta_kernel" in name
    assert sc == 0 and lds[0] == 0
    assert vg <= 32 and occ == 8


def test_kernel_stores_three_words_per_lane(tmp_path):
    """plain stores from the lane: three global dword stores into the row, no atomics, no LDS traffic, no scratch, no flat access"""
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    out = tmp_path / "k.s"
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(iq8.CSRC, SRC),
                        "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    bodies = [b for b in re.split(r"\n(?=_ZN\S+:)", out.read_text()) if re.match(r"_ZN\S*rx_follow_meta_kernel\S*:", b)]
    assert len(bodies) == 1
    body = bodies[0].split(".Lfunc_end")[0]
    stores = re.findall(r"\bglobal_store_dword(x\d)?\b", body)
    assert sum(int(x[1]) if x else 1 for x in stores) == 3, stores
    assert not re.search(r"global_atomic|flat_(load|store|atomic)|\bds_|scratch_", body)


def test_lives_in_a_translation_unit_of_its_own():
    """no other kernel file launches or defines it, and the library's Makefile builds the new file"""
    for f in sorted(os.listdir(iq8.CSRC)):
        if f.endswith(".hip") and f != SRC:
            assert "rx_follow_meta" not in open(os.path.join(iq8.CSRC, f)).read(), f
    assert SRC in open(os.path.join(iq8.CSRC, "Makefile")).read()
    host = open(os.path.join(iq8.CSRC, "sdrhip_rx.cpp")).read()
    assert host.count("launch_rx_follow_meta(") == 1
    # behind the table's upload, in front of the decimator launch
    assert host.index("ragged_prepare(rx->dec") < host.index("launch_rx_follow_meta(") < host.index("decimate_ragged_device(rx->dec")
