"""CPU-side checks of the sample size that follows the incoming meta blocks (sdrhip_rx_set_follow_bits): declared in include/sdrhip.h
with the documented prototype and contract, exported by libsdrhip.so and reachable from Python, a NULL handle refused, and KFb
(rx_follow_bits_kernels.hip, a translation unit of its own: one kernel, one lane per stream) compiles for gfx950 with no scratch and
no LDS, its stores three plain dwords of the lane."""
import inspect
import os
import re
import subprocess

import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTO = "int sdrhip_rx_set_follow_bits(sdrhip_rx *rx, int on);"
SRC = "rx_follow_bits_kernels.hip"
KERNEL = "rx_follow_bits_kernel"
built = iq8.built


def _norm(s):
    return re.sub(r"\s+", " ", s).replace("( ", "(").strip()


def _header():
    return open(os.path.join(ROOT, "include", "sdrhip.h")).read()


def _comment(h, proto):
    at = h.index(proto)
    return _norm(re.sub(r"\n \*", " ", h[h.rindex("/*", 0, at):at]))  # (the lines of a comment joined: a phrase may wrap)


def test_declared_with_the_documented_prototype_and_exported(built):
    src = _norm(re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    assert _norm(PROTO) in src
    assert hasattr(built.lib(), "sdrhip_rx_set_follow_bits")
    assert "sdrhip_rx_set_follow_bits" in built.EXPORTS


def test_header_states_the_contract_and_cites_the_reference():
    h = _header()
    comment = _comment(h, "int sdrhip_rx_set_follow_bits")
    for cite in ("SDRdaemonFECBuffer.cpp:72-85", "SDRdaemonFECBuffer.cpp:150-153", "sdrdaemonrx.cpp:619-623, 639-643", "Decimators.cpp:27-32, 43-44",
                 "UDPSinkFEC.cpp:160-165"):
        assert cite in comment, cite
    for word in ("on = 0 is the default", "host-side flag only", "nothing is enqueued, nothing is waited for", "also with batches in flight",
                 "a batch in flight keeps the mode", "ignore the flag", "independent of sdrhip_rx_set_follow_meta", "either flag, both or neither",
                 "rule 1 of sdrhip_rx_set_follow_meta", "m_outputMeta.m_sampleBits", "1 <= b <= 16", "held back from earlier calls",
                 "(b' - 1) / 8 + 1", "Only byte 9 is read", "a sender that says 0", "a value above 16", "sdrhip_rx_set_stream_bits array",
                 "cfg.sample_bits", "the followed value wins", "the samples take the new shift at once",
                 "sdrhip_rx_get_stream_bits keeps reporting the host's values", "contains the followed bytes 8 and 9",
                 "in the same order, with the same arguments", "sdrhip_rx_reconfigure", "sdrhip_rx_export_stream", "sdrhip_rx_import_stream",
                 "sdrhip_rx_reset_streams", "falls back under rule 3", "a submit still synchronises nothing", "NULL handle"):
        assert word in comment, word
    # the three sentences the flag relaxes say so, each in its own comment
    assert "unless sdrhip_rx_set_follow_bits is on" in _comment(h, "int sdrhip_rx_set_follow_meta")
    for proto in ("int sdrhip_rx_set_stream_bits", "int sdrhip_rx_set_stream_format"):
        c = _comment(h, proto)
        assert re.search(r"Not covered: [^.]*following sampleBits from the incoming meta blocks unless sdrhip_rx_set_follow_bits is on", c), proto


def test_null_handle_is_refused(built):
    lib = built.lib()
    assert lib.sdrhip_rx_set_follow_bits(None, 1) == -1  # SDRHIP_EINVAL
    assert lib.sdrhip_rx_set_follow_bits(None, 0) == -1
    assert b"NULL" in lib.sdrhip_last_error()


def test_python_surface(built):
    import sdrdaemon_amd as sd

    p = inspect.signature(sd.RxPipe.set_follow_bits).parameters
    assert list(p)[1:] == ["on"] and p["on"].default is True


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 2).set_follow_bits()


def test_kernel_compiles_without_scratch_and_lds(tmp_path):
    """one kernel in the new file; no scratch, no LDS, full occupancy; the register counts are the figures DESIGN.md records"""
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(iq8.CSRC, SRC), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = iq8._resources(r.stderr)
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    sgprs = [int(x) for x in re.findall(r"TotalSGPRs: (\d+)", r.stderr)]
    assert len(res) == len(lds) == len(sgprs) == 1, sorted(res)
    (name, (vg, sc, occ)), = res.items()
    print(name, "VGPRs", vg, "SGPRs", sgprs[0], "scratch", sc, "occupancy", occ, "LDS", lds[0])
    assert KERNEL in name
    assert sc == 0 and lds[0] == 0
    assert vg <= 32 and occ == 8
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "KFb %d VGPRs, %d SGPRs" % (vg, sgprs[0]) in design


def test_kernel_stores_three_words_per_lane(tmp_path):
    """plain stores from the lane: three global dwords into the row, no atomics, no LDS traffic, no scratch, no flat access"""
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    out = tmp_path / "k.s"
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S", os.path.join(iq8.CSRC, SRC),
                        "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    bodies = [b for b in re.split(r"\n(?=_ZN\S+:)", out.read_text()) if re.match(r"_ZN\S*%s\S*:" % KERNEL, b)]
    assert len(bodies) == 1
    body = bodies[0].split(".Lfunc_end")[0]
    stores = re.findall(r"\bglobal_store_dword(x\d)?\b", body)
    assert sum(int(x[1]) if x else 1 for x in stores) == 3, stores
    assert not re.search(r"global_atomic|flat_(load|store|atomic)|\bds_|scratch_", body)


def test_lives_in_a_translation_unit_of_its_own():
    """no other kernel file launches or defines it, the library's Makefile builds the new file, and the ragged step launches it once:
    behind the table's upload, in front of KF"""
    for f in sorted(os.listdir(iq8.CSRC)):
        if f.endswith(".hip") and f != SRC:
            assert "rx_follow_bits" not in open(os.path.join(iq8.CSRC, f)).read(), f
    assert SRC in open(os.path.join(iq8.CSRC, "Makefile")).read()
    host = open(os.path.join(iq8.CSRC, "sdrhip_rx.cpp")).read()
    assert host.count("launch_rx_follow_bits(") == 1
    assert host.index("ragged_prepare(rx->dec") < host.index("launch_rx_follow_bits(") < host.index("launch_rx_follow_meta(")
    # (K2r's job is the step planner's decision: the ragged step asks it with the flag, the rule itself stands in rx_step_plan.h)
    assert "rx_ragged_k2r(" in host and "call.follow_bits != nullptr" in host
    assert "!direct || sw || follow || follow_bits" in open(os.path.join(iq8.CSRC, "rx_step_plan.h")).read()


def test_arithmetic_is_one_text_for_host_and_device():
    """the kernel file includes the host's header and calls its rule; the header marks the shared functions for both sides and stays
    free of HIP without hipcc"""
    k = open(os.path.join(iq8.CSRC, SRC)).read()
    assert '#include "rx_stream_settings.h"' in k and "followed_size_words(" in k
    h = open(os.path.join(iq8.CSRC, "rx_stream_settings.h")).read()
    for f in ("decimated_sample_size", "decimated_shifts", "ragged_shift_word", "followed_size_words"):
        assert re.search(r"RX_HD inline \w+ %s\(" % f, h), f
    assert re.search(r"#if defined\(__HIPCC__\)\s*#define RX_HD __host__ __device__\s*#else\s*#define RX_HD\s*#endif", h)
