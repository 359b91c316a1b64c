"""CPU-side checks of the per-stream input format (sdrhip_rx_set_stream_format / sdrhip_rx_get_stream_format): declared in
include/sdrhip.h with the documented prototypes, their citations and rules, exported, bound in Python, refused for a NULL handle and
loudly without a GPU; and K0x (rx_unpack_mixed_kernels.hip, a translation unit of its own: one kernel) compiles for gfx950 with no
scratch and no LDS."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import test_iq8_abi as iq8

built = iq8.built
SRC = "rx_unpack_mixed_kernels.hip"
NAMES = ["sdrhip_rx_set_stream_format", "sdrhip_rx_get_stream_format"]


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def _comment(h, at):
    """the comment in front of position `at`, its lines joined (the ' * ' that opens a line is no part of a phrase)"""
    return _norm(re.sub(r"\n \* ?", " ", h[h.rindex("/*", 0, at):at]))


def test_declared_exported_and_bound(built):
    src = _norm(re.sub(r"/\*.*?\*/", "", iq8._header(), flags=re.S))
    lib = built.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in built.EXPORTS, n
    assert "int sdrhip_rx_set_stream_format(sdrhip_rx *rx, const int *fmt);" in src
    assert "int sdrhip_rx_get_stream_format(const sdrhip_rx *rx, int stream, int *fmt);" in src
    # next to sdrhip_rx_set_stream_bits
    assert src.index("sdrhip_rx_get_stream_bits(") < src.index("sdrhip_rx_set_stream_format(") < src.index("sdrhip_rx_reset_streams(")
    vp, i, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    assert lib.sdrhip_rx_set_stream_format.argtypes == [vp, ip]
    assert lib.sdrhip_rx_get_stream_format.argtypes == [vp, i, ip]


def test_header_cites_the_reference_and_states_the_rules():
    h = iq8._header()
    at = h.index("int sdrhip_rx_set_stream_format")
    comment = _comment(h, at)
    for cite in ("RtlSdrSource.cpp:542-553", "HackRFSource.cpp:661-674", "sdrdaemonrx.cpp:264-374"):
        assert cite in comment, cite
    for word in ("SDRHIP_IQ_S16", "SDRHIP_IQ_U8", "SDRHIP_IQ_S8", "NULL = bank-wide again", "byte for byte", "sdrhip_rx_set_input_format(fmt[s])",
                 "implies none", "sdrhip_rx_process_ragged (host and device memory)", "sdrhip_rx_submit_ragged", "sdrhip_rx_collect_ragged",
                 "sdrhip_rx_collect_egress", "in any combination", "sdrhip_rx_set_pipelined(1)", "nothing consumed", "datagram entries ignore",
                 "4 * s * in_stride", "16-byte aligned", "a multiple of 4", "n_in[s] * bytes(fmt[s])", "SDRHIP_PACKED",
                 "sum_{t<s} n_in[t] * bytes(fmt[t])", "2 bytes off a dword", "array of equal entries", "host state only", "filled or in flight",
                 "one set of formats", "its value is unused", "sdrhip_rx_reconfigure and sdrhip_rx_reset_streams do not clear",
                 "same kernels in the same order with the same arguments", '"h2d_bytes"', "Not covered"):
        assert word in comment, word
    # the neighbour's comment points here now, and keeps the words its own test looks for
    at = h.index("int sdrhip_rx_set_stream_bits")
    bits = _comment(h, at)
    for word in ("Not covered", "sdrhip_rx_set_input_format", "the Tx pipe", "sdrhip_rx_set_stream_format"):
        assert word in bits, word
    assert "stays bank-wide" not in bits


def test_python_surface(built):
    import sdrdaemon_amd as sd

    p = inspect.signature(sd.RxPipe.set_stream_formats).parameters
    assert list(p) == ["self", "formats"] and p["formats"].default is None
    assert list(inspect.signature(sd.RxPipe.stream_format).parameters) == ["self", "stream"]
    src = inspect.getsource(sd.RxPipe.set_stream_formats)
    assert "_stream_ints(" in src and "sdrhip_rx_set_stream_format" in src
    for entry in (sd.RxPipe.process_ragged, sd.RxPipe.submit_ragged):
        assert "_formatted_input(" in inspect.getsource(entry)


def test_null_handle_and_range(built):
    lib = built.lib()
    f = C.c_int(7)
    fm = (C.c_int * 2)(1, 0)
    assert lib.sdrhip_rx_set_stream_format(None, fm) == -1
    assert lib.sdrhip_rx_set_stream_format(None, None) == -1
    assert lib.sdrhip_rx_get_stream_format(None, 0, C.byref(f)) == -1
    assert b"NULL" in lib.sdrhip_last_error()
    assert f.value == 7 and list(fm) == [1, 0]


def test_settings_type_refuses_values_outside_the_three_formats(tmp_path):
    """RxStreamSettings::set_format on a CPU: range, then room, then values; what it forces; NULL clears (the setter of the ABI adds
    the handle's own refusals in front of it)"""
    prog = tmp_path / "fmt.cpp"
    prog.write_text(r'''
#include "rx_stream_settings.h"
#include <cstdio>
using namespace sdrhip;
int main()
{
    RxStreamSettings st;
    st.init(3);
    if (st.forces_ragged() != RX_SET_NONE || st.formats() || st.format(2, 1) != 2) return 1;
    const int bad[3] = {0, 3, 1}, neg[3] = {-1, 0, 0}, ok[3] = {0, 1, 2};
    RxSetResult r = st.set_format(bad);
    if (r.kind != RxSetResult::RANGE || r.index != 1 || r.value != 3 || st.formats()) return 2;
    if (st.set_format(neg).kind != RxSetResult::RANGE || st.formats()) return 3;
    const uint64_t v = st.version();
    if (st.set_format(ok).kind != RxSetResult::OK || st.forces_ragged() != RX_SET_FORMAT || st.any()) return 4;
    if (st.format(0, 0) != 0 || st.format(0, 1) != 1 || st.format(0, 2) != 2 || st.version() != v) return 5;
    if (st.set_format(bad).kind != RxSetResult::RANGE || st.format(0, 1) != 1) return 6; // (refused: the old values stand)
    const unsigned bits[3] = {8, 12, 16};
    const int fec[3] = {1, 2, 3};
    st.set_bits(bits);
    if (st.forces_ragged() != RX_SET_BITS) return 7;
    st.set_fec(fec);
    if (st.forces_ragged() != RX_SET_FEC) return 8;
    st.set_bits(nullptr); st.set_fec(nullptr);
    if (st.forces_ragged() != RX_SET_FORMAT) return 9;
    if (st.set_format(nullptr).kind != RxSetResult::OK || st.forces_ragged() != RX_SET_NONE || st.formats()) return 10;
    std::printf("OK\n");
    return 0;
}
''')
    exe = str(tmp_path / "fmt")
    subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", iq8.CSRC, str(prog), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "OK" and not r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    with pytest.raises(ValueError):
        sd.engine._iq_format("u16", ("s16", "u8", "s8"))
    if sd.device_count() > 0:
        return
    with pytest.raises(sd.SdrHipError):  # (no GPU: no context, no pipe -- never a quiet host path)
        sd.RxPipe(sd.Context(0), 2).set_stream_formats(["u8", "s16"])
    with pytest.raises(sd.SdrHipError):
        sd.RxPipe(sd.Context(0), 2).process_ragged([np.zeros((4, 2), np.uint8), np.zeros((4, 2), np.int16)], None)


def test_kernel_compiles_without_scratch_and_lds(tmp_path):
    """one kernel in the new file; no scratch, no LDS, full occupancy (the figures DESIGN.md records: 20 VGPRs, 47 SGPRs)"""
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
    assert "19unpack_mixed_kernel" in name
    assert sc == 0 and lds[0] == 0
    assert vg <= 64 and occ == 8


def test_lives_in_a_translation_unit_of_its_own():
    """no other kernel file defines or launches it, the library's Makefile builds the new file, and the host sources have exactly one
    call site of K0x's launch and one of K0p's (the helper that the asynchronous batch and the synchronous ragged call share); both
    of those fill the table"""
    for f in sorted(os.listdir(iq8.CSRC)):
        if f.endswith(".hip") and f != SRC:
            assert "unpack_mixed" not in open(os.path.join(iq8.CSRC, f)).read(), f
    assert SRC in open(os.path.join(iq8.CSRC, "Makefile")).read()
    hosts = {f: open(os.path.join(iq8.CSRC, f)).read() for f in sorted(os.listdir(iq8.CSRC)) if f.endswith(".cpp")}
    for launch in ("launch_unpack_mixed(", "launch_unpack_packed("):
        assert sum(h.count(launch) for h in hosts.values()) == 1, launch
    for unit in ("sdrhip_rx.cpp", "sdrhip_rx_async.cpp"):
        assert "unpackx_fill(" in hosts[unit] and "rx_unpack_launch(" in hosts[unit], unit
    assert "RX_SET_FORMAT" in open(os.path.join(iq8.CSRC, "rx_stream_settings.h")).read()
