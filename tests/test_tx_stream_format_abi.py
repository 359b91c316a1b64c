"""CPU-side checks of the Tx pipe's per-stream output format (sdrhip_tx_set_stream_format / sdrhip_tx_get_stream_format): declared in
include/sdrhip.h with the documented prototypes, their citations and rules, exported, bound in Python, refused for a NULL handle and
loudly without a GPU; and K5x / K6x (interp_mixed_kernels.hip, a translation unit of its own) compile for gfx950 with no scratch and
within the registers and LDS their bank-wide twins allocate."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import interp_kernel_names as ikn
import test_iq8_abi as iq8
from test_rx_stream_format_abi import _comment, _norm

built = iq8.built
SRC = "interp_mixed_kernels.hip"
NAMES = ["sdrhip_tx_set_stream_format", "sdrhip_tx_get_stream_format"]


def test_declared_exported_and_bound(built):
    src = _norm(re.sub(r"/\*.*?\*/", "", iq8._header(), flags=re.S))
    lib = built.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in built.EXPORTS, n
    assert "int sdrhip_tx_set_stream_format(sdrhip_tx *tx, const int *fmt);" in src
    assert "int sdrhip_tx_get_stream_format(const sdrhip_tx *tx, int stream, int *fmt);" in src
    # directly behind sdrhip_rx_get_stream_format
    assert re.search(r"sdrhip_rx_get_stream_format\([^;]*\); int sdrhip_tx_set_stream_format\([^;]*\); int sdrhip_tx_get_stream_format\(", src)
    vp, i, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    assert lib.sdrhip_tx_set_stream_format.argtypes == [vp, ip]
    assert lib.sdrhip_tx_get_stream_format.argtypes == [vp, i, ip]


def test_header_cites_the_reference_and_states_the_rules():
    h = iq8._header()
    comment = _comment(h, h.index("int sdrhip_tx_set_stream_format"))
    for cite in ("HackRFSink.cpp:671-672", "FileSink.cpp:216-277", "sdrdaemontx.cpp:195-255"):
        assert cite in comment, cite
    for word in ("SDRHIP_IQ_S16 or SDRHIP_IQ_S8", "NULL = bank-wide again", "byte for byte", "sdrhip_tx_set_output_format(fmt[s])",
                 "samples, meta blocks, records and all carried histories", "sdrhip_tx_process (host and device memory)", "pipelined mode",
                 "sdrhip_tx_flush", "sdrhip_tx_submit", "sdrhip_tx_collect", "sdrhip_tx_process_datagrams", "sdrhip_tx_submit_datagrams",
                 "sdrhip_tx_submit_datagrams_tagged", "sdrhip_tx_collect_datagrams", "when it is handed in", "as it takes the factor",
                 "4 * s * out_stride", "4-byte units", "first 2 * n bytes", "nothing behind them is written", "16-byte aligned", "a multiple of 4",
                 "SDRHIP_EALIGN", "array of equal entries", "host state only", "nothing is enqueued", "SDRHIP_IQ_U8", "batches are in flight",
                 "a pipelined batch waits", "its value is unused", "sdrhip_tx_reconfigure and sdrhip_tx_reset_streams do not clear",
                 "takes the destination's format", "tx_gather", "same kernels in the same order with the same arguments",
                 "sum_s n[s] * bytes(fmt[s])", '"d2h_bytes"', "Not covered"):
        assert word in comment, word
    # the Rx neighbour no longer names the gap, and keeps the words its own tests look for
    rxc = _comment(h, h.index("int sdrhip_rx_set_stream_format"))
    assert "an output format per stream of the Tx pipe" not in rxc
    for word in ("Not covered", "sdrhip_tx_set_stream_format"):
        assert word in rxc, word


def test_python_surface(built):
    import sdrdaemon_amd as sd

    p = inspect.signature(sd.TxPipe.set_stream_formats).parameters
    assert list(p) == ["self", "formats"] and p["formats"].default is None
    assert list(inspect.signature(sd.TxPipe.stream_format).parameters) == ["self", "stream"]
    assert "sdrhip_tx_set_stream_format" in inspect.getsource(sd.TxPipe.set_stream_formats)
    assert "sdrhip_tx_get_stream_format" in inspect.getsource(sd.TxPipe.stream_format)
    for entry in (sd.TxPipe.process, sd.TxPipe.collect, sd.TxPipe.flush):
        assert "_rows(" in inspect.getsource(entry), entry
    for entry in (sd.TxPipe.process_datagrams, sd.TxPipe.collect_datagrams):
        assert "_dg_result(" in inspect.getsource(entry), entry


def test_rows_of_a_mixed_buffer():
    """TxPipe._rows / _out without a handle: one array per stream, of its own dtype, at byte 4 * s * pitch"""
    import sdrdaemon_amd as sd

    p = sd.TxPipe.__new__(sd.TxPipe)
    p.nstreams, p._stream_formats, p._out_dtype = 3, ["s16", "s8", "s16"], np.int16
    out, pad = p._out(3, 5)
    assert out.shape == (3, 32) and out.dtype == np.uint8 and pad == 8
    out[:] = np.arange(96, dtype=np.uint8).reshape(3, 32)
    r = p._rows(out, 5)
    assert [a.dtype for a in r] == [np.int16, np.int8, np.int16] and all(a.shape == (5, 2) for a in r)
    assert r[1][4, 1] == 32 + 9 and r[2].view(np.uint8)[0, 0] == 64
    r = p._rows(out, [1, 0, 2])
    assert [a.shape for a in r] == [(1, 2), (0, 2), (2, 2)]
    p._stream_formats = None
    out, pad = p._out(3, 5)
    assert out.shape == (3, 8, 2) and out.dtype == np.int16 and p._rows(out, 5).shape == (3, 5, 2)
    p.h = None  # (no handle: nothing to destroy)


def test_null_handle_and_range(built):
    lib = built.lib()
    f = C.c_int(7)
    fm = (C.c_int * 2)(2, 0)
    assert lib.sdrhip_tx_set_stream_format(None, fm) == -1
    assert lib.sdrhip_tx_set_stream_format(None, None) == -1
    assert lib.sdrhip_tx_get_stream_format(None, 0, C.byref(f)) == -1
    assert b"NULL" in lib.sdrhip_last_error()
    assert f.value == 7 and list(fm) == [2, 0]


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    with pytest.raises(ValueError):
        sd.engine._iq_format("u8", ("s16", "s8"))  # (U8 is no Tx format: the names are checked before the library is asked)
    if sd.device_count() > 0:
        return
    with pytest.raises(sd.SdrHipError):  # (no GPU: no context, no pipe -- never a quiet host path)
        sd.TxPipe(sd.Context(0), 2).set_stream_formats(["s8", "s16"])


def _compile(tmp_path, src):
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(iq8.CSRC, src), "-o", str(tmp_path / (src + ".o"))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = iq8._resources(r.stderr)
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(lds) == len(res)
    return {n: v + (l,) for (n, v), l in zip(res.items(), lds)}  # VGPRs, scratch, occupancy, LDS bytes


# The K5x families: a table variant (path, flags) of interp_variant.h; its two bank-wide twins are the kernels of the same
# (path, L, WPW) with the table flag taken away (int16) or replaced by the 8-bit flag.  (The case ids are the ones these cases have
# always had: the name fragments of the four templates the table variants replaced.)
FAMILIES = {"30interp_wave_mixed_count_kernel": ("wave", ikn.TABLE | ikn.COUNT), "24interp_wave_mixed_kernel": ("wave", ikn.TABLE),
            "25interp_mixed_count_kernel": ("valu", ikn.TABLE | ikn.COUNT), "19interp_mixed_kernel": ("valu", ikn.TABLE)}


def _twins(flags):
    return (flags & ~ikn.TABLE, (flags & ~ikn.TABLE) | ikn.S8)


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """the resource reports of the new file and of interp_kernels.hip (its twins), compiled once"""
    d = tmp_path_factory.mktemp("k5x")
    return _compile(d, SRC), _compile(d, "interp_kernels.hip")


def test_no_scratch_and_the_kernels_that_are_there(resources):
    res, _ = resources
    kernels = ikn.by_meaning(res)
    k5x = [n for k, n in kernels.items() if k[3] & ikn.TABLE]
    # K5w x4 .. x64 with one or four waves per workgroup, K5 x2 .. x64, each uniform and with per-stream counts; K6x
    for path, flags in FAMILIES.values():
        assert len([k for k in kernels if k[0] == path and k[3] == flags]) == (10 if path == "wave" else 6), (path, flags)
    assert len(k5x) == 2 * (10 + 6) and len(kernels) == len(k5x) and len(res) == len(k5x) + 1, sorted(res)
    for n, (vg, sc, occ, lds) in sorted(res.items()):
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        if n not in k5x:  # K6x: no LDS, full occupancy
            assert "20interp1_mixed_kernel" in n and lds == 0 and vg <= 64 and occ == 8, (n, vg, lds, occ)


@pytest.mark.parametrize("family,L", [(f, L) for f in sorted(FAMILIES) for L in range(2 if FAMILIES[f][0] == "wave" else 1, 7)])
def test_kernels_compile_within_their_twins_resources(resources, family, L):
    """Every K5x kernel reports no more VGPRs and no more LDS than the larger of its two bank-wide twins, at no lower occupancy; the
    reported counts are printed.  (Each branch of a K5x kernel ends in an assembly comment of its own, so that the two bodies do not
    share a tail: with one shared, K5 x64 reported 74 VGPRs against its twins' 68 and 70.)"""
    res, base = resources
    path, flags = FAMILIES[family]
    base_kernels = ikn.by_meaning(base)
    missed, seen = [], 0
    for (p, l, wpw, f), n in sorted(ikn.by_meaning(res).items(), key=str):
        if (p, l, f) != (path, L, flags):
            continue
        seen += 1
        vg, sc, occ, lds = res[n]
        assert n.endswith("PKi"), n  # (the table: the last kernel argument)
        twins = [base[base_kernels[(path, L, wpw, t)]] for t in _twins(flags)]
        tv, tl = max(t[0] for t in twins), max(t[3] for t in twins)
        print(n, "VGPRs", vg, "twins", [t[0] for t in twins], "LDS", lds, "twins", tl, "occupancy", occ, [t[2] for t in twins])
        assert lds <= tl, "%s: %d bytes of LDS, its twins %d" % (n, lds, tl)
        assert occ >= min(t[2] for t in twins), "%s: occupancy %d, its twins %s" % (n, occ, [t[2] for t in twins])
        if vg > tv:
            missed.append("%s: %d VGPRs, the larger of its twins %d" % (n, vg, tv))
    assert seen == (2 if path == "wave" else 1)  # (K5w: one and four waves per workgroup)
    assert not missed, missed


def test_lives_in_a_translation_unit_of_its_own(resources):
    """no other kernel file instantiates a table variant or launches K6x -- by its text and, for interp_kernels.hip, which includes the
    same templates, by its compile report --, the library's Makefile builds the file, InterpArgs did not grow (the table is a second
    kernel argument), and the host has one call site of the bank's one launcher and one of the K6x launch"""
    _, base = resources
    assert len(ikn.by_meaning(base)) == len(base) == 74 and not [k for k in ikn.by_meaning(base) if k[3] & ikn.TABLE], sorted(base)
    for f in sorted(os.listdir(iq8.CSRC)):
        if f.endswith(".hip") and f != SRC:
            text = open(os.path.join(iq8.CSRC, f)).read()
            assert not re.search(r"variant(_kernel)?<[^>;]*IV_TABLE", text) and "interp1_mixed" not in text, f
            assert ('#include "interp_variant.h"' in text) == (f == "interp_kernels.hip"), f
    assert SRC in open(os.path.join(iq8.CSRC, "Makefile")).read()
    text = open(os.path.join(iq8.CSRC, SRC)).read()
    assert "launch_variant<IV_TABLE>" in text and "launch_variant<IV_TABLE | IV_COUNT>" in text
    variant = open(os.path.join(iq8.CSRC, "interp_variant.h")).read()
    assert variant.count("InterpArgs a, const int *fmt") == 2 and "readfirstlane(fmt[blockIdx.y])" in variant
    internal = open(os.path.join(iq8.CSRC, "sdrhip_internal.h")).read()
    args = internal[internal.index("struct InterpArgs {"):internal.index("};", internal.index("struct InterpArgs {"))]
    assert "fmt" not in args
    assert len(re.findall(r"^hipError_t launch_interpolate\w*\(", internal, flags=re.M)) == 3  # the launcher, its table half, K6x
    hosts = {f: open(os.path.join(iq8.CSRC, f)).read() for f in sorted(os.listdir(iq8.CSRC)) if f.endswith(".cpp")}
    for launch in ("launch_interpolate(", "launch_interpolate1_mixed("):
        assert sum(h.count(launch) for h in hosts.values()) == 1, launch
    assert not any("launch_interpolate_table(" in h for h in hosts.values())  # (reached through the one launcher alone)
