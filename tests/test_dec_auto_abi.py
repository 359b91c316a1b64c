"""CPU-side checks of dec_max_rows = auto (the batched CM256 decoder decides per frame between its one-launch form and the general
chain): include/sdrhip.h states the mode, the deferral rule, the byte guarantee and the counter; the library builds; and the hot kernel
-- gf_decode128_fft_plan_kernel<false>, which gained the deferral -- keeps its residency on gfx950: no scratch, at most 128 VGPRs, at
most 40 KB of LDS (four workgroups per CU).  The parent: 126 VGPRs (125 allocated before the granule), 36.4 KB."""
import os
import re
import subprocess

import pytest

import test_iq8_abi as iq8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
built = iq8.built


def _norm(s):
    return re.sub(r"[\s*]+", " ", s)


def _header():
    return open(os.path.join(ROOT, "include", "sdrhip.h")).read()


def test_option_paragraph_names_auto_the_rule_and_the_guarantee():
    h = _header()
    at = h.index("int sdrhip_ctx_set_option")
    par = _norm(h[h.rindex("/*", 0, at):at])
    for word in ('"dec_max_rows" = 1..128 | auto (default 128)', "N > 32", "maxrow >= 32", "DEFERRED iff", "mode, not a promise",
                 "header byte 2", "`indices` array", "byte for byte as under dec_max_rows = 128", '"dec_rows_exceeded" does not grow',
                 '"dec_deferred"', "bounds their row indices", "sender's fecblk", "not a count of the recovery blocks that happened to arrive",
                 "dec_plan = kernel, dec_path = dense, enc_path = karatsuba", '"tx_gather" keeps requiring a number <= 32'):
        assert word in par, word


def test_counter_paragraph_names_dec_deferred():
    h = _header()
    at = h.index("int sdrhip_ctx_get_counter")
    par = _norm(h[h.rindex("/*", 0, at):at])
    assert '"dec_deferred" = frames' in par
    assert "does not grow under dec_max_rows = auto" in par
    assert "recovery row >= 32" in par and "more than 32 recovery blocks" in par


def test_the_library_builds_and_python_documents_the_mode(built):
    import sdrdaemon_amd as sd

    lib = built.lib()
    assert hasattr(lib, "sdrhip_ctx_set_option") and hasattr(lib, "sdrhip_ctx_get_counter")
    assert "auto" in sd.Context.set_option.__doc__ and "dec_max_rows" in sd.Context.set_option.__doc__
    assert "dec_deferred" in sd.Context.counter.__doc__


def test_the_adapter_sets_auto_once_and_no_count():
    a = open(os.path.join(ROOT, "sdrdaemon_amd", "adapters", "UDPSourceFEC.h")).read()
    assert a.count('"dec_max_rows"') == 2  # (the comment and the one call)
    assert 'sdrhip_ctx_set_option(m_ctx, "dec_max_rows", "auto")' in a
    ctor = a[a.index("sdrhip_ctx_create("):a.index("m_open.reset(-1)")]
    assert '"dec_max_rows", "auto"' in ctor, "set when the handle is created, not per batch"


def test_hot_kernel_keeps_its_residency(tmp_path):
    """-Rpass-analysis=kernel-resource-usage of gf_kernels.hip, as the library's Makefile compiles it; the figures DESIGN.md records
    (K4f section): 126 VGPRs, no scratch, 36372 bytes of LDS"""
    if not os.path.exists(iq8.HIPCC):
        pytest.skip("hipcc not present")
    r = subprocess.run([iq8.HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(iq8.CSRC, "gf_kernels.hip"), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = iq8._resources(r.stderr)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(lds) == len(res)
    hot = [n for n in names if "gf_decode128_fft_plan_kernelILb0EE" in n]
    assert len(hot) == 1, names
    vg, sc, occ = res[hot[0]]
    lb = dict(zip(names, lds))[hot[0]]
    print(hot[0], "VGPRs", vg, "scratch", sc, "occupancy", occ, "LDS", lb)
    assert sc == 0
    assert vg <= 128
    assert lb <= 40 * 1024
    assert occ >= 4
    d = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%d VGPRs, no scratch, %d bytes of LDS" % (vg, lb) in d, "DESIGN.md (K4f) records the three numbers"
