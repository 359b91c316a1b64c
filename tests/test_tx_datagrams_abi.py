"""CPU-side checks of the Tx pipe fed datagrams (sdrhip_tx_process_datagrams, sdrhip_tx_collector): declared in include/sdrhip.h,
exported by libsdrhip.so, refused loudly without a GPU, and the ragged interpolator instantiations compile for gfx950 without
scratch and with no more registers than the uniform ones."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import interp_kernel_names as ikn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sdrhip_tx_process_datagrams", "sdrhip_tx_collector"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from sdrdaemon_amd import _lib

    return _lib


def test_declared_and_exported(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrhip.h")).read(), flags=re.S)
    lib = built.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in built.EXPORTS, n


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    nd, nf = (C.c_size_t * 1)(0), (C.c_size_t * 1)()
    assert lib.sdrhip_tx_process_datagrams(None, None, nd, 0, None, 0, 0, None, None, nf, 0) == -1
    h = C.c_void_p()
    assert lib.sdrhip_tx_collector(None, C.byref(h)) == -1 and not h.value
    with pytest.raises(sd.SdrHipError):
        sd.TxPipe(sd.Context(0), 4).process_datagrams([np.zeros((0, 512), np.uint8)] * 4)


def _resources(stderr):
    names = re.findall(r"Function Name: (\S+)", stderr)
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", stderr)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", stderr)]
    assert len(names) == len(vgprs) == len(scratch)
    return {n: (v, s) for n, v, s in zip(names, vgprs, scratch)}


def test_ragged_kernels_compile_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    csrc = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
    r = subprocess.run([hipcc, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "interp_kernels.hip"), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = _resources(r.stderr)
    # K5 (interpolate2 .. 64) and K5w (interpolate4 .. 64, one or four waves per workgroup)
    kernels = ikn.by_meaning(res)  # (path, L, WPW, flags) -> name
    ragged = {k: n for k, n in kernels.items() if k[3] == ikn.COUNT}
    assert len([k for k in ragged if k[0] == "valu"]) == 6 and len([k for k in ragged if k[0] == "wave"]) == 10, sorted(ragged.values())
    for (path, L, wpw, _), n in ragged.items():
        vg, sc = res[n]
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
        uniform = kernels[(path, L, wpw, 0)]  # the plain kernel of the same ratio and workgroup
        assert vg <= res[uniform][0], "%s: %d VGPRs, the uniform kernel %d" % (n, vg, res[uniform][0])
