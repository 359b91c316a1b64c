"""CPU-side checks of the FEC buffer bank (sdrhip_fecbuf_*): declared in include/sdrhip.h, exported by libsdrhip.so, refused
loudly without a GPU, and its kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sdrhip_fecbuf_create", "sdrhip_fecbuf_destroy", "sdrhip_fecbuf_reset", "sdrhip_fecbuf_write_and_read", "sdrhip_fecbuf_stats"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from sdrdaemon_amd import _lib

    return _lib


def test_declared_and_exported(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrhip.h")).read(), flags=re.S)
    assert "sdrhip_fecbuf_frame" in src
    lib = built.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in built.EXPORTS, n


def test_frame_record_layout(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "sdrhip.h"\n#include <stddef.h>\n'
                 'typedef char chk[(sizeof(sdrhip_fecbuf_frame) == 16 && offsetof(sdrhip_fecbuf_frame, flags) == 12) ? 1 : -1];\n'
                 'int main(void){return SDRHIP_FECBUF_DECODED + SDRHIP_FECBUF_META + SDRHIP_FECBUF_REPAIRED + SDRHIP_FECBUF_DECODE_ERROR != 15;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-c", "-o", str(tmp_path / "t.o")],
                   check=True)


def test_no_gpu_means_loud_failure(built):
    import sdrdaemon_amd as sd

    if sd.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = built.lib()
    h = C.c_void_p()
    rc = lib.sdrhip_fecbuf_create(None, 4, C.byref(h))
    assert rc == -1 and not h.value
    assert lib.sdrhip_fecbuf_write_and_read(None, None, None, 0, None, 0, None, 0, None, None, 0) == -1
    with pytest.raises(sd.SdrHipError):
        sd.FECBufferBank(sd.Context(0), 4)


def test_kernels_compile_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    csrc = os.path.join(ROOT, "sdrdaemon_amd", "csrc")
    r = subprocess.run([hipcc, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "fecbuf_kernels.hip"), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    kernels = {n for n in names if "fecbuf" in n}
    assert len(kernels) == 3, names
    assert len(scratch) == len(names)
    for n, sc in zip(names, scratch):
        assert sc == 0, "%s uses %d bytes of scratch" % (n, sc)
