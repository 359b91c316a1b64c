"""CPU-side checks of the per-stream lifecycle entries (sdrhip_*_reset_streams, sdrhip_*_export_stream / _import_stream):
declared in include/sdrhip.h with the constructors they stand for, exported by libsdrhip.so, bound in sdrdaemon_amd/_lib.py and
present in the Python surface; a NULL handle is refused with SDRHIP_EINVAL by every one of them (the two size queries answer 0);
the header still compiles as C99 and C++11."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESET = ["sdrhip_decimators_reset_streams", "sdrhip_interpolators_reset_streams", "sdrhip_fecbuf_reset_streams",
         "sdrhip_rx_reset_streams", "sdrhip_tx_reset_streams"]
MOVE = ["sdrhip_rx_export_stream", "sdrhip_rx_import_stream", "sdrhip_tx_export_stream", "sdrhip_tx_import_stream"]
SIZES = ["sdrhip_rx_stream_state_bytes", "sdrhip_tx_stream_state_bytes"]
EINVAL = -1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from sdrdaemon_amd import _lib

    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "sdrhip.h")).read()


def test_header_and_binding_agree(built):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = built.lib()
    for n in RESET:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % n, src)
        assert m, n
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 2 and args[1].replace(" ", "") == "constuint8_t*mask", (n, args)
        assert n in built.EXPORTS, n
        fn = getattr(lib, n)
        assert fn.argtypes is not None and len(fn.argtypes) == 2, n
        assert fn.argtypes[0] is C.c_void_p and fn.argtypes[1] is C.POINTER(C.c_uint8), n
    for n in MOVE:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % n, src)
        assert m, n
        args = [a.strip().replace(" ", "") for a in m.group(1).split(",")]
        assert args[1:] == ["intstream", "void*blob" if "export" in n else "constvoid*blob", "size_tbytes"], (n, args)
        fn = getattr(lib, n)
        assert n in built.EXPORTS and fn.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t], n
    for n in SIZES:
        assert re.search(r"\bsize_t\s+%s\s*\(\s*const\s+sdrhip_[rt]x\s*\*" % n, src), n
        assert n in built.EXPORTS and getattr(lib, n).restype is C.c_size_t, n
    assert re.search(r"#define\s+SDRHIP_EINVAL\s+\(?%d\)?" % EINVAL, src) or "SDRHIP_EINVAL = %d" % EINVAL in src


def test_header_cites_the_constructors():
    h = _header()
    at = h.index("int sdrhip_decimators_reset_streams")
    comment = h[h.rindex("/*", 0, at):at]
    for cite in ("Decimators.h:56-70", "Interpolators.h:47-52", "UDPSinkFEC.cpp", "SDRdaemonFECBuffer.cpp", "MetaDataFEC::init()"):
        assert cite in comment, cite
    for word in ("never synchronises", "reads nothing back", "NULL = every stream", "an all-zero mask launches nothing",
                 "launches exactly what it launched before they existed"):
        assert word in comment, word


def test_null_handle_is_einval(built):
    lib = built.lib()
    mask = (C.c_uint8 * 4)(1, 0, 0, 1)
    for n in RESET:
        assert getattr(lib, n)(None, mask) == EINVAL, n
        assert b"NULL" in lib.sdrhip_last_error(), n
        assert getattr(lib, n)(None, None) == EINVAL, n
    blob = C.create_string_buffer(1 << 18)
    for n in MOVE:
        assert getattr(lib, n)(None, 0, blob, len(blob)) == EINVAL, n
        assert b"NULL" in lib.sdrhip_last_error(), n
    for n in SIZES:
        assert getattr(lib, n)(None) == 0, n


def test_python_surface(built):
    import sdrdaemon_amd as sd

    for cls in (sd.Decimators, sd.Interpolators, sd.FECBufferBank):
        p = inspect.signature(cls.reset).parameters
        assert list(p)[1:] == ["streams"] and p["streams"].default is None, cls
    for cls in (sd.RxPipe, sd.TxPipe):
        p = inspect.signature(cls.reset_streams).parameters
        assert list(p)[1:] == ["streams"] and p["streams"].default is None, cls
        assert list(inspect.signature(cls.export_stream).parameters)[1:] == ["stream"], cls
        assert list(inspect.signature(cls.import_stream).parameters)[1:] == ["stream", "blob"], cls
    from sdrdaemon_amd import engine

    assert engine._stream_mask(None, 3) is None
    assert list(engine._stream_mask([2, 0], 3)) == [1, 0, 1] and list(engine._stream_mask([], 2)) == [0, 0]
    with pytest.raises(ValueError):
        engine._stream_mask([3], 3)


def test_header_compiles_as_c99_and_cxx11(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "sdrhip.h"\n'
                 "typedef int (*reset_fn)(sdrhip_rx *, const uint8_t *);\n"
                 "int main(void){reset_fn f = sdrhip_rx_reset_streams; return f == 0;}\n")
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(c), "-c", "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", "-I", inc, str(c), "-c", "-o", str(tmp_path / "t2.o")], check=True)
