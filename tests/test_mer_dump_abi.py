"""CPU-side checks of the device text dump's C-ABI (include/kmernator_amd.h, kmr_dump_text*): the six entry points are exported and
bound, a NULL handle or output pointer is KMR_ERR_INVALID_ARG before anything is touched, and the additions left
KMR_ABI_VERSION at 1."""
import ctypes as C

import kmernator_amd as ka
from kmernator_amd import _lib

SYMBOLS = ["kmr_dump_text_size", "kmr_dump_text", "kmr_text_info", "kmr_text_copy", "kmr_text_device_ptr", "kmr_text_free"]
INVALID_ARG = -1
U64_MAX = (1 << 64) - 1


def test_the_six_symbols_are_exported_and_bound():
    lib = ka.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert lib.kmr_abi_version() == 1


def test_null_handle_or_output_is_invalid_arg():
    lib = ka.load()
    kept, nbytes, out, ptr = C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_void_p()
    for kind in (0, 1):
        assert lib.kmr_dump_text_size(None, kind, 2, 0, U64_MAX, C.byref(kept), C.byref(nbytes)) == INVALID_ARG
        assert lib.kmr_dump_text(None, kind, 2, 0, U64_MAX, C.byref(out)) == INVALID_ARG
        assert not out.value
    # a NULL output pointer is refused before the handle is looked at: any non-NULL address will do for it
    standin = C.create_string_buffer(64)
    h = C.cast(standin, C.c_void_p)
    assert lib.kmr_dump_text(h, 0, 2, 0, U64_MAX, None) == INVALID_ARG
    assert lib.kmr_dump_text_size(h, 0, 2, 0, U64_MAX, None, C.byref(nbytes)) == INVALID_ARG
    assert lib.kmr_dump_text_size(h, 0, 2, 0, U64_MAX, C.byref(kept), None) == INVALID_ARG
    assert lib.kmr_text_info(None, C.byref(kept), C.byref(nbytes)) == INVALID_ARG
    assert lib.kmr_text_copy(None, standin, 64) == INVALID_ARG
    assert lib.kmr_text_device_ptr(None, C.byref(ptr)) == INVALID_ARG
    assert lib.kmr_text_device_ptr(h, None) == INVALID_ARG
    lib.kmr_text_free(None)          # a no-op, as free(NULL)


def test_python_mirror_has_the_text_methods():
    for name in ("dumpCountsText", "dumpGraphsText", "dumpTextSize", "dumpCounts", "dumpGraphs"):
        assert callable(getattr(ka.KmerSpectrum, name)), name
    for name in ("numpy", "device_tensor", "close"):
        assert callable(getattr(ka.DumpText, name)), name
