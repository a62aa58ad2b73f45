"""PWA_POISON without a GPU (include/pwalign.h): the counter's symbol and its NULL case.  The parser of the switch's value is checked
inside the library by pwa_selftest_host (test_abi.py); what the switch does to a call is test_gpu_poisoned_buffers.py."""
import ctypes as C

from conftest import load_pkg


def test_poison_stats_symbol_and_null_context():
    pkg = load_pkg()
    L = pkg.lib()
    assert "pwa_ctx_poison_stats" in pkg.EXPORTS
    fn = L.pwa_ctx_poison_stats
    assert fn.argtypes == [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    buffers, nbytes = C.c_uint64(7), C.c_uint64(9)
    assert fn(None, C.byref(buffers), C.byref(nbytes)) == -1   # PWA_E_INVALID
    assert (buffers.value, nbytes.value) == (7, 9)             # nothing is written for a NULL context
    assert fn(None, None, None) == -1
    assert hasattr(pkg.Context, "poison_stats")


def test_poison_parser_selftest():
    """pwa_selftest_host holds the parser's cases: decimal and 0x.. of 0 .. 255 parse, anything else is refused, unset is not an error"""
    L = load_pkg().lib()
    L.pwa_selftest_host.argtypes = [C.c_uint32]
    L.pwa_selftest_host.restype = C.c_int
    assert L.pwa_selftest_host(7) == 0
