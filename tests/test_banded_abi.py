"""The banded calls at the C boundary, without a GPU: exported, listed, declared, and refusing a null context."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg

NAMES = ["pwa_align_banded_batch", "pwa_align_banded_batch_cigar", "pwa_align_banded_last_stats"]


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_null_context_is_invalid():
    L = load_pkg().lib()
    one32, one64 = (C.c_uint32 * 1)(0), (C.c_uint64 * 2)(0, 0)
    sc, band = (C.c_int32 * 1)(), (C.c_int32 * 1)(0)
    ops = C.create_string_buffer(16)
    assert L.pwa_align_banded_batch(None, 0, 1, -1, -2, -1, b"", one64, 1, one32, one32, 1, sc, ops, one64, one64, None, None, band, band) == -1
    assert L.pwa_align_banded_batch_cigar(None, 0, 1, -1, -2, -1, b"", one64, 1, one32, one32, 1, sc, ops, 16, one64, ops, 16, one64, None, None,
                                          None, band, band) == -1
    assert L.pwa_align_banded_last_stats(None, None, None, None) == -1


def test_band_around():
    pkg = load_pkg()
    assert pkg.band_around(10, 14, 3) == (-3, 7)
    assert pkg.band_around(14, 10, 3) == (-7, 3)
    assert pkg.band_around(5, 5, 0) == (0, 0)
    assert pkg.band_around(100, 4000, 60, diag=1234) == (1174, 1294)
