"""CPU-side checks of the affine-gap (gotoh) score entry points: both symbols are exported and declared in the header, and neither
does anything without a context."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg

NAMES = ("pwa_gotoh_batch_create", "pwa_scores_gotoh")
PWA_E_INVALID = -1


def test_symbols_are_exported_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name


def test_null_context_is_invalid():
    pkg = load_pkg()
    L = pkg.lib()
    blob, off, _ = pkg.pack_sequences([b"ACGT", b"ACGTT"])
    pa, pb = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1)
    sc = (C.c_int32 * 1)()
    h = C.c_void_p()
    assert L.pwa_gotoh_batch_create(None, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 1, 0, C.byref(h)) == PWA_E_INVALID
    assert not h.value
    assert L.pwa_scores_gotoh(None, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 1, sc, None, None) == PWA_E_INVALID
