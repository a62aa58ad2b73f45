"""CPU-side checks of the substitution-matrix entry points: the five symbols are exported, listed in EXPORTS and declared in the
header, and none of them does anything without a context."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg

NAMES = ("pwa_align_subst_batch", "pwa_align_subst_batch_cigar", "pwa_subst_batch_create", "pwa_scores_subst", "pwa_align_subst_last_stats")
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
    code = (C.c_uint8 * 256)()
    submat = (C.c_int32 * 1)(1)
    pa, pb = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1)
    sc = (C.c_int32 * 1)()
    ops = C.create_string_buffer(16)
    ooff, nops = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)()
    coff, moff = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    cg, md = C.create_string_buffer(64), C.create_string_buffer(64)
    h = C.c_void_p()
    head = (None, 0, code, 1, submat, -2, -1, blob, off, 2, pa, pb, 1)
    assert L.pwa_align_subst_batch(*head, sc, ops, ooff, nops, None, None) == PWA_E_INVALID
    assert L.pwa_align_subst_batch_cigar(*head, sc, cg, 64, coff, md, 64, moff, None, None, None) == PWA_E_INVALID
    assert L.pwa_subst_batch_create(*head, 0, C.byref(h)) == PWA_E_INVALID
    assert not h.value
    assert L.pwa_scores_subst(*head, sc, None, None) == PWA_E_INVALID
    f, w, b = C.c_float(0), C.c_float(0), C.c_uint64(0)
    assert L.pwa_align_subst_last_stats(None, C.byref(f), C.byref(w), C.byref(b)) == PWA_E_INVALID
