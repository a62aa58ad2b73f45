"""The banded substitution-matrix calls at the C boundary, without a GPU: exported, listed, declared, and refusing a null context."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg

NAMES = ["pwa_align_banded_subst_batch", "pwa_align_banded_subst_batch_cigar", "pwa_scores_banded_subst"]


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("align_banded_subst_batch", "align_banded_subst_batch_cigar", "scores_banded_subst"):
        assert callable(getattr(pkg.Context, name)), name


def test_null_context_is_invalid():
    L = load_pkg().lib()
    one32, one64 = (C.c_uint32 * 1)(0), (C.c_uint64 * 2)(0, 0)
    sc, band = (C.c_int32 * 1)(), (C.c_int32 * 1)(0)
    code, submat = (C.c_uint8 * 256)(), (C.c_int32 * 1)(1)
    ops = C.create_string_buffer(8)
    head = (None, 0, code, 1, submat, -2, -1, b"", one64, 1, one32, one32, 1)
    assert L.pwa_align_banded_subst_batch(*head, sc, ops, one64, one64, None, None, band, band) == -1
    assert L.pwa_align_banded_subst_batch_cigar(*head, sc, ops, 8, one64, ops, 8, one64, None, None, None, band, band) == -1
    assert L.pwa_scores_banded_subst(*head, sc, one32, one32, band, band) == -1
    assert L.pwa_scores_banded_subst(*head, sc, None, None, band, band) == -1
