"""The substitution-matrix extension calls at the C boundary, without a GPU: exported, listed, declared with PWA_EXT_NO_PEND, reachable
from Python, and refusing a null context."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg

NAMES = ["pwa_extend_banded_subst_batch", "pwa_extend_banded_subst_batch_cigar", "pwa_scores_extend_banded_subst"]
METHODS = ["extend_banded_subst_batch", "extend_banded_subst_batch_cigar", "scores_extend_banded_subst", "extend_banded_stats"]


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"^#define\s+PWA_EXT_NO_PEND\s+INT32_MIN\b", code, flags=re.M)
    assert pkg.EXT_NO_PEND == -(1 << 31)
    for m in METHODS:
        assert callable(getattr(pkg.Context, m)), m


def test_null_context_is_invalid():
    L = load_pkg().lib()
    one32, one64 = (C.c_uint32 * 1)(0), (C.c_uint64 * 2)(0, 0)
    sc, band = (C.c_int32 * 1)(), (C.c_int32 * 1)(0)
    ops, nops, ends = C.create_string_buffer(8), (C.c_uint64 * 1)(), (C.c_uint64 * 2)()
    code, sub = (C.c_uint8 * 256)(), (C.c_int32 * 1)(1)
    head = (None, code, 1, sub, -2, -1, 10, b"", one64, 1, one32, one32, 1)
    assert L.pwa_extend_banded_subst_batch(*head, sc, ops, one64, nops, ends, one32, sc, one32, band, band) == -1
    assert L.pwa_extend_banded_subst_batch_cigar(*head, sc, ops, 8, one64, ops, 8, one64, ends, one32, sc, one32, None, band, band) == -1
    assert L.pwa_scores_extend_banded_subst(*head, sc, one32, one32, one32, sc, one32, band, band) == -1
    assert L.pwa_scores_extend_banded_subst(*head, sc, None, None, None, None, None, band, band) == -1
