"""The banded scores calls at the C boundary, without a GPU: exported, listed, declared, and refusing a null context."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg

NAMES = ["pwa_scores_banded", "pwa_scores_banded_last_stats"]


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
    assert L.pwa_scores_banded(None, 0, 1, -1, -2, -1, b"", one64, 1, one32, one32, 1, sc, one32, one32, band, band) == -1
    assert L.pwa_scores_banded(None, 0, 1, -1, -2, -1, b"", one64, 1, one32, one32, 1, sc, None, None, band, band) == -1
    assert L.pwa_scores_banded_last_stats(None, None, None) == -1
