"""The banded extension calls at the C boundary, without a GPU: exported, listed, declared, and refusing a null context."""
import ctypes as C
import os
import re

from conftest import ROOT, load_pkg

NAMES = ["pwa_extend_banded_batch", "pwa_extend_banded_batch_cigar", "pwa_scores_extend_banded", "pwa_extend_banded_last_stats"]


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
    ops, nops, ends = C.create_string_buffer(8), (C.c_uint64 * 1)(), (C.c_uint64 * 2)()
    assert L.pwa_extend_banded_batch(None, 1, -1, -2, -1, 10, b"", one64, 1, one32, one32, 1, sc, ops, one64, nops, ends, one32, band, band) == -1
    assert L.pwa_extend_banded_batch_cigar(None, 1, -1, -2, -1, 10, b"", one64, 1, one32, one32, 1, sc, ops, 8, one64, ops, 8, one64, ends, one32,
                                           None, band, band) == -1
    assert L.pwa_scores_extend_banded(None, 1, -1, -2, -1, 10, b"", one64, 1, one32, one32, 1, sc, one32, one32, one32, band, band) == -1
    assert L.pwa_scores_extend_banded(None, 1, -1, -2, -1, -1, b"", one64, 1, one32, one32, 1, sc, None, None, None, band, band) == -1
    assert L.pwa_extend_banded_last_stats(None, None, None, None) == -1
