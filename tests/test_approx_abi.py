"""The approximate-search calls at the C boundary, without a GPU: exported, listed, declared, refusing a null context, and the task
plan (pwa_approx_plan, host only) against its contract."""
import ctypes as C
import os
import re

import pytest

import approx_oracle as AO
from conftest import ROOT, load_pkg

NAMES = ["pwa_approx_find", "pwa_approx_occurrences", "pwa_approx_last_stats", "pwa_approx_plan"]
INVALID, CAPACITY = -1, -5


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for method in ("count_approx", "find_approx"):
        assert callable(getattr(pkg.Context, method))
    assert callable(pkg.approx_plan)


def test_null_context_and_null_pointers_are_invalid():
    L = load_pkg().lib()
    off, k = (C.c_uint64 * 2)(0, 1), (C.c_uint32 * 1)(0)
    cnt, occ_off, occ, need = (C.c_uint32 * 1)(), (C.c_uint64 * 2)(), (C.c_uint64 * 1)(), C.c_uint64(0)
    assert L.pwa_approx_find(None, b"A", 1, b"A", off, 1, k, cnt, None, None) == INVALID
    assert L.pwa_approx_occurrences(None, b"A", 1, b"A", off, 1, k, occ_off, occ, 1, C.byref(need)) == INVALID
    assert L.pwa_approx_last_stats(None, None, None, None, None) == INVALID
    nt = C.c_uint64(0)
    assert L.pwa_approx_plan(10, None, None, 1, 4, None, None, None, None, 0, C.byref(nt)) == INVALID
    assert L.pwa_approx_plan(10, k, k, 1, 4, None, None, None, None, 0, None) == INVALID
    one = (C.c_uint32 * 1)(3)
    assert L.pwa_approx_plan(10, one, k, 1, 0, None, None, None, None, 0, C.byref(nt)) == INVALID   # chunk 0
    assert L.pwa_approx_plan(10, k, k, 1, 4, None, None, None, None, 0, C.byref(nt)) == INVALID     # m = 0


def ragged(ms):
    """(m, k) for k in {0, 1, m-1, m, m+3} of every m"""
    return [(m, k) for m in ms for k in (0, 1, m - 1, m, m + 3)]


@pytest.mark.parametrize("chunk", [1, 64, 1000])
def test_plan_tiles_orders_and_warms_up(chunk):
    pkg = load_pkg()
    mk = ragged([1, 2, 17, 64, 150, 512])
    pat_len, max_dist = [m for m, _ in mk], [k for _, k in mk]
    for n in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7):
        tasks = pkg.approx_plan(n, pat_len, max_dist, chunk)
        assert tasks == AO.plan(n, pat_len, max_dist, chunk)
        assert [(q, lo) for q, _, lo, _ in tasks] == sorted((q, lo) for q, _, lo, _ in tasks)   # (pattern, lo) order
        for q, (m, k) in enumerate(mk):
            mine = [t for t in tasks if t[0] == q]
            at = 0
            for _, scan_lo, lo, hi in mine:   # the report ranges tile [0, n) in ascending order
                assert lo == at and lo < hi <= lo + chunk
                assert scan_lo <= max(0, lo - (m + min(k, m)))
                at = hi
            assert at == n


def test_plan_capacity_protocol():
    L = load_pkg().lib()
    pl, md = (C.c_uint32 * 2)(5, 9), (C.c_uint32 * 2)(1, 2)
    nt = C.c_uint64(0)
    assert L.pwa_approx_plan(100, pl, md, 2, 30, None, None, None, None, 0, C.byref(nt)) == CAPACITY
    assert nt.value == 8
    tp = (C.c_uint32 * 8)()
    ts, tl, th = ((C.c_uint64 * 8)() for _ in range(3))
    nt = C.c_uint64(0)
    assert L.pwa_approx_plan(100, pl, md, 2, 30, tp, ts, tl, th, 7, C.byref(nt)) == CAPACITY
    assert nt.value == 8 and list(th) == [0] * 8   # nothing written
    assert L.pwa_approx_plan(100, pl, md, 2, 30, tp, ts, tl, th, 8, C.byref(nt)) == 0
    assert nt.value == 8 and list(tp) == [0] * 4 + [1] * 4 and list(th[:4]) == [30, 60, 90, 100]
    assert L.pwa_approx_plan(0, pl, md, 2, 30, None, None, None, None, 0, C.byref(nt)) == 0 and nt.value == 0
    assert L.pwa_approx_plan(100, pl, md, 0, 30, None, None, None, None, 0, C.byref(nt)) == 0 and nt.value == 0
