"""pwa_approx_starts / pwa_approx_starts_last_stats / pwa_approx_minima at the C boundary, without a GPU: exported, listed, declared,
refusing null arguments, and the host-only minima call against the oracle and its error cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import approx_locate_oracle as LO
import approx_oracle as AO
from conftest import ROOT, load_pkg

NAMES = ["pwa_approx_starts", "pwa_approx_starts_last_stats", "pwa_approx_minima"]
INVALID = -1


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    assert re.search(r"#define\s+PWA_APPROX_NO_START\s+0xffffffffu", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for method in ("starts_approx", "locate_approx", "align_approx"):
        assert callable(getattr(pkg.Context, method))
    assert callable(pkg.approx_minima)
    assert pkg.APPROX_NO_START == 0xffffffff


def test_null_context_and_null_pointers_are_invalid():
    L = load_pkg().lib()
    off, occ_off, occ, out = (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 2)(0, 1), (C.c_uint64 * 1)(1 << 32), (C.c_uint32 * 1)()
    assert L.pwa_approx_starts(None, b"A", 1, b"A", off, 1, occ_off, occ, out) == INVALID
    assert L.pwa_approx_starts_last_stats(None, None, None, None) == INVALID
    m, k = (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(0)
    assert L.pwa_approx_minima(1, m, k, 1, None, occ) == INVALID
    assert L.pwa_approx_minima(1, m, k, 1, occ_off, None) == INVALID
    assert L.pwa_approx_minima(1, None, k, 1, occ_off, occ) == INVALID
    assert L.pwa_approx_minima(1, m, None, 1, occ_off, occ) == INVALID
    assert L.pwa_approx_minima(1, m, k, 1, occ_off, occ) == 0 and list(occ_off) == [0, 1]   # "A" in "A": kept


def minima(pkg, hits, lens, ks, n):
    return pkg.approx_minima(hits, lens, ks, n)


def test_minima_of_ragged_lists_against_the_rows():
    pkg = load_pkg()
    rng = np.random.default_rng(31)
    kept = 0
    for _ in range(60):
        alphabet = b"ACGT"[:int(rng.integers(1, 5))]
        n = int(rng.integers(1, 300))
        text = AO.random_seq(rng, n, alphabet)
        pats = [AO.random_seq(rng, int(rng.integers(1, 40)), alphabet) for _ in range(int(rng.integers(1, 7)))]
        pats.append(b"N" * 5)   # a pattern without a hit at small k
        ks = [int(rng.choice([0, 1, len(p) // 4, len(p) - 1, len(p), len(p) + 3])) for p in pats]
        ks[-1] = 1
        rows = [AO.last_row(p, text) for p in pats]
        hits = [AO.hits(p, text, k) for p, k in zip(pats, ks)]
        assert hits[-1] == []
        got = minima(pkg, hits, [len(p) for p in pats], ks, n)
        assert got == [LO.minima_from_row(r, k) for r, k in zip(rows, ks)]
        kept += sum(len(g) for g in got)
    assert kept > 100


def test_minima_corner_lists():
    pkg = load_pkg()
    # no patterns; patterns with empty lists only
    assert minima(pkg, [], [], [], 10) == []
    assert minima(pkg, [[], []], [3, 4], [1, 9], 10) == [[], []]
    # a single hit: between two columns without one
    assert minima(pkg, [[(5, 1)]], [4], [1], 10) == [[(5, 1)]]
    # a plateau from the first column: c(0) = m = 2 = c(1) = c(2), then a descent
    assert minima(pkg, [[(1, 2), (2, 2), (3, 1), (4, 2)]], [2], [2], 4) == [[(3, 1)]]
    # ... and one column 1 that does descend from c(0)
    assert minima(pkg, [[(1, 1), (2, 2)]], [2], [2], 2) == [[(1, 1)]]
    # a plateau to n: the text end is a rise; its leftmost end is kept
    assert minima(pkg, [[(7, 0), (8, 0), (9, 0), (10, 0)]], [3], [0], 10) == [[(7, 0)]]
    # a plateau left by a descent is not kept, the one below it is
    assert minima(pkg, [[(3, 2), (4, 2), (5, 1), (6, 1)]], [5], [2], 9) == [[(5, 1)]]
    # k >= m: every end is a hit (AB against AAAA...: D = 1 at every end, one plateau entered from c(0) = 2 and ended by the text)
    row = AO.last_row(b"AB", b"A" * 30)
    hits = AO.hits(b"AB", b"A" * 30, 5)
    assert len(hits) == 30 and minima(pkg, [hits], [2], [5], 30) == [LO.minima_from_row(row, 5)] == [[(1, 1)]]
    # the all-A text against an all-A pattern: every end is a hit at k = m, the row descends to 0 and stays
    p, t = b"A" * 6, b"A" * 40
    hits = AO.hits(p, t, 6)
    assert len(hits) == 40
    assert minima(pkg, [hits, hits], [6, 6], [6, 9], 40) == [[(6, 0)]] * 2 == [LO.minima_from_row(AO.last_row(p, t), 6)] * 2


def raw_minima(n, lens, ks, occ_off, occ):
    L = load_pkg().lib()
    n_pat = len(lens)
    a = (C.c_uint64 * len(occ_off))(*occ_off)
    b = (C.c_uint64 * max(len(occ), 1))(*[e << 32 | d for e, d in occ])
    rc = L.pwa_approx_minima(n, (C.c_uint32 * n_pat)(*lens), (C.c_uint32 * n_pat)(*ks), n_pat, a, b)
    return rc, list(a), [(x >> 32, x & 0xffffffff) for x in b][:len(occ)]


def test_minima_invalid_lists_are_refused_and_left_alone():
    good = [(2, 1), (3, 0), (9, 1)]
    assert raw_minima(10, [4, 4], [1, 1], [0, 3, 3], good) == (0, [0, 2, 2], [(3, 0), (9, 1), (9, 1)])
    for bad in ([0, 3, 2],):                                            # offsets not ascending
        assert raw_minima(10, [4, 4], [1, 1], bad, good) == (INVALID, bad, good)
    for occ in ([(3, 0), (2, 1), (9, 1)], [(2, 1), (2, 1), (9, 1)]):    # ends not strictly ascending within a pattern
        assert raw_minima(10, [4, 4], [1, 1], [0, 3, 3], occ) == (INVALID, [0, 3, 3], occ)
    for occ in ([(0, 1), (3, 0), (9, 1)], [(2, 1), (3, 0), (11, 1)]):   # an end outside 1 .. n
        assert raw_minima(10, [4, 4], [1, 1], [0, 3, 3], occ) == (INVALID, [0, 3, 3], occ)
    occ = [(2, 1), (3, 2), (9, 1)]                                      # dist > k' = min(max_dist, m)
    assert raw_minima(10, [4, 4], [1, 1], [0, 3, 3], occ) == (INVALID, [0, 3, 3], occ)
    assert raw_minima(10, [1, 4], [5, 1], [0, 1, 1], [(2, 2)]) == (INVALID, [0, 1, 1], [(2, 2)])   # ... k' is clipped to m = 1
    assert raw_minima(10, [4, 4], [1, 1], [0, 2, 3], good)[0] == 0     # ends ascend per pattern, not over the list
