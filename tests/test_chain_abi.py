"""The chaining calls at the C boundary, without a GPU: exported, listed, declared, refusing a null context and null pointers, and the
host-only plan (pwa_chain_plan: every validation code with its first offending read, the parameter limits, the range counts) against
chain_oracle.py."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import chain_oracle as CO
from conftest import ROOT, load_pkg

NAMES = ["pwa_chain_plan", "pwa_chain_anchors", "pwa_chain_last_stats"]
INVALID, CAPACITY = -1, -5
GOOD = [(5, 5, 3), (9, 9, 3)]


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    block = hdr[hdr.index("Collinear chaining of anchors"):hdr.index("int pwa_chain_plan")]
    for word in ("dx = x_i - x_j, dy = y_i - y_j, dd = |dx - dy|", "0 < dx <= max_dist, 0 < dy <= max_dist and dd <= bandwidth",
                 "cand(j) = f(j) + min(len_i, dx, dy) - beta(dd)", "((gap_scale * dd) >> 8) + (floor(log2 dd) >> 1)", "f(i) = max(len_i, max_j cand(j))",
                 "the largest j among the admissible j of maximal cand", "the smallest index with maximal f", "no skip heuristic",
                 "lookback H 1 .. 512, max_dist 1 .. 2^30, bandwidth 0 .. 2^20, gap_scale 0 .. 1024", "(q_b, y_e, t_b,", "PWA_RANGE_BYTES"):
        assert word in block, word
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    for method in ("chain", "seed", "map_reads"):
        assert callable(getattr(pkg.Context, method))
    assert callable(pkg.chain_plan) and callable(pkg.revcomp)


def test_revcomp():
    pkg = load_pkg()
    assert pkg.revcomp(b"ACGTacgtNn-x") == b"x-nNacgtACGT"
    assert pkg.revcomp("AAC") == b"GTT" and pkg.revcomp(b"") == b""
    assert CO.revcomp(b"ACGTacgtNn-x") == pkg.revcomp(b"ACGTacgtNn-x")


def test_null_context_and_null_pointers_are_invalid():
    L = load_pkg().lib()
    t, q, ln, off = (C.c_uint32 * 2)(5, 9), (C.c_uint32 * 2)(5, 9), (C.c_uint32 * 2)(3, 3), (C.c_uint64 * 2)(0, 2)
    sc, cnt, last, span, diag = (C.c_int32 * 1)(), (C.c_uint32 * 1)(), (C.c_uint32 * 1)(), (C.c_uint32 * 4)(), (C.c_int32 * 2)()
    full = [None, t, q, ln, off, 1, 64, 5000, 500, 38, sc, cnt, last, span, diag, None, None]
    assert L.pwa_chain_anchors(*full) == INVALID
    for at in (1, 2, 3, 4, 10, 11, 12, 13, 14):   # still the null context's answer, whatever else is missing
        args = list(full)
        args[at] = None
        assert L.pwa_chain_anchors(*args) == INVALID
    assert L.pwa_chain_last_stats(None, None, None, None) == INVALID
    bad, nr = C.c_uint32(7), C.c_uint64(7)
    for at in range(4):
        args = [t, q, ln, off, 1, 64, 5000, 500, 38, 0, C.byref(bad), C.byref(nr)]
        args[at] = None
        assert L.pwa_chain_plan(*args) == INVALID
        assert bad.value == 0xffffffff and nr.value == 0
    assert L.pwa_chain_plan(t, q, ln, off, 1, 64, 5000, 500, 38, 0, None, None) == 0
    assert L.pwa_chain_plan(None, None, None, None, 0, 64, 5000, 500, 38, 0, C.byref(bad), C.byref(nr)) == 0   # the empty list
    assert nr.value == 0
    assert L.pwa_chain_plan(None, None, None, None, 0, 0, 5000, 500, 38, 0, None, None) == INVALID            # ... with a bad parameter


def test_plan_reports_every_code_with_the_first_offending_read():
    pkg = load_pkg()
    top = (1 << 31) - 1
    cases = [
        ([GOOD, [(5, 5, 0)]], INVALID, 1),                                  # a len of 0
        ([GOOD, GOOD, [(9, 9, 3), (5, 5, 3)]], INVALID, 2),                 # x decreases
        ([[(5, 9, 3), (5, 8, 3)]], INVALID, 0),                             # equal x, y decreases
        ([[(5, 8, 3), (5, 9, 3), (5, 9, 3)], [(4, 7, 4), (5, 9, 3)]], 0, None),   # equal anchors, equal ends: legal
        ([GOOD, [(top - 1, 0, 1)]], 0, None),                               # x = 2^31 - 1
        ([GOOD, [(top, 0, 1)]], CAPACITY, 1),                               # x = 2^31
        ([[(0, top - 1, 1)]], 0, None),
        ([[(0, top, 1)]], CAPACITY, 0),                                     # y = 2^31
        ([[], [(0, 0, 1 << 29), (1 << 29, 1 << 29, (1 << 29) - 1)]], 0, None),     # sum of len = 2^30 - 1
        ([[], [(0, 0, 1 << 29), (1 << 29, 1 << 29, 1 << 29)]], CAPACITY, 1),       # sum of len = 2^30
        ([[(5, 5, 0)], [(top, 0, 1)]], INVALID, 0),                         # two bad reads: the earlier one
        ([[(top, 0, 1)], [(5, 5, 0)]], CAPACITY, 0),
        ([[(9, 9, 3), (5, 5, 0)]], INVALID, 0),                             # inside a read, anchor by anchor: the len of 0 comes first
        ([[(1, 1, 1), (top, 0, 1), (0, 0, 0)]], CAPACITY, 0),
    ]
    for reads, code, bad in cases:
        got = pkg.chain_plan(reads)
        assert (got["code"], got["bad_read"]) == (code, bad), reads
        assert CO.validate(reads) == (code, bad), reads
        if code:
            assert got["ranges"] == 0


def test_plan_refuses_offsets_that_decrease_and_too_many_anchors():
    L = load_pkg().lib()
    bad, nr = C.c_uint32(0), C.c_uint64(0)
    t = (C.c_uint32 * 4)(1, 2, 3, 4)
    ln = (C.c_uint32 * 4)(1, 1, 1, 1)
    off = (C.c_uint64 * 4)(0, 2, 1, 4)
    assert L.pwa_chain_plan(t, t, ln, off, 3, 64, 5000, 500, 38, 0, C.byref(bad), C.byref(nr)) == INVALID and bad.value == 1
    # 2^24 anchors pass, 2^24 + 1 do not (a perfect diagonal of len 1: the sum of len stays below 2^30)
    n = (1 << 24) + 1
    d = np.arange(n, dtype=np.uint32)
    one = np.ones(n, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.pwa_chain_plan(p(d), p(d), p(one), (C.c_uint64 * 3)(0, 0, n - 1), 2, 64, 5000, 500, 38, 0, C.byref(bad), C.byref(nr)) == 0
    assert nr.value == 1
    assert L.pwa_chain_plan(p(d), p(d), p(one), (C.c_uint64 * 3)(0, 0, n), 2, 64, 5000, 500, 38, 0, C.byref(bad), C.byref(nr)) == CAPACITY
    assert bad.value == 1


@pytest.mark.parametrize("name, lo, hi", [("lookback", 1, 512), ("max_dist", 1, 1 << 30), ("bandwidth", 0, 1 << 20), ("gap_scale", 0, 1024)])
def test_parameters_at_and_past_each_limit(name, lo, hi):
    pkg = load_pkg()
    for v, ok in [(lo, True), (hi, True), (hi + 1, False), (0xffffffff, False)] + ([(lo - 1, False)] if lo else []):
        got = pkg.chain_plan([GOOD, [(5, 5, 0)]][:1 if ok else 2], **{name: v})   # a bad parameter comes before a bad read
        assert got["code"] == (0 if ok else INVALID), (name, v)
        assert got["bad_read"] is None
        assert CO.validate([GOOD], **{name: v})[0] == got["code"]


def test_range_counts_against_the_greedy_cut():
    pkg = load_pkg()
    rng = random.Random(3)
    counts = [rng.choice([0, 0, 1, 2, 5, 40, 300]) for _ in range(60)] + [0, 0, 0]
    reads = [[(10 + i, 10 + i, 1) for i in range(c)] for c in counts]
    total = sum(CO.ANCHOR_BYTES * c + CO.RECORD_BYTES for c in counts)
    seen = set()
    for budget in (0, total, total - 1, total // 2, total // 7, 6040, 6039, 840, 100, 60, 59, 40, 1):
        got = pkg.chain_plan(reads, budget=budget)
        want = CO.ranges(counts, budget)
        assert got["code"] == 0 and got["ranges"] == len(want), budget
        seen.add(len(want))
    assert 1 in seen and len([c for c in counts if c]) in seen and len(seen) >= 6
    assert pkg.chain_plan([[], [], []], budget=1)["ranges"] == 0
    assert pkg.chain_plan([], budget=1) == dict(code=0, bad_read=None, ranges=0)
