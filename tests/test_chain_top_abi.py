"""The top-N chaining calls at the C boundary, without a GPU: exported, listed, declared, refusing a null context and null pointers,
the host-only plan (pwa_chain_top_plan: every validation code with its first offending read, each new parameter at and past both
limits, the range counts) against chain_top_oracle.py, and pwa_mapq against the oracle's."""
import ctypes as C
import os
import random
import re

import pytest

import chain_oracle as CO
import chain_top_oracle as TO
from conftest import ROOT, load_pkg

NAMES = ["pwa_chain_top_plan", "pwa_chain_top", "pwa_chain_top_last_stats", "pwa_mapq"]
INVALID, CAPACITY = -1, -5
GOOD = [(5, 5, 3), (9, 9, 3)]


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    assert hdr.index("Top-N chains of a read") > hdr.index("int pwa_chain_last_stats")
    block = hdr[hdr.index("Top-N chains of a read"):hdr.index("int pwa_chain_top_plan")]
    for word in ("max_chains N 1 .. 16, min_score 1 .. 2^30, min_count 1 .. 2^24, flags 0 or PWA_CHAIN_ROOTED", "descending f",
                 "smaller index first among equal f", "base = f(p), branch = p", "score = f(e) - base",
                 "score >= min_score and count >= min_count and (PWA_CHAIN_ROOTED is not set or branch = -1)",
                 "A dropped walk still claims its anchors", "min(60, (60 * (s1 - s2) * min(c1, 10)) div (10 * s1))", "s2 clamped to [0, s1]",
                 "48 per anchor", "40 * max_chains + 16 per read", "0xFFFFFFFF", "#define PWA_CHAIN_ROOTED 1u"):
        assert word in block, word
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    for method in ("chain_top", "map_reads"):
        assert callable(getattr(pkg.Context, method))
    assert callable(pkg.chain_top_plan) and callable(pkg.mapq) and pkg.CHAIN_ROOTED == TO.ROOTED == 1


def test_null_context_and_null_pointers_are_invalid():
    L = load_pkg().lib()
    t, q, ln, off = (C.c_uint32 * 2)(5, 9), (C.c_uint32 * 2)(5, 9), (C.c_uint32 * 2)(3, 3), (C.c_uint64 * 2)(0, 2)
    nch, sc, cnt, last, span, diag, br = ((C.c_uint32 * 1)(), (C.c_int32 * 2)(), (C.c_uint32 * 2)(), (C.c_uint32 * 2)(), (C.c_uint32 * 8)(),
                                          (C.c_int32 * 4)(), (C.c_int32 * 2)())
    full = [None, t, q, ln, off, 1, 64, 5000, 500, 38, 2, 1, 1, 0, nch, sc, cnt, last, span, diag, br, None, None, None, None]
    assert L.pwa_chain_top(*full) == INVALID
    for at in (1, 2, 3, 4, 14, 15, 16, 17, 18, 19, 20):   # still the null context's answer, whatever else is missing
        args = list(full)
        args[at] = None
        assert L.pwa_chain_top(*args) == INVALID
    assert L.pwa_chain_top_last_stats(None, None, None, None, None, None) == INVALID
    bad, nr = C.c_uint32(7), C.c_uint64(7)
    for at in range(4):
        args = [t, q, ln, off, 1, 64, 5000, 500, 38, 4, 40, 3, 0, 0, C.byref(bad), C.byref(nr)]
        args[at] = None
        assert L.pwa_chain_top_plan(*args) == INVALID
        assert bad.value == 0xffffffff and nr.value == 0
    assert L.pwa_chain_top_plan(t, q, ln, off, 1, 64, 5000, 500, 38, 4, 40, 3, 1, 0, None, None) == 0
    assert L.pwa_chain_top_plan(None, None, None, None, 0, 64, 5000, 500, 38, 4, 40, 3, 0, 0, C.byref(bad), C.byref(nr)) == 0   # the empty list
    assert nr.value == 0
    assert L.pwa_chain_top_plan(None, None, None, None, 0, 64, 5000, 500, 38, 0, 40, 3, 0, 0, None, None) == INVALID        # ... with a bad parameter
    assert L.pwa_chain_top_plan(None, None, None, None, 0, 0, 5000, 500, 38, 4, 40, 3, 0, 0, None, None) == INVALID


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
        ([[(0, top, 1)]], CAPACITY, 0),                                     # y = 2^31
        ([[], [(0, 0, 1 << 29), (1 << 29, 1 << 29, (1 << 29) - 1)]], 0, None),     # sum of len = 2^30 - 1
        ([[], [(0, 0, 1 << 29), (1 << 29, 1 << 29, 1 << 29)]], CAPACITY, 1),       # sum of len = 2^30
        ([[(5, 5, 0)], [(top, 0, 1)]], INVALID, 0),                         # two bad reads: the earlier one
        ([[(top, 0, 1)], [(5, 5, 0)]], CAPACITY, 0),
        ([[(9, 9, 3), (5, 5, 0)]], INVALID, 0),                             # inside a read, anchor by anchor: the len of 0 comes first
    ]
    for reads, code, bad in cases:
        got = pkg.chain_top_plan(reads)
        assert (got["code"], got["bad_read"]) == (code, bad), reads
        assert TO.validate(reads) == (code, bad), reads
        assert pkg.chain_plan(reads)["code"] == code
        if code:
            assert got["ranges"] == 0
    L = pkg.lib()
    bad, nr = C.c_uint32(0), C.c_uint64(0)
    t, ln, off = (C.c_uint32 * 4)(1, 2, 3, 4), (C.c_uint32 * 4)(1, 1, 1, 1), (C.c_uint64 * 4)(0, 2, 1, 4)
    assert L.pwa_chain_top_plan(t, t, ln, off, 3, 64, 5000, 500, 38, 4, 40, 3, 0, 0, C.byref(bad), C.byref(nr)) == INVALID and bad.value == 1


@pytest.mark.parametrize("name, lo, hi", [("max_chains", 1, 16), ("min_score", 1, 1 << 30), ("min_count", 1, 1 << 24), ("flags", 0, 1),
                                          ("lookback", 1, 512), ("max_dist", 1, 1 << 30), ("bandwidth", 0, 1 << 20), ("gap_scale", 0, 1024)])
def test_parameters_at_and_past_each_limit(name, lo, hi):
    pkg = load_pkg()
    for v, ok in [(lo, True), (hi, True), (hi + 1, False), (0xffffffff, False)] + ([(lo - 1, False)] if lo else []):
        got = pkg.chain_top_plan([GOOD, [(5, 5, 0)]][:1 if ok else 2], **{name: v})   # a bad parameter comes before a bad read
        assert got["code"] == (0 if ok else INVALID), (name, v)
        assert got["bad_read"] is None
        assert TO.validate([GOOD], **{name: v})[0] == got["code"]


def test_range_counts_against_the_greedy_cut():
    pkg = load_pkg()
    rng = random.Random(3)
    counts = [rng.choice([0, 0, 1, 2, 5, 40, 300]) for _ in range(60)] + [0, 0, 0]
    reads = [[(10 + i, 10 + i, 1) for i in range(c)] for c in counts]
    for N in (1, 4, 16):
        total = sum(TO.ANCHOR_BYTES * c + TO.read_bytes(N) for c in counts)
        one = TO.ANCHOR_BYTES * 300 + TO.read_bytes(N)
        seen = set()
        for budget in (0, total, total - 1, total // 2, total // 7, one, one - 1, 2 * one, 1000, TO.read_bytes(N) + 48, TO.read_bytes(N) + 47, 1):
            got = pkg.chain_top_plan(reads, max_chains=N, budget=budget)
            want = TO.ranges(counts, budget, N)
            assert got["code"] == 0 and got["ranges"] == len(want), (N, budget)
            seen.add(len(want))
        assert 1 in seen and len([c for c in counts if c]) in seen and len(seen) >= 6
    assert pkg.chain_top_plan([[], [], []], budget=1)["ranges"] == 0
    assert pkg.chain_top_plan([], budget=1) == dict(code=0, bad_read=None, ranges=0)
    # the two calls cut the same list differently: 20 and 40 bytes there, 48 and 40 N + 16 here
    fits = sum(CO.ANCHOR_BYTES * c + CO.RECORD_BYTES for c in counts)
    assert pkg.chain_plan(reads, budget=fits)["ranges"] == len(CO.ranges(counts, fits)) == 1 < pkg.chain_top_plan(reads, budget=fits)["ranges"]


def test_mapq():
    pkg = load_pkg()
    m = pkg.mapq
    assert m(100, 0, 10) == 60 and m(100, 100, 10) == 0 and m(100, 250, 10) == 0      # s2 = 0, s2 = s1, s2 > s1 (clamped)
    assert m(100, -7, 10) == 60                                                       # s2 < 0 (clamped)
    assert m(0, 0, 10) == 0 and m(-1, -5, 10) == 0 and m(-(1 << 31), 0, 10) == 0      # s1 <= 0
    assert [m(100, 0, c) for c in (0, 9, 10, 11)] == [0, 54, 60, 60]
    assert m(1 << 30, 0, 10) == 60 and m(1 << 30, 1, 10) == 59 and m(1 << 30, 1 << 29, 0xffffffff) == 30
    assert m(600, 592, 40) == 0 and m(600, 0, 40) == 60
    grid = [0, 1, 2, 3, 7, 10, 40, 99, 100, 101, 592, 600, 1 << 16, (1 << 30) - 1, 1 << 30]
    for s1 in [-5] + grid:
        for s2 in [-1] + grid:
            for c1 in (0, 1, 2, 3, 5, 9, 10, 11, 1 << 24):
                assert m(s1, s2, c1) == TO.mapq(s1, s2, c1), (s1, s2, c1)
