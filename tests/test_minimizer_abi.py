"""The minimizer calls at the C boundary, without a GPU: exported, listed, declared, refusing null pointers and k and w out of range, and
the host-only plan (pwa_mm_plan: every validation code with its first offending read, the limits given through offsets alone, the
range counts) against minimizer_oracle.py."""
import ctypes as C
import os
import random
import re

import pytest

import minimizer_oracle as MO
from conftest import ROOT, load_pkg

NAMES = ["pwa_mm_create", "pwa_mm_fetch", "pwa_mm_last_stats", "pwa_mm_sketch", "pwa_mm_plan", "pwa_mm_seed", "pwa_mm_seed_fetch",
         "pwa_mm_seed_last_stats"]
INVALID, CAPACITY = -1, -5
NO_READ = 0xffffffff


def plan(n_min, offsets, k, max_occ, budget=0):
    """pwa_mm_plan on raw offsets -> (code, bad read or None, k-mers, ranges)"""
    L = load_pkg().lib()
    off = (C.c_uint64 * max(len(offsets), 1))(*offsets)
    bad, ns, nr = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
    rc = L.pwa_mm_plan(n_min, off, max(len(offsets) - 1, 0), k, max_occ, budget, C.byref(bad), C.byref(ns), C.byref(nr))
    return rc, None if bad.value == NO_READ else bad.value, ns.value, nr.value


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    block = hdr[hdr.index("Minimizer sketches, a minimizer index, seeding against it"):hdr.index("typedef struct pwa_mm_index")]
    for word in ("uppercase only", "lowercase, 'N', NUL, >= 0x80", "1 <= k <= 31", "the first symbol most significant", "key = (~key + (key << 21)) & mask",
                 "key ^= key >> 28", "key = (key + (key << 31)) & mask", "bijection on 2k bits", "+infinity", "1 <= w <= 128", "one window, [0, K)",
                 "the leftmost one among equals", "With w = 1 the sketch is every valid k-mer", "h(j) > h(p) for all j < p in W",
                 "h(j) >= h(p) for all j > p in W", "in ascending (hash, t)", "n < k gives a valid, empty index", "more than max_occ hits",
                 "counted among the text's minimizers", "in ascending (t, q)", "(len - k + 1) x min(max_occ, n_min)", "a total of 2^32 k-mers or more",
                 "PWA_OCC_CHUNK_HITS", "A range without a k-mer is not run or counted", "min_off_out complete", "the total k-mer count always suffices",
                 "Any pointer may be NULL", "fault word"):
        assert word in block, word
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert hasattr(L, "pwa_mm_destroy") and "pwa_mm_destroy" in pkg.EXPORTS and re.search(r"\bvoid\s+pwa_mm_destroy\s*\(", hdr)
    assert callable(pkg.minimizer_plan) and callable(pkg.Context.sketch)
    for method in ("seed", "entries", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.MinimizerIndex, method)), method


def test_null_pointers_are_invalid():
    L = load_pkg().lib()
    off, out = (C.c_uint64 * 2)(0, 4), (C.c_uint64 * 2)()
    t, q, h = (C.c_uint32 * 4)(), (C.c_uint32 * 4)(), (C.c_uint64 * 4)()
    ix = C.c_void_p()
    assert L.pwa_mm_create(None, b"ACGT", 4, 2, 2, C.byref(ix)) == INVALID
    assert L.pwa_mm_sketch(None, b"ACGT", off, 1, 2, 2, out, t, h, 4, None) == INVALID
    assert L.pwa_mm_fetch(None, h, t, 4) == INVALID and L.pwa_mm_last_stats(None, None, None) == INVALID
    assert L.pwa_mm_seed(None, b"ACGT", off, 1, 64, out) == INVALID and L.pwa_mm_seed(None, None, None, 0, 64, None) == INVALID
    assert L.pwa_mm_seed_fetch(None, t, q, 4) == INVALID and L.pwa_mm_seed_fetch(None, None, None, 0) == INVALID
    assert L.pwa_mm_seed_last_stats(None, None, None, None, None, None, None, None) == INVALID
    L.pwa_mm_destroy(None)                                                     # harmless
    # the plan: read_off is its one required pointer; the three outputs may each be NULL
    bad, ns, nr = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
    assert L.pwa_mm_plan(100, None, 1, 2, 64, 0, C.byref(bad), C.byref(ns), C.byref(nr)) == INVALID
    assert (bad.value, ns.value, nr.value) == (NO_READ, 0, 0)
    assert L.pwa_mm_plan(100, off, 1, 2, 64, 0, None, None, None) == 0
    assert L.pwa_mm_plan(100, off, 1, 2, 64, 0, None, C.byref(ns), None) == 0 and ns.value == 3
    assert L.pwa_mm_plan(100, None, 0, 2, 64, 0, C.byref(bad), C.byref(ns), C.byref(nr)) == 0        # the empty list
    assert (bad.value, ns.value, nr.value) == (NO_READ, 0, 0)
    assert L.pwa_mm_plan(100, None, 0, 2, 0, 0, None, None, None) == INVALID                           # ... with max_occ = 0


def test_k_and_w_at_their_limits():
    pkg = load_pkg()
    for k, code in [(0, INVALID), (1, 0), (31, 0), (32, INVALID), (0xffffffff, INVALID)]:
        # a parameter comes before a bad read
        assert plan(100, [0, 40], k, 64)[0] == code and (code == 0 or plan(100, [0, 10, 5], k, 64) == (INVALID, None, 0, 0)), k
        assert MO.validate(100, [0, 40], k, 64)[0] == code
    assert plan(100, [0, 40], 31, 64)[2] == 10 and plan(100, [0, 40], 5, 0) == (INVALID, None, 0, 0)
    # the calls with a context check k and w before they touch it -- but after a null context; the Python layer checks them itself
    for k, w in [(0, 5), (32, 5), (5, 0), (5, 129)]:
        with pytest.raises(ValueError):
            pkg.Context.sketch(None, [b"ACGT"], k, w)
        with pytest.raises(ValueError):
            pkg.MinimizerIndex(None, b"ACGT", k, w)
    assert pkg.minimizer_plan(100, [40], 31) == dict(code=0, bad_read=None, slots=10, ranges=1)
    assert pkg.minimizer_plan(100, [40], 32)["code"] == INVALID


def test_plan_reports_every_code_with_the_first_offending_read():
    top = 1 << 31
    cases = [
        (100, [0, 10, 5, 30], 3, 64),                          # read_off decreases at read 1
        (100, [0, 10, 5, 5 + top], 3, 64),                     # ... and that comes before the long read 2
        (100, [0, top, 5], 3, 64),                             # the long read 0 before the decrease at read 1
        (100, [0, 10, 10 + top - 1], 3, 1),                    # a read of 2^31 - 1 bytes
        (100, [0, 10, 10 + top], 3, 1),                        # ... of 2^31
        (100, [5, 5, 5 + top, 7 + top], 3, 1),                 # offsets need not start at 0
        (100, [0, 1, 2, 2 + top, 1], 3, 1),                    # read 2 before the decrease at read 3
        (1 << 20, [0, 8, 8 + (1 << 30)], 1, 4),                # worst-case hits 2^30 * 4 = 2^32 at read 1
        (1 << 20, [0, 8, 8 + (1 << 30) - 1], 1, 4),            # ... 2^32 - 4
        (3, [0, 8, 8 + (1 << 30)], 1, 4),                      # the index has 3 entries: 3 * 2^30
        (2, [0, 8 + (1 << 30)], 1, 0xffffffff),                # 2 * (2^30 + 8)
        (1 << 20, [0, top - 1], 1, 2),                         # (2^31 - 1) * 2 = 2^32 - 2
        (1 << 20, [0, top - 1], 1, 3),
        (0xffffffff, [0, 1], 1, 0xffffffff),                   # one k-mer of 2^32 - 1 hits at the worst
        (1 << 40, [0, 1], 1, 0xffffffff),                      # max_occ caps it below 2^32 whatever n_min
        (1 << 40, [0, 2], 1, 0xffffffff),                      # two such k-mers: 2^33 - 2
        (0, [0, 50], 5, 64),                                   # an empty index
        (0, [0, 500, 400], 5, 64),                             # ... still validated
    ]
    codes = set()
    for n_min, off, k, max_occ in cases:
        got = plan(n_min, off, k, max_occ)
        want = MO.validate(n_min, off, k, max_occ)
        assert got[:3] == want, (n_min, off, k, max_occ)
        if want[0]:
            assert got[3] == 0
        codes.add((want[0], want[1]))
    assert {(0, None), (INVALID, 1), (CAPACITY, 0), (CAPACITY, 1), (CAPACITY, 2)} <= codes
    assert plan(100, [0, 10, 10 + top - 1], 3, 1)[:2] == (0, None) and plan(100, [0, 10, 10 + top], 3, 1)[:2] == (CAPACITY, 1)
    assert plan(1 << 20, [0, top - 1], 1, 2)[:3] == (0, None, top - 1) and plan(1 << 20, [0, top - 1], 1, 3)[:2] == (CAPACITY, 0)
    # worst-case hits of exactly 2^32 - 1 = 65535 * 65537 and of exactly 2^32 = 65536 * 65536, the second factor once max_occ, once n_min
    assert plan(1 << 20, [0, 65535], 1, 65537)[:2] == (0, None) and MO.worst_hits(65535, 1 << 20, 1, 65537) == (1 << 32) - 1
    assert plan(65537, [0, 65535], 1, 1 << 20)[:2] == (0, None) and MO.worst_hits(65535, 65537, 1, 1 << 20) == (1 << 32) - 1
    assert plan(1 << 20, [4, 4, 4 + 65536], 1, 65536)[:2] == (CAPACITY, 1) and MO.worst_hits(65536, 1 << 20, 1, 65536) == 1 << 32
    assert plan(65536, [4, 4, 4 + 65536], 1, 1 << 20)[:2] == (CAPACITY, 1)
    # the total: reads below 2^31 bytes on a one-entry index, k = 1
    big = top - 1
    assert plan(1, [0, big, 2 * big, 2 * big + 1], 1, 64) == (0, None, (1 << 32) - 1, 3)
    assert plan(1, [0, big, 2 * big, 2 * big + 2], 1, 64) == (CAPACITY, None, 0, 0)
    assert plan(1, [0, big, 2 * big, 2 * big + 2, 5], 1, 64)[:2] == (INVALID, 3)                  # a bad read comes before the total


def test_range_counts_against_the_greedy_cut():
    pkg = load_pkg()
    rng = random.Random(3)
    n_min, k, max_occ = 900, 11, 8
    lens = [rng.choice([0, 0, 5, 11, 12, 40, 300, 1500]) for _ in range(60)] + [0, 3, 0]
    worst = [MO.worst_hits(ln, n_min, k, max_occ) for ln in lens]
    total, longest = sum(worst), max(worst)
    assert longest == 1490 * 8
    seen = set()
    for budget in (0, total, total - 1, total // 2, total // 7, longest, longest - 1, 1000, 129, 128, 127, 8, 7, 1):
        got = pkg.minimizer_plan(n_min, lens, k, max_occ, budget=budget)
        want = MO.ranges(n_min, lens, k, max_occ, budget)
        assert got["code"] == 0 and got["ranges"] == len(want), budget
        seen.add(len(want))
    assert 1 in seen and len([w for w in worst if w]) in seen and len(seen) >= 6
    # an index smaller than max_occ: its size is the second factor
    for budget in (0, 5000, 100, 1):
        assert pkg.minimizer_plan(3, lens, k, max_occ, budget=budget)["ranges"] == len(MO.ranges(3, lens, k, max_occ, budget))
    assert MO.worst_hits(1500, 3, k, max_occ) == 1490 * 3
    assert pkg.minimizer_plan(n_min, [0, 3, 10], k, budget=1)["ranges"] == 0                     # no k-mer
    assert pkg.minimizer_plan(0, lens, k, budget=1) == dict(code=0, bad_read=None, slots=sum(max(ln - k + 1, 0) for ln in lens), ranges=0)   # an empty index
    assert pkg.minimizer_plan(n_min, [], k, budget=1) == dict(code=0, bad_read=None, slots=0, ranges=0)
