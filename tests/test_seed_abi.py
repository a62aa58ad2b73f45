"""The seeding calls at the C boundary, without a GPU: exported, listed, declared, refusing a null index, and the host-only plan
(pwa_seed_plan: every validation code with its first offending read, the limits given through offsets alone, the slot counts, the range
counts) against seed_oracle.py."""
import ctypes as C
import os
import random
import re

import pytest

import seed_oracle as SO
from conftest import ROOT, load_pkg

NAMES = ["pwa_seed_plan", "pwa_sa_seed", "pwa_sa_seed_fetch", "pwa_sa_seed_last_stats"]
INVALID, CAPACITY = -1, -5
NO_READ = 0xffffffff


def plan(n, offsets, k, step, max_occ, budget=0):
    """pwa_seed_plan on raw offsets -> (code, bad read or None, slots, ranges)"""
    L = load_pkg().lib()
    off = (C.c_uint64 * max(len(offsets), 1))(*offsets)
    bad, ns, nr = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
    rc = L.pwa_seed_plan(n, off, max(len(offsets) - 1, 0), k, step, max_occ, budget, C.byref(bad), C.byref(ns), C.byref(nr))
    return rc, None if bad.value == NO_READ else bad.value, ns.value, nr.value


def offsets_of(lengths):
    out = [0]
    for ln in lengths:
        out.append(out[-1] + ln)
    return out


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    block = hdr[hdr.index("Seeding a list of reads against a kept index"):hdr.index("int pwa_seed_plan")]
    for word in ("read_bytes[read_off[r] .. read_off[r + 1])", "q = 0, step, 2 step, ... while q + k <= len", "(len - k) / step + 1 slots, or 0 when len < k",
                 "t + k <= n and text[t .. t + k) == read[q .. q + k) as raw bytes", "NUL", ">= 0x80", "more than max_occ hits", "contributes none",
                 "in ascending (t, q)", "no terminator is appended", "slots x min(max_occ, max(n - k + 1, 0)), reach 2^32", "a read of 2^31 bytes or more",
                 "a total of 2^32 slots or more", "anc_off_out is all zeros", "PWA_OCC_CHUNK_HITS", "one read alone may exceed it",
                 "A range without a slot launches nothing and is not counted", "PWA_E_INVALID when no", "Any pointer may be NULL"):
        assert word in block, word
    assert "pwa_sa_seed: at most N worst-case hits per range of reads" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert callable(pkg.seed_plan) and callable(pkg.Context.index) and callable(pkg.TextIndex.seed) and callable(pkg.TextIndex.close)
    assert hasattr(pkg.TextIndex, "__enter__") and hasattr(pkg.TextIndex, "__exit__")


def test_a_null_index_and_null_pointers_are_invalid():
    L = load_pkg().lib()
    off, anc = (C.c_uint64 * 2)(0, 4), (C.c_uint64 * 2)()
    t, q = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    assert L.pwa_sa_seed(None, b"ACGT", off, 1, 2, 1, 64, anc) == INVALID
    assert L.pwa_sa_seed(None, None, None, 0, 2, 1, 64, None) == INVALID
    assert L.pwa_sa_seed_fetch(None, t, q, 4) == INVALID and L.pwa_sa_seed_fetch(None, None, None, 0) == INVALID
    sm, om, a, b, c = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert L.pwa_sa_seed_last_stats(None, C.byref(sm), C.byref(om), C.byref(a), C.byref(b), C.byref(c)) == INVALID
    assert L.pwa_sa_seed_last_stats(None, None, None, None, None, None) == INVALID
    # the plan: read_off is its one required pointer; the three outputs may each be NULL
    bad, ns, nr = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
    assert L.pwa_seed_plan(100, None, 1, 2, 1, 64, 0, C.byref(bad), C.byref(ns), C.byref(nr)) == INVALID
    assert (bad.value, ns.value, nr.value) == (NO_READ, 0, 0)
    assert L.pwa_seed_plan(100, off, 1, 2, 1, 64, 0, None, None, None) == 0
    assert L.pwa_seed_plan(100, off, 1, 2, 1, 64, 0, None, C.byref(ns), None) == 0 and ns.value == 3
    assert L.pwa_seed_plan(100, None, 0, 2, 1, 64, 0, C.byref(bad), C.byref(ns), C.byref(nr)) == 0        # the empty list
    assert (bad.value, ns.value, nr.value) == (NO_READ, 0, 0)
    assert L.pwa_seed_plan(100, None, 0, 0, 1, 64, 0, None, None, None) == INVALID                           # ... with a bad parameter


@pytest.mark.parametrize("at", [0, 1, 2])
def test_k_step_and_max_occ_of_zero(at):
    for other in (1, 5, 0xffffffff):
        par = [other] * 3
        par[at] = 0
        # a parameter comes before a bad read
        assert plan(100, [0, 10, 5], *par) == (INVALID, None, 0, 0), par
        assert SO.validate(100, [0, 10, 5], *par) == (INVALID, None, 0)
    assert plan(100, [0, 10], 0, 0, 0) == (INVALID, None, 0, 0)
    assert plan(100, [0, 10], 0xffffffff, 0xffffffff, 0xffffffff)[0] == 0


def test_plan_reports_every_code_with_the_first_offending_read():
    top = 1 << 31
    cases = [
        (100, [0, 10, 5, 30], 3, 1, 64),                          # read_off decreases at read 1
        (100, [0, 10, 5, 5 + top], 3, 1, 64),                     # ... and that comes before the long read 2
        (100, [0, top, 5], 3, 1, 64),                             # the long read 0 before the decrease at read 1
        (100, [0, 10, 10 + top - 1], 3, 1, 1),                    # a read of 2^31 - 1 bytes
        (100, [0, 10, 10 + top], 3, 1, 1),                        # ... of 2^31
        (100, [5, 5, 5 + top, 7 + top], 3, 1, 1),                 # offsets need not start at 0
        (100, [0, 1, 2, 2 + top, 1], 3, 1, 1),                    # read 2 before the decrease at read 3
        (1 << 20, [0, 8, 8 + (1 << 30)], 1, 1, 4),                # worst-case hits 2^30 * 4 = 2^32 at read 1
        (1 << 20, [0, 8, 8 + (1 << 30) - 1], 1, 1, 4),            # ... 2^32 - 4
        (3, [0, 8, 8 + (1 << 30)], 1, 1, 4),                      # the text has 3 k-mers: 3 * 2^30
        (2, [0, 8 + (1 << 30)], 1, 1, 0xffffffff),                # 2 * (2^30 + 8)
        (1 << 20, [0, top - 1], 1, 1, 2),                         # (2^31 - 1) * 2 = 2^32 - 2
        (1 << 20, [0, top - 1], 1, 1, 3),
        (0xffffffff, [0, 1], 1, 1, 0xffffffff),                   # one slot of 2^32 - 1 hits at the worst
        (1 << 32, [0, 1], 1, 1, 0xffffffff),                      # max_occ caps it below 2^32 whatever the text
        (1 << 33, [0, 2], 1, 1, 0xffffffff),                      # two such slots: 2^33 - 2
        (100, [0, 50], 101, 1, 64),                               # n < k
        (100, [0, 500, 400], 101, 1, 64),                         # ... still validated
    ]
    codes = set()
    for n, off, k, step, max_occ in cases:
        got = plan(n, off, k, step, max_occ)
        want = SO.validate(n, off, k, step, max_occ)
        assert got[:3] == want, (n, off, k, step, max_occ)
        if want[0]:
            assert got[3] == 0
        codes.add((want[0], want[1]))
    assert {(0, None), (INVALID, 1), (CAPACITY, 0), (CAPACITY, 1), (CAPACITY, 2)} <= codes
    assert plan(100, [0, 10, 10 + top - 1], 3, 1, 1)[:2] == (0, None) and plan(100, [0, 10, 10 + top], 3, 1, 1)[:2] == (CAPACITY, 1)
    assert plan(1 << 20, [0, top - 1], 1, 1, 2)[:3] == (0, None, top - 1) and plan(1 << 20, [0, top - 1], 1, 1, 3)[:2] == (CAPACITY, 0)
    # worst-case hits of exactly 2^32 - 1 = 3 * 5 * 17 * 257 * 65537 and of exactly 2^32: max_occ 65537 on 65535 slots, 65536 on 65536
    assert plan(1 << 20, [0, 65535], 1, 1, 65537)[:2] == (0, None) and SO.worst_hits(65535, 1 << 20, 1, 1, 65537) == (1 << 32) - 1
    assert plan(1 << 20, [4, 4, 4 + 65536], 1, 1, 65536)[:2] == (CAPACITY, 1) and SO.worst_hits(65536, 1 << 20, 1, 1, 65536) == 1 << 32


def test_total_slots_at_the_limit():
    # reads below 2^31 bytes on a one-byte text, k = 1: a slot's worst case is one hit, so only the total can be too large
    big = (1 << 31) - 1
    assert plan(1, offsets_of([big, big, 1]), 1, 1, 64) == (0, None, (1 << 32) - 1, 3)       # 2^32 - 1 slots; each long read alone exceeds the budget
    assert plan(1, offsets_of([big, big, 2]), 1, 1, 64) == (CAPACITY, None, 0, 0)            # 2^32
    assert SO.validate(1, offsets_of([big, big, 1]), 1, 1, 64) == (0, None, (1 << 32) - 1)
    assert SO.validate(1, offsets_of([big, big, 2]), 1, 1, 64) == (CAPACITY, None, 0)
    assert len(SO.ranges(1, [big, big, 1], 1, 1, 64)) == 3
    # ... and with a step: (2^31 - 2) / 2 + 1 = 2^30 slots per read
    assert plan(1, offsets_of([big] * 3 + [big - 2]), 1, 2, 64)[:3] == (0, None, (1 << 32) - 1)
    assert plan(1, offsets_of([big] * 4), 1, 2, 64)[:3] == (CAPACITY, None, 0)
    # a bad read comes before the total
    assert plan(1, offsets_of([big, big, 2]) + [5], 1, 1, 64)[:2] == (INVALID, 3)


@pytest.mark.parametrize("k, step", [(1, 1), (5, 1), (5, 3), (8, 8), (16, 5), (3, 40)])
def test_slot_counts(k, step):
    pkg = load_pkg()
    lens = [0, k - 1, k, k + 1, k + step - 1, k + step, 3 * k + 7 * step]
    for ln in lens:
        want = len([q for q in range(0, ln, step) if q + k <= ln])
        assert SO.slots(ln, k, step) == want
        assert plan(1000, [0, ln], k, step, 64)[:3] == (0, None, want), ln
    got = pkg.seed_plan(1000, lens, k, step)
    assert got == dict(code=0, bad_read=None, slots=sum(SO.slots(ln, k, step) for ln in lens), ranges=1)
    assert [SO.slots(ln, k, step) for ln in lens[:6]] == [0, 0, 1, 2 if step == 1 else 1, 1, 2]   # k + 1 holds a second slot only at step 1


def test_range_counts_against_the_greedy_cut():
    pkg = load_pkg()
    rng = random.Random(3)
    n, k, step, max_occ = 5000, 11, 2, 8
    lens = [rng.choice([0, 0, 5, 11, 12, 40, 300, 1500]) for _ in range(60)] + [0, 3, 0]
    worst = [SO.worst_hits(ln, n, k, step, max_occ) for ln in lens]
    total, longest = sum(worst), max(worst)
    assert longest == 745 * 8
    seen = set()
    for budget in (0, total, total - 1, total // 2, total // 7, longest, longest - 1, 1000, 129, 128, 127, 8, 7, 1):
        got = pkg.seed_plan(n, lens, k, step, max_occ, budget=budget)
        want = SO.ranges(n, lens, k, step, max_occ, budget)
        assert got["code"] == 0 and got["ranges"] == len(want), budget
        seen.add(len(want))
    assert 1 in seen and len([w for w in worst if w]) in seen and len(seen) >= 6
    assert pkg.seed_plan(n, [0, 3, 10], k, budget=1)["ranges"] == 0                     # no slot
    assert pkg.seed_plan(10, lens, k, budget=1) == dict(code=0, bad_read=None, slots=sum(SO.slots(ln, k, 1) for ln in lens), ranges=0)   # n < k
    assert pkg.seed_plan(n, [], k, budget=1) == dict(code=0, bad_read=None, slots=0, ranges=0)
    # a budget beyond 2^32 - 1 counts as that (a range's hits are indexed by uint32): 2^32 - 1 worst-case hits still fit one range
    big = (1 << 31) - 1
    assert pkg.seed_plan(1, [big, big, 1], 1, budget=1 << 40)["ranges"] == 1 == len(SO.ranges(1, [big, big, 1], 1, 1, 64, 1 << 40))
