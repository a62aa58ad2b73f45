"""The wavefront-alignment calls at the C boundary, without a GPU: exported, listed, declared, refusing a null context and null pointers,
and the host-only plan (pwa_wfa_plan: validation, penalties, bound, cells) against the oracle."""
import ctypes as C
import os
import random
import re

import pytest

import wfa_oracle as WO
from conftest import ROOT, load_pkg

NAMES = ["pwa_wfa_plan", "pwa_scores_wfa", "pwa_align_wfa_batch", "pwa_align_wfa_batch_cigar", "pwa_wfa_last_stats"]
INVALID, CAPACITY = -1, -5
SCORINGS = [(1, -4, -6, -1), (5, -4, -16, -4), (1, -1, 0, -1), (0, -4, -6, -2), (3, 1, -2, -1), (-1, -3, 0, -2)]


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    assert re.search(r"#define\s+PWA_WFA_NONE\s+INT32_MIN", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for method in ("scores_wfa", "align_wfa_batch", "align_wfa_batch_cigar", "align_wfa_stats"):
        assert callable(getattr(pkg.Context, method))
    assert callable(pkg.wfa_plan)
    assert pkg.WFA_NONE == -(1 << 31)


def test_null_context_and_null_pointers_are_invalid():
    L = load_pkg().lib()
    off, pa, pb = (C.c_uint64 * 3)(0, 1, 2), (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1)
    sc, pen = (C.c_int32 * 1)(), (C.c_uint32 * 1)()
    ops, ooff, nops = C.create_string_buffer(4), (C.c_uint64 * 1)(0), (C.c_uint64 * 1)()
    cg, md, co, mo = C.create_string_buffer(64), C.create_string_buffer(64), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    assert L.pwa_scores_wfa(None, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, None, sc, pen) == INVALID
    assert L.pwa_align_wfa_batch(None, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, sc, ops, ooff, nops, None) == INVALID
    assert L.pwa_align_wfa_batch_cigar(None, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, sc, cg, 64, co, md, 64, mo, None, None) == INVALID
    assert L.pwa_wfa_last_stats(None, None, None, None, None) == INVALID
    n, m = (C.c_uint64 * 1)(3), (C.c_uint64 * 1)(4)
    p4 = (C.c_int32 * 4)()
    assert L.pwa_wfa_plan(1, -4, -6, -1, n, m, None, 1, None, None, None) == INVALID
    assert L.pwa_wfa_plan(1, -4, -6, -1, None, m, None, 1, p4, None, None) == INVALID
    assert L.pwa_wfa_plan(1, -4, -6, -1, n, None, None, 1, p4, None, None) == INVALID
    assert L.pwa_wfa_plan(1, -4, -6, -1, n, m, None, 1, p4, None, None) == 0 and tuple(p4) == (10, 12, 3, 1)
    assert L.pwa_wfa_plan(1, -4, -6, -1, None, None, None, 0, p4, None, None) == 0


def test_range_planner_selftest():
    """pwa_selftest_host ends with the wavefront unit's range planner (pwa::selftest_wfa_plan), host only: every one of the five forms
    under scorings with a shallow and a deep ring, a few hundred pairs of 0 .. some thousand symbols on either side, without bounds, with
    loose ones and with runs of pairs the host rules out, budgets from "one range" down to less than any pair.  It checks that the ranges
    tile the list and are the greedy cut; that every pair not ruled out stands once in its range's launch list, longest plan first,
    with its own lengths, blob offsets and result slot; that the workspace slices of a range are disjoint, lie inside the range's
    workspace and hold what the kernels address by their own formulas; that the op slices tile the range's op bytes in pair order (none
    for a score form); and that the buffer capacities cover every range"""
    L = load_pkg().lib()
    L.pwa_selftest_host.argtypes = [C.c_uint32]
    L.pwa_selftest_host.restype = C.c_int
    for seed in (0, 0x5eed, 0xffffffff):
        assert L.pwa_selftest_host(seed) == 0, seed


@pytest.mark.parametrize("bad", [(1, 1, -1, -1), (2, 3, -1, -1), (0, -1, -1, 0), (-2, -3, 0, -1), (1, 0, 1, -1), (1, 0, -1, 1)])
def test_plan_refuses_a_scoring_without_a_penalty_form(bad):
    """match == mismatch, match < mismatch, match - 2 gap_extend == 0 (twice), a positive gap open, a positive gap extend"""
    L = load_pkg().lib()
    n, m = (C.c_uint64 * 1)(3), (C.c_uint64 * 1)(4)
    p4 = (C.c_int32 * 4)(7, 7, 7, 7)
    assert L.pwa_wfa_plan(*bad, n, m, None, 1, p4, None, None) == INVALID
    assert tuple(p4) == (7, 7, 7, 7)
    with pytest.raises(ValueError):
        WO.penalties(*bad)


def test_plan_range_rule():
    L = load_pkg().lib()
    p4 = (C.c_int32 * 4)()
    big = 10 * 1000 * 1000   # 1/-4/-6/-1: the largest magnitude is |gap_open| + |gap_extend| = 7
    for n, m, ok in [(big, big, True), (1 << 27, 1 << 27, False), ((1 << 28) // 7 - 2, 0, True), ((1 << 28) // 7 - 1, 0, False), (0, (1 << 28) // 7, False)]:
        assert WO.in_range(n, m, 1, -4, -6, -1) == ok
        rc = L.pwa_wfa_plan(1, -4, -6, -1, (C.c_uint64 * 1)(n), (C.c_uint64 * 1)(m), None, 1, p4, None, None)
        assert rc == (0 if ok else CAPACITY), (n, m)


@pytest.mark.parametrize("sc", SCORINGS)
def test_plan_against_the_oracle_on_ragged_lengths(sc):
    pkg = load_pkg()
    rng = random.Random(sum(sc))
    lengths = [(0, 0), (0, 7), (9, 0), (1, 1), (5, 5), (5, 8), (300, 17), (17, 300), (1000, 1003)]
    lengths += [(rng.randint(0, 400), rng.randint(0, 400)) for _ in range(40)]
    x, o, e, g = WO.penalties(*sc)
    got = pkg.wfa_plan(*sc, lengths)
    assert got["pen"] == (x, o, e, g)
    for k, (n, m) in enumerate(lengths):
        assert (got["p_max"][k], got["cells"][k]) == WO.plan(n, m, *sc), (n, m)
        assert got["p_max"][k] == (o + n * e if n else 0) + (o + m * e if m else 0)
    # bounds: far below, around the one-gap score of the pair, at and above the score of a perfect match
    bounds = []
    for n, m in lengths:
        one_gap = WO.score_of(o + abs(n - m) * e, n, m, sc[0], g) if n != m else WO.score_of(0, n, m, sc[0], g)
        bounds.append(rng.choice([-(1 << 20), one_gap - 3, one_gap - 1, one_gap, one_gap + 1, one_gap + 40]))
    got = pkg.wfa_plan(*sc, lengths, bounds)
    kinds = set()
    for k, (n, m) in enumerate(lengths):
        want = WO.plan(n, m, *sc, bounds[k])
        assert (got["p_max"][k], got["cells"][k]) == want, (n, m, bounds[k])
        kinds.add(want[0] is None)
    assert kinds == {True, False}


def test_plan_host_side_not_found_cases():
    pkg = load_pkg()
    # P_max < 0: a bound above the score of identical sequences; P_max < o + |n - m| e: a bound above the score of the one forced gap
    got = pkg.wfa_plan(1, -4, -6, -1, [(5, 5), (5, 5), (5, 8), (5, 8), (0, 0), (0, 0), (0, 3), (0, 3)], [5, 6, -4, -3, 0, 1, -9, -8])
    assert got["p_max"] == [0, None, 21, None, 0, None, 21, None]
    assert got["cells"] == [1, 0, WO.cells_to(21, 5, 8, 12, 3), 0, 1, 0, WO.cells_to(21, 0, 3, 12, 3), 0]
    assert pkg.wfa_plan(1, -4, -6, -1, [(5, 8)], -4) == pkg.wfa_plan(1, -4, -6, -1, [(5, 8)], [-4])   # one int for every pair
