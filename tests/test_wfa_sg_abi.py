"""The semi-global wavefront calls at the C boundary, without a GPU: exported, listed, declared, refusing a null context, null pointers
and scorings without a per-pattern-symbol penalty form, and the host-only plan (pwa_wfa_sg_plan: validation, penalties, bound, the closed
form of the cells) against wfa_sg_oracle.py."""
import ctypes as C
import os
import random
import re

import pytest

import wfa_sg_oracle as SO
from conftest import ROOT, load_pkg

NAMES = ["pwa_wfa_sg_plan", "pwa_scores_wfa_sg", "pwa_align_wfa_sg_batch", "pwa_align_wfa_sg_batch_cigar"]
INVALID, CAPACITY = -1, -5
SCORINGS = [(1, -4, -6, -1), (0, -1, 0, -1), (2, -3, -5, -2), (1, -1, 0, -1), (5, -4, -16, -4), (3, -3, -9, -3), (1, -40, -6, -1), (-1, -3, 0, -2)]
BAD = [(1, 1, -1, -1), (2, 3, -1, -1), (1, 0, 1, -1), (1, 0, -1, 1), (1, -1, -1, 0), (0, -1, 0, 0), (-2, -3, 0, -1), (-1, -3, 0, -1)]


def test_symbols_are_exported_listed_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    block = hdr[hdr.index("Semi-global wavefront alignments"):hdr.index("int pwa_wfa_sg_plan")]
    for word in ("eI0 = -gap_extend", "eD0 = match - gap_extend", "score = match n - g P", "M[0][k] = extend(k)", "LOWEST", "khD", "P_worst", "codes form"):
        assert word in block, word
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    for method in ("scores_wfa_sg", "align_wfa_sg_batch", "align_wfa_sg_batch_cigar", "align_wfa_stats"):
        assert callable(getattr(pkg.Context, method))
    assert callable(pkg.wfa_sg_plan)


def test_null_context_and_null_pointers_are_invalid():
    L = load_pkg().lib()
    off, pa, pb = (C.c_uint64 * 3)(0, 1, 2), (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1)
    sc, pen, ej = (C.c_int32 * 1)(), (C.c_uint32 * 1)(), (C.c_uint64 * 1)()
    ops, ooff, nops = C.create_string_buffer(4), (C.c_uint64 * 1)(0), (C.c_uint64 * 1)()
    cg, md, co, mo = C.create_string_buffer(64), C.create_string_buffer(64), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    end, start = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    calls = [(L.pwa_scores_wfa_sg, [None, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, None, sc, pen, ej], [5, 6, 8, 9, 12]),
             (L.pwa_align_wfa_sg_batch, [None, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, sc, ops, ooff, nops, end, start, None], [5, 6, 8, 9, 11, 12, 13, 14]),
             (L.pwa_align_wfa_sg_batch_cigar, [None, 1, -4, -6, -1, b"AC", off, 2, pa, pb, 1, sc, cg, 64, co, md, 64, mo, end, start, None, None],
              [5, 6, 8, 9, 11, 12, 14, 15, 17])]
    for fn, full, nullable in calls:
        assert fn(*full) == INVALID
        for at in nullable:   # still the null context's answer, whatever else is missing
            args = list(full)
            args[at] = None
            assert fn(*args) == INVALID
        bad = list(full)
        bad[1:5] = [1, -1, -1, 0]
        assert fn(*bad) == INVALID
    n, m = (C.c_uint64 * 1)(3), (C.c_uint64 * 1)(4)
    p5 = (C.c_int32 * 5)()
    assert L.pwa_wfa_sg_plan(1, -4, -6, -1, n, m, None, 1, None, None, None) == INVALID
    assert L.pwa_wfa_sg_plan(1, -4, -6, -1, None, m, None, 1, p5, None, None) == INVALID
    assert L.pwa_wfa_sg_plan(1, -4, -6, -1, n, None, None, 1, p5, None, None) == INVALID
    assert L.pwa_wfa_sg_plan(1, -4, -6, -1, n, m, None, 1, p5, None, None) == 0 and tuple(p5) == (5, 6, 1, 2, 1)
    assert L.pwa_wfa_sg_plan(1, -4, -6, -1, None, None, None, 0, p5, None, None) == 0


@pytest.mark.parametrize("bad", BAD)
def test_plan_refuses_a_scoring_without_a_penalty_form(bad):
    """match == mismatch, match < mismatch, a positive gap open, a positive gap extend, gap_extend == 0 (twice: eI would be 0),
    match - gap_extend == 0 and < 0"""
    L = load_pkg().lib()
    n, m = (C.c_uint64 * 1)(3), (C.c_uint64 * 1)(4)
    p5 = (C.c_int32 * 5)(7, 7, 7, 7, 7)
    assert L.pwa_wfa_sg_plan(*bad, n, m, None, 1, p5, None, None) == INVALID
    assert tuple(p5) == (7, 7, 7, 7, 7)
    with pytest.raises(ValueError):
        SO.penalties(*bad)
    with pytest.raises(load_pkg().PwaError):
        load_pkg().wfa_sg_plan(*bad, [(3, 4)])


def test_the_global_form_still_takes_what_only_it_can():
    """gap_extend = 0 with match > 0 has a global penalty form and no semi-global one, and the two conversions differ on the rest"""
    pkg = load_pkg()
    assert pkg.wfa_plan(1, -1, -1, 0, [(3, 4)])["pen"] == (4, 2, 1, 1)
    with pytest.raises(pkg.PwaError):
        pkg.wfa_sg_plan(1, -1, -1, 0, [(3, 4)])
    assert pkg.wfa_plan(1, -4, -6, -1, [(3, 4)])["pen"] == (10, 12, 3, 1)
    assert pkg.wfa_sg_plan(1, -4, -6, -1, [(3, 4)])["pen"] == (5, 6, 1, 2, 1)


def test_plan_range_rule():
    L = load_pkg().lib()
    p5 = (C.c_int32 * 5)()
    big = 10 * 1000 * 1000   # 1/-4/-6/-1: the largest magnitude is |gap_open| + |gap_extend| = 7
    for n, m, ok in [(big, big, True), (1 << 27, 1 << 27, False), ((1 << 28) // 7 - 2, 0, True), ((1 << 28) // 7 - 1, 0, False), (0, (1 << 28) // 7, False)]:
        assert SO.in_range(n, m, 1, -4, -6, -1) == ok
        rc = L.pwa_wfa_sg_plan(1, -4, -6, -1, (C.c_uint64 * 1)(n), (C.c_uint64 * 1)(m), None, 1, p5, None, None)
        assert rc == (0 if ok else CAPACITY), (n, m)
        assert L.pwa_wfa_plan(1, -4, -6, -1, (C.c_uint64 * 1)(n), (C.c_uint64 * 1)(m), None, 1, p5, None, None) == rc


@pytest.mark.parametrize("sc", SCORINGS)
def test_plan_against_the_oracle_on_ragged_lengths(sc):
    """the closed form of the cells against the term-by-term sum: n = 0, m = 0, n > m, n < m, and bounds that put P_max below, at and
    above o + eD (where the span starts to grow to the left) and around the forced 'D' run of n > m"""
    pkg = load_pkg()
    rng = random.Random(sum(sc) + 3)
    lengths = [(0, 0), (0, 7), (9, 0), (1, 1), (5, 5), (5, 8), (8, 5), (300, 17), (17, 300), (1000, 1003), (1, 0), (2, 1)]
    lengths += [(rng.randint(0, 400), rng.randint(0, 400)) for _ in range(40)]
    x, o, ei, ed, g = SO.penalties(*sc)
    got = pkg.wfa_sg_plan(*sc, lengths)
    assert got["pen"] == (x, o, ei, ed, g)
    for k, (n, m) in enumerate(lengths):
        assert (got["p_max"][k], got["cells"][k]) == SO.plan(n, m, *sc), (n, m)
        assert got["p_max"][k] == SO.p_worst(n, m, x, o, ed)
    kinds = set()
    for shift in (-3, -1, 0, 1, 2, 40):
        bounds = []
        for n, m in lengths:   # the score that leaves P_max = o + eD + shift, or the forced gap's penalty + shift
            at = o + max(n - m, 1) * ed + shift
            bounds.append(sc[0] * n - g * at)
        got = pkg.wfa_sg_plan(*sc, lengths, bounds)
        for k, (n, m) in enumerate(lengths):
            want = SO.plan(n, m, *sc, bounds[k])
            assert (got["p_max"][k], got["cells"][k]) == want, (n, m, bounds[k])
            if want[0] is not None and n:
                assert want[0] == min(SO.p_worst(n, m, x, o, ed), o + max(n - m, 1) * ed + shift)
            kinds.add(want[0] is None)
    assert kinds == {True, False}
    far = pkg.wfa_sg_plan(*sc, lengths, -(1 << 20))
    assert far == pkg.wfa_sg_plan(*sc, lengths)


def test_plan_host_side_not_found_cases():
    pkg = load_pkg()
    # 1/-4/-6/-1: x, o, eI, eD = 5, 6, 1, 2.  P_max < 0: a bound above the score of an exact occurrence; n > m and P_max < o + (n - m) eD:
    # a bound above the score of the forced 'D' run; n = 0 scores 0
    lengths = [(5, 9), (5, 9), (5, 3), (5, 3), (0, 0), (0, 0), (0, 3), (0, 3), (4, 0), (4, 0)]
    got = pkg.wfa_sg_plan(1, -4, -6, -1, lengths, [5, 6, -5, -4, 0, 1, 0, 1, -10, -9])
    assert got["p_max"] == [0, None, 10, None, 0, None, 0, None, 14, None]
    assert got["cells"] == [10, 0, SO.cells_to(10, 5, 3, 6, 2), 0, 1, 0, 4, 0, SO.cells_to(14, 4, 0, 6, 2), 0]
    assert pkg.wfa_sg_plan(1, -4, -6, -1, [(5, 3)], -5) == pkg.wfa_sg_plan(1, -4, -6, -1, [(5, 3)], [-5])   # one int for every pair
