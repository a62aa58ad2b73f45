"""The banded calls at their int32 range limits on the device: the alignment and score calls (byte compare and substitution matrix)
at the largest scoring that the 2^28 rule admits, the X-drop extension calls at the largest that their 2^27 rule admits, and one step
over either -- where every call must refuse before any device work.  Scores, cells, op lists, strings, rows and pattern ends byte for
byte against the numpy oracles (tied to plain Python DPs at these magnitudes by test_banded_oracle_limits.py), the scores calls
against the alignment calls.

A is the rule's own term as validate_align (pwalign_align.hip) computes it: max(|match|, |mismatch|, |gap_open| + |gap_extend|, 1), with
max |submat| in place of the first two under a table; top(n, m, bits) is the largest A with (n + m + 2) * A < 2^bits.  Every `near the
bound` figure below is asserted on the ORACLE's result, so a case cannot drift away from the edge unnoticed.

Stripe heights as in test_gpu_banded.py: PWA_BANDED_RL=4|8 forces 256- or 512-row stripes, S below.  An oracle result is computed once
per module and shared by the forms and, where the case does not depend on S, by both heights."""
import functools
import random

import numpy as np
import pytest

import banded_ext_oracle as XO
import banded_oracle as BO
from conftest import load_pkg, switched_context
from test_gpu_banded import HEIGHTS
from test_gpu_cigar import fmt
from test_gpu_gotoh import _mutate, _rand

pytestmark = pytest.mark.gpu

MODES = ["nw", "sw", "sg"]
TERMS = ["match", "mismatch", "gaps"]
TALL = (b"A" * 4000, b"C" * 3)
SMALL, SMALL_BAND = (b"ACGT", b"ACGA"), (-1, 1)   # the neighbours of a refused pair in a three-pair list


def top(n, m, bits):
    t = ((1 << bits) - 1) // (n + m + 2)
    assert (n + m + 2) * t < 1 << bits <= (n + m + 2) * (t + 1)
    return t


def _mm(match, mismatch, alpha=b"ACGT"):
    """match on the diagonal, mismatch off it"""
    return load_pkg().subst_table(alpha, np.where(np.eye(len(alpha), dtype=bool), match, mismatch))


def _through(term, a):
    """A = a through one term, the others small -> the byte-compare scoring, and (table, gap_open, gap_extend) with one entry at +-a"""
    go, ge = (-(a // 2), -(a - a // 2)) if term == "gaps" else (-1, -1)
    sc = (a if term == "match" else 1, -a if term == "mismatch" else -1, go, ge)
    m = np.where(np.eye(4, dtype=bool), 1, -1)
    if term == "match":
        m[2, 2] = a      # one positive entry
    if term == "mismatch":
        m[0, 1] = -a     # one negative entry (pattern A on text C: the tall pair's only cell score)
    assert max(abs(sc[0]), abs(sc[1]), abs(go) + abs(ge)) == a == max(int(np.abs(m).max()), abs(go) + abs(ge))
    return sc, (load_pkg().subst_table(b"ACGT", m), go, ge)


def _lists(pairs):
    seqs = [x for pt in pairs for x in pt]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


def _cap(bits):
    pkg = load_pkg()
    assert pkg.lib().pwa_strerror(-5).decode() == "capacity exceeded"   # PWA_E_CAPACITY
    return pytest.raises(pkg.PwaError, match=r"capacity exceeded \(.*must stay below 2\^%d" % bits)


@pytest.fixture(scope="module", params=[4, 8])
def hctx(request):
    with switched_context(PWA_BANDED_RL=str(request.param)) as c:
        c.rl = request.param
        yield c


# ------------------------------------------------------------------ the alignment and score calls: (n + m + 2) * A < 2^28
def _align_calls(c, mode, pairs, bands, sc=None, tab=None):
    """[(op lists, strings, (scores, end_i, end_j))]: the three byte-compare forms under sc, the three table forms under tab"""
    seqs, pa, pb = _lists(pairs)
    out = []
    if sc is not None:
        out.append((c.align_banded_batch(mode, seqs, pa, pb, *sc, bands), c.align_banded_batch_cigar(mode, seqs, pa, pb, *sc, bands),
                    c.scores_banded(mode, seqs, pa, pb, *sc, bands, want_end=True)))
    if tab is not None:
        out.append((c.align_banded_subst_batch(mode, seqs, pa, pb, *tab, bands), c.align_banded_subst_batch_cigar(mode, seqs, pa, pb, *tab, bands),
                    c.scores_banded_subst(mode, seqs, pa, pb, *tab, bands, want_end=True)))
    return out


def _check_align(c, mode, pairs, bands, want, tag, sc=None, tab=None):
    for got, gc, (s, ei, ej) in _align_calls(c, mode, pairs, bands, sc, tab):
        assert len(got) == len(gc) == len(s) == len(want)
        for k, (g, cg, w) in enumerate(zip(got, gc, want)):
            p, t = pairs[k]
            key = (tag, mode, k, len(p), len(t), bands[k])
            assert (g["score"], g["end"], g["start"]) == (w["score"], w["end"], w["start"]), key
            assert g["ops"] == w["ops"], key
            assert (cg["score"], cg["end"], cg["start"]) == (w["score"], w["end"], w["start"]), key
            assert (cg["cigar"], cg["mdz"]) == fmt(p, t, w["ops"], w["start"]), key
            assert (s[k], (ei[k], ej[k])) == (g["score"], g["end"]), key


def _square_pairs(S):
    """case a's pairs: an identical (2 S + 1) x (2 S + 1) pair and a 10 % mutated one of the same lengths, band (-8, 8)"""
    n = 2 * S + 1
    rng = random.Random(3 * S)
    p = _rand(rng, n, b"ACGT")
    q = _rand(rng, n, b"ACGT")
    return [(p, p), (q, (_mutate(rng, q, b"ACGT", rate=0.1) + _rand(rng, n, b"ACGT"))[:n])], [(-8, 8)] * 2


@functools.lru_cache(maxsize=None)
def _case_a(S, mode):
    pairs, bands = _square_pairs(S)
    n = 2 * S + 1
    t = top(n, n, 28)
    sc = (t, -t, -(t // 3), -(t - t // 3))
    return pairs, bands, sc, BO.align_many(pairs, bands, mode, sc[:2], *sc[2:])


@pytest.mark.parametrize("mode", MODES)
def test_a_largest_positive_keys(hctx, mode):
    """the identical pair scores n * top with n M ops; SW's row key H << 4 sits in the last percent below the sign bit, and the records
    cross two stripe boundaries"""
    S = HEIGHTS[hctx.rl]
    pairs, bands, sc, want = _case_a(S, mode)
    n = 2 * S + 1
    assert (want[0]["score"], want[0]["ops"], want[0]["end"]) == (n * sc[0], b"M" * n, (n, n))
    assert 0 < want[1]["score"] < want[0]["score"] and set(want[1]["ops"]) == set(b"MID")
    if mode == "sw":
        assert want[0]["score"] * 16 > 0.99 * (1 << 31)
    _check_align(hctx, mode, pairs, bands, want, ("a", S), sc=sc, tab=(_mm(sc[0], sc[1]), sc[2], sc[3]))


@functools.lru_cache(maxsize=None)
def _case_b(S, mode):
    rng = random.Random(5 * S)
    n = S + 88
    m = n + 4000
    pairs, bands = [(_rand(rng, n, b"AC"), _rand(rng, m, b"GT"))], [(0, 4000)]
    t = top(n, m, 28)
    sc = (1, -t, -1, -(t - 1))
    return pairs, bands, sc, BO.align_many(pairs, bands, mode, sc[:2], *sc[2:])


@pytest.mark.parametrize("mode", MODES)
def test_b_most_negative_keys_through_the_hand_off_row(hctx, mode):
    """no symbol in common under a band of 4001 diagonals (the cap is 4096), one stripe boundary: every hand-off entry is a large
    negative key or the sentinel"""
    pairs, bands, sc, want = _case_b(HEIGHTS[hctx.rl], mode)
    assert bands[0][1] - bands[0][0] + 1 == 4001
    if mode == "nw":
        assert want[0]["score"] < -0.85 * (1 << 28)
    _check_align(hctx, mode, pairs, bands, want, ("b", hctx.rl), sc=sc, tab=(_mm(sc[0], sc[1]), sc[2], sc[3]))


C_SCORINGS = {"open0": lambda t: (1, -t, 0, -t), "extend0": lambda t: (1, -t, -t, 0)}   # extend0: an extension ties its opening


@functools.lru_cache(maxsize=None)
def _case_c(shape, kind, mode):
    pair, band = {"wide": ((b"A", b"C" * 4000), (0, 3999)), "tall": (TALL, (-3997, 0))}[shape]
    sc = C_SCORINGS[kind](top(len(pair[0]), len(pair[1]), 28))
    return [pair], [band], sc, BO.align_many([pair], [band], mode, sc[:2], *sc[2:])


@pytest.mark.parametrize("shape,mode", [("wide", "nw"), ("wide", "sw"), ("wide", "sg"), ("tall", "nw"), ("tall", "sg")])
@pytest.mark.parametrize("kind", ["open0", "extend0"])
def test_c_closest_to_the_bound(hctx, shape, kind, mode):
    """one symbol against 4000 and 4000 against three: the most negative score the rule admits.  The tall pair runs 16 stripes of 256
    rows or 8 of 512, and every hand-off entry holds a near-limit key next to the sentinel"""
    pairs, bands, sc, want = _case_c(shape, kind, mode)
    if kind == "open0" and (mode == "nw" or shape == "tall"):
        assert want[0]["score"] < -0.99 * (1 << 28)
    _check_align(hctx, mode, pairs, bands, want, ("c", shape, kind, hctx.rl), sc=sc, tab=(_mm(sc[0], sc[1]), sc[2], sc[3]))


@functools.lru_cache(maxsize=None)
def _at_top_28(which, S, term, mode):
    """case d's pairs at A = top through one term -> pairs, bands, sc, tab and the two oracle results"""
    pairs, bands = _square_pairs(S) if which == "square" else ([TALL], [(-3997, 0)])
    sc, tab = _through(term, top(len(pairs[0][0]), len(pairs[0][1]), 28))
    return pairs, bands, sc, tab, BO.align_many(pairs, bands, mode, sc[:2], *sc[2:]), BO.align_many(pairs, bands, mode, *tab)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("term", TERMS)
def test_d_at_the_bound_through_each_term(hctx, term, mode):
    pairs, bands, sc, tab, want, want_tab = _at_top_28("square", HEIGHTS[hctx.rl], term, mode)
    _check_align(hctx, mode, pairs, bands, want, ("d", term, hctx.rl), sc=sc)
    _check_align(hctx, mode, pairs, bands, want_tab, ("d table", term, hctx.rl), tab=tab)


def test_d_at_the_bound_tall_pair_through_the_match_term(hctx):
    """(its mismatch and gap terms at the bound: test_c_closest_to_the_bound)"""
    pairs, bands, sc, tab, want, want_tab = _at_top_28("tall", 0, "match", "nw")
    _check_align(hctx, "nw", pairs, bands, want, ("d tall", hctx.rl), sc=sc)
    _check_align(hctx, "nw", pairs, bands, want_tab, ("d tall table", hctx.rl), tab=tab)


@pytest.mark.parametrize("which", ["square", "tall"])
def test_d_one_step_over_is_refused(hctx, which):
    """A = top + 1 through each term in turn: PWA_E_CAPACITY from all six calls, alone and as the middle pair of three, before any
    device work -- the stats of the last valid calls stay"""
    S = HEIGHTS[hctx.rl]
    pairs, bands = (_square_pairs(S)[0][:1], [(-8, 8)]) if which == "square" else ([TALL], [(-3997, 0)])
    t = top(len(pairs[0][0]), len(pairs[0][1]), 28)
    seqs, pa, pb = _lists([SMALL])
    assert hctx.align_banded_batch("nw", seqs, pa, pb, 1, -1, -1, -1, [SMALL_BAND])[0]["score"] == 2
    assert hctx.scores_banded("nw", seqs, pa, pb, 1, -1, -1, -1, [SMALL_BAND]) == [2]
    before = (hctx.align_banded_stats(), hctx.scores_banded_stats())
    assert before[0]["fill_ms"] > 0 and before[1]["in_band_cells"] > 0
    for term in TERMS:
        sc, tab = _through(term, t + 1)
        for lp, lb in ((pairs, bands), ([SMALL] + pairs + [SMALL], [SMALL_BAND] + bands + [SMALL_BAND])):
            seqs, pa, pb = _lists(lp)
            for mode in MODES if which == "square" else ["nw", "sg"]:
                for fn, args in [(hctx.align_banded_batch, sc), (hctx.align_banded_batch_cigar, sc), (hctx.scores_banded, sc),
                                 (hctx.align_banded_subst_batch, tab), (hctx.align_banded_subst_batch_cigar, tab), (hctx.scores_banded_subst, tab)]:
                    with _cap(28):
                        fn(mode, seqs, pa, pb, *args, lb)
    assert (hctx.align_banded_stats(), hctx.scores_banded_stats()) == before


# ------------------------------------------------------------------ the X-drop extension calls: (n + m + 2) * A < 2^27
def _check_ext(c, pairs, bands, xdrop, want, tag, sc=None, tab=None):
    """want: banded_ext_oracle's results under the table (with pend); the byte-compare forms return everything but the pattern end"""
    seqs, pa, pb = _lists(pairs)
    if sc is not None:
        got, gc = c.extend_banded_batch(seqs, pa, pb, *sc, bands, xdrop), c.extend_banded_batch_cigar(seqs, pa, pb, *sc, bands, xdrop)
        s, ei, ej, rw = c.scores_extend_banded(seqs, pa, pb, *sc, bands, xdrop, want_end=True)
        for k, (g, cg, w) in enumerate(zip(got, gc, want)):
            p, t = pairs[k]
            key = (tag, xdrop, k, len(p), len(t), bands[k])
            assert (g["score"], g["end"], g["start"], g["rows"]) == (w["score"], w["end"], (0, 0), w["rows"]), key
            assert g["ops"] == w["ops"], key
            assert (cg["score"], cg["end"], cg["start"], cg["rows"]) == (w["score"], w["end"], (0, 0), w["rows"]), key
            assert (cg["cigar"], cg["mdz"]) == fmt(p, t, w["ops"], (0, 0)), key
            assert (s[k], (ei[k], ej[k]), rw[k]) == (g["score"], g["end"], g["rows"]), key
    if tab is not None:
        got, gc = c.extend_banded_subst_batch(seqs, pa, pb, *tab, bands, xdrop), c.extend_banded_subst_batch_cigar(seqs, pa, pb, *tab, bands, xdrop)
        s, ei, ej, rw, pe = c.scores_extend_banded_subst(seqs, pa, pb, *tab, bands, xdrop, want_end=True)
        for k, (g, cg, w) in enumerate(zip(got, gc, want)):
            p, t = pairs[k]
            key = (tag, "table", xdrop, k, len(p), len(t), bands[k])
            assert (g["score"], g["end"], g["start"], g["rows"], g["pend"]) == (w["score"], w["end"], (0, 0), w["rows"], w["pend"]), key
            assert g["ops"] == w["ops"], key
            assert (cg["score"], cg["end"], cg["start"], cg["rows"], cg["pend"]) == (w["score"], w["end"], (0, 0), w["rows"], w["pend"]), key
            assert (cg["cigar"], cg["mdz"]) == fmt(p, t, w["ops"], (0, 0)), key
            assert (s[k], (ei[k], ej[k]), rw[k], pe[k]) == (g["score"], g["end"], g["rows"], g["pend"]), key


E_XDROPS = [-1, 1 << 27, 5]


@functools.lru_cache(maxsize=None)
def _case_e():
    t = top(4000, 3, 27)
    tab = (load_pkg().subst_table(b"AC", np.full((2, 2), -t)), 0, -t)
    return (1, -t, 0, -t), tab, XO.extend_multi([TALL], [(-4000, 0)], *tab, E_XDROPS)


@pytest.mark.parametrize("xdrop", E_XDROPS)
def test_e_negative_row_keys_next_to_the_no_cell_key(hctx, xdrop):
    """4000 against three without a common symbol: nothing beats the anchor, and every row's best is a negative value down to the
    bound.  A wrapped key would show as a positive best score, a row key taken for `no in-band cell` as an early stop"""
    sc, tab, want = _case_e()
    w = want[xdrop][0]
    assert (w["score"], w["end"], w["ops"]) == (0, (0, 0), b"")
    if xdrop == 5:
        assert w["rows"] == 0 and w["pend"] is None
    else:
        assert w["rows"] == 4000 and w["pend"][1] == 1 and w["pend"][0] < -0.99 * (1 << 27)
    _check_ext(hctx, [TALL], [(-4000, 0)], xdrop, want[xdrop], ("e", hctx.rl), sc=sc, tab=tab)


def _all_terms(t):
    return (t, -t, -(t // 2), -(t - t // 2))


@functools.lru_cache(maxsize=None)
def _case_f(S):
    """case a's identical pair at top(n, n, 27), and X + A.. against X + C.. with |X| = S + 1 and every term at the bound of its own
    lengths: the drop 2 * top is taken off a best near 2^26, and values of that size decide the stop row"""
    pairs, bands = _square_pairs(S)
    n = 2 * S + 1
    sc = _all_terms(top(n, n, 27))
    drops = [-1, 1 << 27, 3 * sc[0]]
    ident = (pairs[:1], bands[:1], sc, drops, XO.extend_multi(pairs[:1], bands[:1], _mm(sc[0], sc[1]), sc[2], sc[3], drops))
    x = _rand(random.Random(7 * S), S + 1, b"ACGT")
    pair, band = (x + b"A" * 40, x + b"C" * 40), (-32, 32)
    sc = _all_terms(top(S + 41, S + 41, 27))
    drops = [2 * sc[0], -1]
    stop = ([pair], [band], sc, drops, XO.extend_multi([pair], [band], _mm(sc[0], sc[1]), sc[2], sc[3], drops))
    return ident, stop


def test_f_positive_side_and_a_stop_at_near_limit_values(hctx):
    S = HEIGHTS[hctx.rl]
    ident, stop = _case_f(S)
    pairs, bands, sc, drops, want = ident
    n = 2 * S + 1
    for xdrop in drops:
        w = want[xdrop][0]
        assert (w["score"], w["end"], w["ops"], w["rows"], w["pend"]) == (n * sc[0], (n, n), b"M" * n, n, (n * sc[0], n))
        _check_ext(hctx, pairs, bands, xdrop, want[xdrop], ("f", S), sc=sc, tab=(_mm(sc[0], sc[1]), sc[2], sc[3]))
    assert n * sc[0] > 0.49 * (1 << 27)   # (H <= min(n, m) * match: half the rule's range)
    pairs, bands, sc, drops, want = stop
    w, free = want[2 * sc[0]][0], want[-1][0]
    assert (w["score"], w["end"]) == ((S + 1) * sc[0], (S + 1, S + 1)) and w["score"] > 0.8 * (1 << 26)
    assert S + 1 < w["rows"] < S + 41 and w["pend"] is None and free["rows"] == S + 41 and free["pend"] is not None
    for xdrop in drops:
        _check_ext(hctx, pairs, bands, xdrop, want[xdrop], ("f stop", S), sc=sc, tab=(_mm(sc[0], sc[1]), sc[2], sc[3]))


@functools.lru_cache(maxsize=None)
def _at_top_27(S, term):
    pairs, bands = _square_pairs(S)
    n = 2 * S + 1
    sc, tab = _through(term, top(n, n, 27))
    drops = [-1, 1 << 27, 50]
    return pairs, bands, sc, tab, drops, XO.extend_multi(pairs, bands, _mm(sc[0], sc[1]), sc[2], sc[3], drops), XO.extend_multi(pairs, bands, *tab, drops)


@pytest.mark.parametrize("term", TERMS)
def test_g_at_the_bound_through_each_term(hctx, term):
    """(the tall pair with its mismatch and gap terms at the bound: test_e_negative_row_keys_next_to_the_no_cell_key)"""
    pairs, bands, sc, tab, drops, want, want_tab = _at_top_27(HEIGHTS[hctx.rl], term)
    for xdrop in drops:
        _check_ext(hctx, pairs, bands, xdrop, want[xdrop], ("g", term, hctx.rl), sc=sc)
        _check_ext(hctx, pairs, bands, xdrop, want_tab[xdrop], ("g", term, hctx.rl), tab=tab)


@pytest.mark.parametrize("which", ["square", "tall"])
def test_g_one_step_over_is_refused_and_the_2_28_rule_still_admits_it(hctx, which):
    S = HEIGHTS[hctx.rl]
    pairs, bands = (_square_pairs(S)[0][:1], [(-8, 8)]) if which == "square" else ([TALL], [(-4000, 0)])
    t = top(len(pairs[0][0]), len(pairs[0][1]), 27)
    seqs, pa, pb = _lists([SMALL])
    assert hctx.extend_banded_batch(seqs, pa, pb, 1, -1, -1, -1, [SMALL_BAND], 10)[0]["score"] == 3
    before = hctx.extend_banded_stats()
    assert before["fill_ms"] > 0 and before["rows_considered"] == 4
    for term in TERMS:
        sc, tab = _through(term, t + 1)
        for lp, lb in ((pairs, bands), ([SMALL] + pairs + [SMALL], [SMALL_BAND] + bands + [SMALL_BAND])):
            seqs, pa, pb = _lists(lp)
            for xdrop in (-1, 1 << 27, 5):
                for fn, args in [(hctx.extend_banded_batch, sc), (hctx.extend_banded_batch_cigar, sc), (hctx.scores_extend_banded, sc),
                                 (hctx.extend_banded_subst_batch, tab), (hctx.extend_banded_subst_batch_cigar, tab),
                                 (hctx.scores_extend_banded_subst, tab)]:
                    with _cap(27):
                        fn(seqs, pa, pb, *args, lb, xdrop)
        assert hctx.extend_banded_stats() == before
        seqs, pa, pb = _lists(pairs)
        got = (hctx.scores_banded("nw", seqs, pa, pb, *sc, bands), hctx.scores_banded_subst("nw", seqs, pa, pb, *tab, bands))
        if which == "square":
            assert got == ([BO.align(*pairs[0], bands[0], "nw", sc[:2], *sc[2:])["score"]], [BO.align(*pairs[0], bands[0], "nw", *tab)["score"]])
    assert hctx.extend_banded_stats() == before
