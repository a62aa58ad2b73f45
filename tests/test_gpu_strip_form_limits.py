"""The magnitude switches of the strip kernels' cell forms (choose_cell_form, pwalign.hip), each at its bound: the list at the bound runs
the narrow form -- asserted by the kernel name -- and equals the oracle; one step outside it runs the wide form and equals it too.
Every list is one the library admits by its own rule; nothing forces a form past its guard.

  hw4's packed (H, dist) key, BM_DISTP   max_n + max_m <= 4000 and (max_n + max_m + 2) * max|score| < 65536  (batch_nwdist.hip.h: dist
                                         in 12 bits, two priority bits, H above)
  hw3 shifted against plain, BM_AFFS     (max_n + max_m + 4) * A * 4 < 2^27,  A = max(|match|, |mismatch|, |gap_open|, |gap_extend|)
  gotoh NW shifted against plain         the same rule (BM_GNWS / BM_GNW)
  gap-shifted linear NW, BM_NWG          match - 2 gap and mismatch - 2 gap in a byte, and (max_n + max_m + 4) * A * 4 < 2^30

Both bounds are over the list's longest pattern and longest text, so a shape n x m is a list of its own: the pair of that shape
with nothing in common (AC against GT, or two halves of the alphabet), a related pair of that shape, a mutated one, and 1 x m and
n x 1 beside them.  The strips alone are under test (PWA_SCORES_ROUTE=0, PWA_FORCE_LANES=0); the height is the cost model's except
where a test pins it.  The linear NW call has no range check of its own, so its outer side is never refused: the plain form takes
it."""
import random
import re

import pytest

import oracle_lib as O
from conftest import switched_context
from test_gpu_strip_table import mismatches, oracle_results, rand_seq, related, run_named

pytestmark = pytest.mark.gpu

STRIPS = {"PWA_SCORES_ROUTE": "0", "PWA_FORCE_LANES": "0"}
LETTERS = bytes(range(65, 91))


def mode_of(name):
    """'batch_affine_kernel<R=52,BM_AFFS,SC_PERM>' -> ('BM_AFFS', 'SC_PERM'); a name with a second engine's part in it matches nothing"""
    m = re.fullmatch(r"batch_(?:scores|affine|gotoh)_kernel<R=\d+,(BM_[A-Z]+),(SC_[A-Z]+)>", name)
    assert m, name
    return m.groups()


def shape_list(n, m, alpha, seed):
    """the list of shape n x m: max_n == n and max_m == m exactly -> (seqs, pair_a, pair_b); pair 0 is the one with nothing in common"""
    rng = random.Random("%d %d %d" % (n, m, seed))
    half = len(alpha) // 2
    x = rand_seq(rng, max(n, m), alpha)
    pairs = [(rand_seq(rng, n, alpha[:half]), rand_seq(rng, m, alpha[half:])), (x[:n], x[:m]), (related(rng, x, n, alpha), x[-m:]),
             (rand_seq(rng, 1, alpha), rand_seq(rng, m, alpha)), (rand_seq(rng, n, alpha), rand_seq(rng, 1, alpha))]
    seqs = [s for pr in pairs for s in pr]
    pa, pb = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
    assert max(len(seqs[a]) for a in pa) == n and max(len(seqs[b]) for b in pb) == m
    return seqs, pa, pb


def check(c, call, lst, scoring, want_name):
    """runs the list, asserts the reported kernel through want_name(name) and the results against the oracle -> the oracle's results"""
    seqs, pa, pb = lst
    name, bits, profile, got = run_named(c, call, seqs, pa, pb, scoring)
    assert want_name(name), (call, scoring, name)
    assert bits == 32 and profile == 0
    want = oracle_results(call, seqs, pa, pb, scoring)
    assert got == want, (call, scoring, name, mismatches(got, want, seqs, pa, pb))
    return want


# ------------------------------------------------------------------ hw4's packed key
DIST_SHAPES = [(2000, 2000), (3999, 1), (1, 3999), (3000, 1000), (127, 3873)]          # n + m == 4000: the key's dist field at its end
DIST_SCORINGS = [(1, -3, -1), (16, -16, -7), (16, -16, -16), (-16, 16, 16), (1, 1, 1), (16, 15, 16), (-14, -15, -16)]
PACKED = re.compile(r"batch_nwdist_kernel<R=(64|128),PACKED>")
PLAIN_DIST = re.compile(r"batch_nwdist_kernel<R=(32|64),SC_PERM>")


def packed_ok(n, m, scoring):
    """choose_cell_form's rule for the packed key"""
    return n + m <= 4000 and (n + m + 2) * max(abs(s) for s in scoring) < 65536


@pytest.mark.parametrize("height", [64, 128])
@pytest.mark.parametrize("n,m", DIST_SHAPES)
def test_packed_distances_at_the_length_bound(n, m, height):
    """n + m == 4000 runs the packed key at both of its strip heights; the same list with its longest pattern one symbol longer runs
    the two-value form (R = 64 has both; the call is not refused, 4001 is simply outside the key)"""
    seqs, pa, pb = shape_list(n, m, b"ACGT", 4000)
    longer = [s + b"A" if k == pa[0] else s for k, s in enumerate(seqs)]
    with switched_context(PWA_FORCE_R=str(height), **STRIPS) as c:
        for sc in DIST_SCORINGS:
            check(c, "nwdist", (seqs, pa, pb), sc, lambda name: name == "batch_nwdist_kernel<R=%d,PACKED>" % height)
            if height == 64:
                check(c, "nwdist", (longer, pa, pb), sc, lambda name: name == "batch_nwdist_kernel<R=64,SC_PERM>")


def dist_scorings(a):
    """max |score| == a through each term in turn, and through all three, on both sides of zero"""
    sc = [(a, -1, -1), (1, -a, -1), (1, -1, -a), (a, -a, -a), (-a, a, a), (a, a - 1, a)]
    assert all(max(abs(s) for s in x) == a for x in sc)
    return sc


@pytest.mark.parametrize("n,m,a", [(1926, 1927, 17), (3726, 127, 17), (2000, 2000, 16), (127, 3873, 16)])
def test_packed_distances_at_the_product_bound(n, m, a):
    """(n + m + 2) * a is the last product below 65 536 (3855 * 17 = 65 535, 4002 * 16 = 64 032): the packed key; a + 1 is outside"""
    assert (n + m + 2) * a < 65536 <= (n + m + 2) * (a + 1) and n + m <= 4000
    lst = shape_list(n, m, b"ACGT", a)
    with switched_context(**STRIPS) as c:
        for sc in dist_scorings(a):
            check(c, "nwdist", lst, sc, PACKED.fullmatch)
        for sc in dist_scorings(a + 1):
            check(c, "nwdist", lst, sc, PLAIN_DIST.fullmatch)


# ------------------------------------------------------------------ hw3 and gotoh NW: shifted against plain
SPAN = 508                                                     # max_n + max_m: max_n + max_m + 4 == 512
AFF_SHAPES = [(254, 254), (4, 504), (504, 4), (127, 381)]
A_IN = ((1 << 27) - 1) // (4 * (SPAN + 4))                     # 65 535: the largest A inside the rule


def hw3_scorings(a, path):
    """A == a through each term the score path allows.  SC_PERM keeps its two cell scores in a byte table -- match - 2 gap_extend and
    mismatch - 2 gap_extend in the shifted form -- so there only gap_open can be large; SC_CMP takes any.  hw3 admits positive gap
    scores: a sentinel that is extended along a row then climbs instead of falling."""
    if path == "SC_PERM":
        sc = [(1, -1, -a, -1), (2, -3, -a, -60), (1, -1, a, 1), (2, -3, a, 60), (1, -1, a, -60)]
    else:
        sc = [(a, -1, -1, -1), (1, -a, -1, -1), (1, -1, -a, -1), (1, -1, 0, -a), (a, -a, -a, -a), (1, -1, a, 1), (1, -1, 0, a), (1, -1, a, a)]
    assert all(max(abs(s) for s in x) == a for x in sc)
    return sc


def gotoh_scorings(a, path):
    """the same for the gotoh call, whose gap terms are <= 0"""
    if path == "SC_PERM":
        sc = [(1, -1, -a, -1), (2, -3, -a, -60), (3, -4, -a, 0)]
    else:
        sc = [(a, -1, -1, -1), (1, -a, -1, -1), (1, -1, -a, -1), (1, -1, 0, -a), (a, -a, -a, -a)]
    assert all(max(abs(s) for s in x) == a for x in sc)
    return sc


@pytest.mark.parametrize("path", ["SC_PERM", "SC_CMP"])
@pytest.mark.parametrize("call,narrow,wide,scorings", [("affine", "BM_AFFS", "BM_AFF", hw3_scorings), ("gotoh nw", "BM_GNWS", "BM_GNW", gotoh_scorings)])
def test_shifted_affine_forms_at_their_bound(call, narrow, wide, scorings, path):
    """max_n + max_m + 4 == 512: A == 65 535 is the last scoring of the shifted form, 65 536 the first of the plain one.  The lists do
    sit at the bound: where gap_extend carries A, the oracle's scores come within 3 % of (max_n + max_m) * A in size (4 x 504: 500
    gap columns).  A match term reaches half of that (254 x 254: the whole diagonal).  Where only gap_open can carry A
    (SC_PERM, above) a score holds it once per gap: hw3 opens a gap only after a diagonal step, so a positive gap_open is collected
    in every third column, a third of (max_n + max_m) * A; a negative one reaches -A and little more.  Each is asserted as such."""
    assert 4 * (SPAN + 4) * A_IN < 1 << 27 <= 4 * (SPAN + 4) * (A_IN + 1) and A_IN == 65535
    lists = [shape_list(n, m, b"ACGT" if path == "SC_PERM" else LETTERS, 512) for n, m in AFF_SHAPES]
    for seqs, pa, pb in lists:
        assert (len(set(b"".join(seqs[b] for b in pb))) > 7) == (path == "SC_CMP")   # the texts' alphabet picks the score path
    largest = {}
    with switched_context(**STRIPS) as c:
        for a, form in ((A_IN, narrow), (A_IN + 1, wide)):
            for sc in scorings(a, path):
                for lst in lists:
                    want = check(c, call, lst, sc, lambda name: mode_of(name) == (form, path))
                    if a == A_IN:
                        largest[sc] = max(largest.get(sc, 0), max(abs(w) for w in want))
    for sc, top in largest.items():
        match, mismatch, go, ge = sc
        if abs(ge) == A_IN:
            assert top > 0.97 * SPAN * A_IN, (sc, top)
        elif call == "affine" and go == A_IN and ge > 0:
            assert top > 0.32 * SPAN * A_IN, (sc, top)         # a gap in every third column
        elif match == A_IN:
            assert top > 0.49 * SPAN * A_IN, (sc, top)         # 254 x 254: every cell of the diagonal a match
        elif abs(go) == A_IN:
            assert top >= A_IN, (sc, top)
        else:                                                  # a mismatch of -A: gap columns walk around it, it enters cells and wins next to none
            assert -mismatch == A_IN, sc


# ------------------------------------------------------------------ linear NW: gap-shifted against plain
def test_gap_shifted_nw_at_the_byte_rule():
    """match - 2 gap == 127 against 128, mismatch - 2 gap == -128 against -129, with gaps of both signs"""
    lists = [shape_list(n, m, b"ACGT", 127) for n, m in AFF_SHAPES] + [shape_list(254, 254, LETTERS, 127)]
    inside = [(107, -3, -10), (5, -148, -10), (147, 3, 10), (-5, -108, 10), (107, -148, -10), (127, -128, 0)]
    outside = [(108, -3, -10), (5, -149, -10), (148, 3, 10), (-5, -109, 10), (128, -128, 0), (127, -129, 0)]
    for m, x, g in inside:
        assert -128 <= x - 2 * g and m - 2 * g <= 127 and (m - 2 * g == 127 or x - 2 * g == -128)
    for m, x, g in outside:
        assert m - 2 * g == 128 or x - 2 * g == -129
    with switched_context(**STRIPS) as c:
        for scs, form in ((inside, "BM_NWG"), (outside, "BM_NW")):
            for sc in scs:
                for lst in lists:
                    check(c, "nw", lst, sc, lambda name: mode_of(name)[0] == form)


def test_gap_shifted_nw_at_the_magnitude_rule():
    """max_n + max_m + 4 == 512: A == 524 287 is the last scoring of the gap-shifted form.  Match and mismatch have to lie within a
    byte of 2 gap, so A is one of them and |gap| about half of it: the scores reach half of (max_n + max_m) * A (508 gap columns, or
    254 mismatches)."""
    a_in = ((1 << 30) - 1) // (4 * (SPAN + 4))
    assert 4 * (SPAN + 4) * a_in < 1 << 30 <= 4 * (SPAN + 4) * (a_in + 1) and a_in == 524287
    g = (a_in - 3) // 2                                          # 2 g + 3 == A
    assert 2 * g + 3 == a_in
    inside = [(-2 * g + 5, -2 * g - 3, -g), (2 * g + 3, 2 * g - 4, g), (-2 * g - 3, -2 * g - 3, -g)]
    outside = [(-2 * g + 5, -2 * g - 4, -g), (2 * g + 4, 2 * g - 4, g), (-2 * g - 4, -2 * g - 3, -g)]
    assert all(max(abs(s) for s in sc) == a_in for sc in inside) and all(max(abs(s) for s in sc) == a_in + 1 for sc in outside)
    lists = [shape_list(n, m, b"ACGT", 30) for n, m in AFF_SHAPES] + [shape_list(254, 254, LETTERS, 30)]
    top = 0
    with switched_context(**STRIPS) as c:
        for scs, form in ((inside, "BM_NWG"), (outside, "BM_NW")):
            for sc in scs:
                for lst in lists:
                    want = check(c, "nw", lst, sc, lambda name: mode_of(name)[0] == form)
                    top = max(top, max(abs(w) for w in want))
    assert top > 0.49 * SPAN * a_in
