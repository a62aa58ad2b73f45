"""The three stripe-engine routes behind a range guard, at the guard: hw3's affine scores and hw4's distances (route_eligible,
pwalign.hip: (max_n + max_m + 2) * A < 2^28 over the list's longest first and second sequences) and hw3's affine alignments
(split_off_stripe_pairs, pwalign_affine_tb.hip: the same product below 2^26).  A = max(|match|, |mismatch|, |gap_open| + |gap_extend|, 1)
for hw3, max(|match|, |mismatch|, |gap|, 1) for hw4.  At A_in, the largest A inside the guard, the list runs on the stripe engine and
equals the oracle; at A_in + 1 it stays on the strips and equals it too.

One list per route: lengths 129, 513 and 1025 (more than one stripe, more than one workgroup), an identical pair (the largest
positive values), AC against GT (the most negative), 10 % mutated pairs, 1 x 1025 and 1025 x 1.

The two score routes read a coded arena with their two cell scores in a byte table, which the host builds only where those constants
fit a byte (choose_cell_form: match and mismatch for hw3, match - gap and mismatch - gap for hw4).  So hw3's score route reaches its
guard through the gap term alone -- with match or mismatch at A_in the list stays on the strips, which is asserted, exact -- and hw4
reaches it with all three scores within a byte of each other, each of them the largest in turn."""
import random

import pytest

import oracle_lib as O
from conftest import switched_context
from test_gpu_hw3_align_long import check_exact, mutate, stripe_pairs

pytestmark = pytest.mark.gpu

AFF_STRIPE, AFF_STRIP = "pair_affine_kernel<", "batch_affine_kernel"
DIST_STRIPE, DIST_STRIP = "pair_dist_kernel<", "batch_nwdist"


def guard_list():
    rng = random.Random(521)
    rnd = lambda n, alpha=b"ACGT": bytes(rng.choice(alpha) for _ in range(n))   # noqa: E731
    seqs, pa, pb = [], [], []

    def add(a, b):
        seqs.extend([a, b])
        pa.append(len(seqs) - 2)
        pb.append(len(seqs) - 1)
    s = rnd(1025)
    seqs.append(s)
    pa.append(0)
    pb.append(0)                                     # the identical pair
    add(rnd(1025, b"AC"), rnd(1025, b"GT"))
    for n in (129, 513, 1025):
        base = rnd(n)
        add(base, (mutate(rng, base, 0.1, b"ACGT") + rnd(n))[:n])
    add(rnd(1), rnd(1025))
    add(rnd(1025), rnd(1))
    assert max(len(seqs[a]) for a in pa) == max(len(seqs[b]) for b in pb) == 1025 and len(pa) < 20
    return seqs, pa, pb


def a_in(bits):
    """the largest A inside the guard of the list above: its sizes are max_n + max_m + 2 = 2052"""
    a = ((1 << bits) - 1) // 2052
    assert 2052 * a < 1 << bits <= 2052 * (a + 1)
    return a


def hw3_scorings(a):
    """A = a through each term in turn, the others small, and through all of them at once; then the gap term with positive gap scores
    (hw3 admits them: a sentinel that is extended along a row then climbs instead of falling)
    -> {name: (match, mismatch, gap_open, gap_extend)}"""
    sc = {"match": (a, -1, -1, -1), "mismatch": (1, -a, -1, -1), "all terms": (a, -a, -(a // 2), -(a - a // 2)),
          "gaps": (1, -1, -(a // 2), -(a - a // 2)), "extend": (1, -1, 0, -a),
          "gaps positive": (1, -1, a // 2, a - a // 2), "extend positive": (1, -1, 0, a)}
    assert all(max(abs(m), abs(x), abs(go) + abs(ge)) == a for m, x, go, ge in sc.values())
    return sc


def aff_kernel(c, seqs, pa, pb, sc):
    b = c.batch_affine(seqs, pa, pb, *sc)
    kern = b.info()["kernel"]
    b.close()
    return kern


@pytest.fixture(scope="module")
def hw3_want():
    """the oracle's scores of the list, per scoring (computed once)"""
    seqs, pa, pb = guard_list()
    memo = {}

    def want(sc):
        if sc not in memo:
            memo[sc] = [O.affine_score(seqs[a], seqs[b], *sc) for a, b in zip(pa, pb)]
        return memo[sc]
    return want


def test_hw3_score_route_at_its_guard(hw3_want):
    seqs, pa, pb = guard_list()
    a = a_in(28)
    with switched_context(PWA_SCORES_ROUTE="1") as c:
        for name, sc in hw3_scorings(a).items():
            kern = aff_kernel(c, seqs, pa, pb, sc)
            if name in ("match", "mismatch", "all terms"):   # no byte table for these: the strips, whatever the guard says
                assert kern.startswith(AFF_STRIP) and AFF_STRIPE not in kern, (name, kern)
            else:
                assert kern.startswith(AFF_STRIPE) and AFF_STRIP not in kern, (name, kern)
            got, want = c.scores_affine(seqs, pa, pb, *sc), hw3_want(sc)
            assert got == want, (name, sc, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w])
        # (the stripe engine's values do reach the guard's size: 2050 gap columns at +A, and the 1 x 1025 pair's one gap at -A)
        assert max(hw3_want(hw3_scorings(a)["extend positive"])) > 0.99 * (1 << 28) and min(hw3_want(hw3_scorings(a)["extend"])) < -0.49 * (1 << 28)
        for name, sc in hw3_scorings(a + 1).items():
            kern = aff_kernel(c, seqs, pa, pb, sc)
            assert kern.startswith(AFF_STRIP) and AFF_STRIPE not in kern, (name, kern)
            got, want = c.scores_affine(seqs, pa, pb, *sc), hw3_want(sc)
            assert got == want, (name, sc, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w])


def test_hw3_alignment_route_at_its_guard():
    seqs, pa, pb = guard_list()
    a = a_in(26)
    with switched_context(PWA_AFFINE_TB_ROUTE="1") as c:
        for name, sc in hw3_scorings(a).items():
            check_exact(c, seqs, pa, pb, sc)
            assert stripe_pairs(c) == len(pa), (name, sc)
        for name, sc in hw3_scorings(a + 1).items():
            check_exact(c, seqs, pa, pb, sc)
            assert stripe_pairs(c) == 0, (name, sc)


def hw4_scorings(a):
    """A = a through each term in turn with the other two within a byte of it (match - gap and mismatch - gap are the table's
    constants), on the positive and on the negative side -> {name: (match, mismatch, gap)}"""
    sc = {"match": (a, a - 3, a - 2), "mismatch": (-a + 3, -a, -a + 1), "gap": (-a + 2, -a + 1, -a), "gap positive": (a - 1, a - 3, a)}
    for name, (m, x, g) in sc.items():
        assert max(abs(m), abs(x), abs(g)) == a == abs(dict(match=m, mismatch=x, gap=g)[name.split()[0]])
        assert -128 <= m - g <= 127 and -128 <= x - g <= 127
    return sc


def test_hw4_distance_route_at_its_guard():
    seqs, pa, pb = guard_list()
    a = a_in(28)
    memo = {}

    def want(sc):
        if sc not in memo:
            memo[sc] = [O.nw_distance(seqs[x], seqs[y], *sc) for x, y in zip(pa, pb)]
        return memo[sc]
    with switched_context(PWA_SCORES_ROUTE="1", PWA_NO_PACKED_DIST="1") as c:
        for a_, on_stripes in ((a, True), (a + 1, False)):
            for name, sc in hw4_scorings(a_).items():
                b = c.batch_distances(seqs, pa, pb, *sc)
                kern = b.info()["kernel"]
                b.close()
                if on_stripes:
                    assert kern.startswith(DIST_STRIPE) and DIST_STRIP not in kern, (name, kern)
                else:
                    assert kern.startswith(DIST_STRIP) and DIST_STRIPE not in kern, (name, kern)
                got = c.distances(seqs, pa, pb, *sc)
                assert got == [d for d, _ in want(sc)], (name, sc, [(k, g, w) for k, (g, w) in enumerate(zip(got, want(sc))) if g != w[0]])
        # the scores behind these distances do sit at the guard: all-gap alignments of 2050 columns, and 1025 mismatches
        assert max(s for _, s in want(hw4_scorings(a)["match"])) > 0.99 * (1 << 28)
        assert min(s for _, s in want(hw4_scorings(a)["mismatch"])) < -0.49 * (1 << 28)
