"""Integer-coded row of the packed profile form on the device (batch_scores.hip.h, PROF16 with INT = true; PWA_PROF16_INT): every
case runs the integer row (PWA_PROF16_INT=1) and the f16 row (=0) of the same list, compares them element for element and both
with the oracle.  Scorings with mismatch < gap or match < gap must report profile_int() == 0 and stay exact on the f16 row."""
import random

import numpy as np
import pytest

import oracle_lib as O
from conftest import switched_context


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def admitted(scoring):
    match, mismatch, gap = scoring
    return mismatch - gap >= 0 and match - gap >= 0


def run(knob, seqs, pa, pb, scoring):
    with switched_context(PWA_SCORES_ROUTE="0", PWA_FORCE_LANES="0", PWA_CELL16="1", PWA_PROF16="1", PWA_PROF16_INT=knob) as c:
        b = c.batch("sw", seqs, pa, pb, *scoring)
        forms = (b.profile_form(), b.cell_bits(), b.profile_int(), b.info()["kernel"])
        b.run()
        got = b.fetch()
        b.close()
    return got, forms


def check(seqs, pa, pb, scoring, sample=None):
    got1, (form1, bits1, int1, kern1) = run("1", seqs, pa, pb, scoring)
    got0, (form0, bits0, int0, kern0) = run("0", seqs, pa, pb, scoring)
    assert (form1, bits1, form0, bits0) == (1, 16, 1, 16), (scoring, form1, bits1, form0, bits0)
    assert int1 == (1 if admitted(scoring) else 0) and int0 == 0, (scoring, int1, int0)
    assert kern1 == kern0   # the reported name does not tell the rows apart
    assert got1 == got0, (scoring, [k for k in range(len(pa)) if got1[k] != got0[k]][:5])
    ks = range(len(pa)) if sample is None else random.Random(1).sample(range(len(pa)), sample)
    want = lambda k: O.score("sw", seqs[pa[k]], seqs[pb[k]], *scoring)[0] if seqs[pa[k]] and seqs[pb[k]] else 0
    bad = [k for k in ks if got1[k] != want(k)]
    assert not bad, (scoring, bad[:5])


def all_pairs(n_p, n_t):
    return [i for i in range(n_p) for _ in range(n_t)], [n_p + j for _ in range(n_p) for j in range(n_t)]


@pytest.mark.gpu
def test_profile_shapes_on_both_sides_of_the_admission(ctx):
    """the lists of test_gpu_scores_profile.py: patterns of 1..152 rows, texts of every length residue mod 8, partial tasks;
    scorings with mismatch >= gap (integer row) and mismatch < gap (f16 row)"""
    rng = random.Random(505)
    lens = list(range(1, 153, 7)) + [150, 151, 152]
    pats = [rand_seq(rng, n) for n in lens]
    txts = [rand_seq(rng, m) for m in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257, 1001, 1002, 1003)]
    pa, pb = all_pairs(len(pats), len(txts))
    for scoring in [(1, -1, -1), (2, -3, -5), (5, -4, -4), (1, 0, 0), (0, -1, -1), (3, -2, -2), (13, -20, -2), (2, -3, -1), (5, -4, 0)]:
        check(pats + txts, pa, pb, scoring)


@pytest.mark.gpu
def test_row_and_column_edges(ctx):
    """patterns of 1 and 149..152 rows; texts of 0, 1, 7, 8, 9 and ~10 000 columns; an odd number of texts per pattern"""
    rng = random.Random(612)
    pats = [rand_seq(rng, n) for n in (1, 149, 150, 151, 152)]
    txts = [rand_seq(rng, m) for m in (0, 1, 7, 8, 9, 9999, 10000)]
    pa, pb = all_pairs(len(pats), len(txts))
    for scoring in [(1, -1, -1), (2, -3, -5), (13, -20, -2)]:
        check(pats + txts, pa, pb, scoring)


@pytest.mark.gpu
def test_single_text_and_odd_task_sizes(ctx):
    """tasks of 1 text (pair B of lane 0 and 63 lanes empty), of 129 texts (a second task of one) and of 65 (one pair B)"""
    rng = random.Random(613)
    pats = [rand_seq(rng, 150), rand_seq(rng, 77), rand_seq(rng, 12)]
    for n_t in (1, 65, 129):
        txts = [rand_seq(rng, rng.randint(1, 400)) for _ in range(n_t)]
        pa, pb = all_pairs(len(pats), n_t)
        for scoring in [(1, -1, -1), (7, -7, -7)]:
            check(pats + txts, pa, pb, scoring)


@pytest.mark.gpu
def test_scores_at_the_bound_and_extreme_gaps(ctx):
    """a pair whose score is 2047 (match 23 x 89 rows), 127 x 16 rows, gap = -127 and gap = 0; repeated texts (many equal maxima)"""
    rng = random.Random(614)
    base = rand_seq(rng, 150)
    pats = [base, rand_seq(rng, 150), b"A" * 150, rand_seq(rng, 89)]
    txts = [base * 3, base[:75] + base[:75], b"A" * 400] + [rand_seq(rng, rng.randint(100, 700)) for _ in range(70)]
    pa, pb = all_pairs(len(pats), len(txts))
    for scoring in [(23, -1, -1), (13, -127, -127), (1, -127, -127), (127, -127, -127), (127, 0, -127), (23, 0, 0), (23, -5, 0)]:
        n = 2047 // scoring[0]
        p2 = [p[:n] for p in pats]
        check(p2 + txts, pa, pb, scoring)
    got, _ = run("1", [base[:89], base], [0], [1], (23, -1, -1))
    assert got == [2047]


@pytest.mark.gpu
def test_default_takes_the_integer_row_where_admitted(ctx):
    rng = random.Random(615)
    pats = [rand_seq(rng, 150) for _ in range(4)]
    txts = [rand_seq(rng, 500) for _ in range(128)]
    pa, pb = all_pairs(4, 128)
    for scoring, want in [((1, -1, -1), 1), ((13, -20, -2), 0)]:
        with switched_context(PWA_SCORES_ROUTE="0", PWA_FORCE_LANES="0", PWA_CELL16="1", PWA_PROF16="1") as c:
            b = c.batch("sw", pats + txts, pa, pb, *scoring)
            assert b.profile_form() == 1 and b.profile_int() == want
            b.close()
    with switched_context(PWA_PROF16="0", PWA_SCORES_ROUTE="0", PWA_CELL16="1") as c:
        b = c.batch("sw", pats + txts, pa, pb, 1, -1, -1)
        assert b.profile_form() == 0 and b.profile_int() == 0   # no profile form: no integer row
        b.close()


@pytest.mark.gpu
def test_full_size_c3_with_the_integer_row(ctx):
    """C3 at full size with the integer row forced on: the bench line's checksum, a seeded sample against the oracle, and the f16 row
    of the same list element for element"""
    pats = [O.gen(1, 0, p, 150) for p in range(4096)]
    txts = [O.gen(1, 1, t, 10000) for t in range(256)]
    seqs = pats + txts
    pa = np.repeat(np.arange(4096, dtype=np.uint32), 256)
    pb = np.tile(np.arange(256, dtype=np.uint32) + np.uint32(4096), 4096)
    res = {}
    for knob in ("1", "0"):
        with switched_context(PWA_PROF16_INT=knob) as c:
            b = c.batch("sw", seqs, pa, pb, 1, -1, -1)
            assert b.profile_form() == 1 and b.cell_bits() == 16 and b.profile_int() == int(knob)
            assert b.info()["kernel"] == "batch_scores_kernel<R=76,BM_SWS,SC_PERM>", b.info()
            b.run()
            res[knob] = b.fetch(numpy_out=True)
            b.close()
    s = res["1"]
    assert int(s.astype(np.int64).sum()) == 35376135
    assert np.array_equal(s, res["0"]), int(np.count_nonzero(s != res["0"]))
    for k in np.random.default_rng(4).choice(len(pa), 128, replace=False):
        assert int(s[k]) == O.score("sw", seqs[pa[k]], seqs[pb[k]], 1, -1, -1)[0], k
