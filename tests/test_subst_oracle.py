"""CPU checks of gotoh_oracle.py under a substitution table: it is its own byte compare when the matrix is match on the diagonal and
mismatch elsewhere, it equals a plain three-matrix DP on random asymmetric matrices in all three modes, the score of every op list
under the matrix equals the returned score, and subst_table builds the map and matrix the oracle and the library take."""
import random

import numpy as np
import pytest

import gotoh_oracle as GO
from conftest import load_pkg
from gotoh_oracle import random_table

MODES = ["nw", "sw", "sg"]
GAPS = [(-11, -1), (0, -3), (-6, -1), (-2, 0), (0, 0)]


def _rand(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sc", [(1, -4, -6, -1), (5, -4, -16, -4), (2, 1, -3, -1), (0, 0, 0, 0), (1, -1, 0, -2)])
def test_match_mismatch_matrix_is_the_gotoh_oracle(mode, sc):
    match, mismatch, go, ge = sc
    table = load_pkg().subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), match, mismatch))
    rng = random.Random(3)
    pairs = [(_rand(rng, rng.randint(0, 40)), _rand(rng, rng.randint(0, 60))) for _ in range(30)]
    assert GO.align_many(pairs, mode, table, go, ge) == GO.align_many(pairs, mode, (match, mismatch), go, ge)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", GAPS)
def test_oracle_matches_scalar_dp(mode, gaps):
    go, ge = gaps
    rng = random.Random(len(mode) * 100 + go * 7 + ge)
    for trial in range(10):
        alpha = b"ACGTN"[:rng.randint(1, 5)]
        table = random_table(trial, alpha, lo=-5, hi=6)
        n, m = rng.randint(1, 14), rng.randint(1, 14)
        p, t = _rand(rng, n, alpha), _rand(rng, m, alpha)
        tab = GO.fill(GO._arr(p)[None, :], GO._arr(t)[None, :], mode, table, go, ge)
        H, src, eop, fop = GO.scalar_dp(p, t, mode, table, go, ge)
        assert tab["H"][0].tolist() == H
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                assert tab["src"][0][i, j] == src[i][j], (i, j)
                assert bool(tab["eop"][0][i, j]) == eop[i][j], (i, j)
                assert bool(tab["fop"][0][i, j]) == fop[i][j], (i, j)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", GAPS)
def test_op_scores_equal_scores(mode, gaps):
    go, ge = gaps
    alpha = b"ACDEFGHIKLMNPQRSTVWY"
    table = random_table(5, alpha)
    rng = random.Random(9)
    pairs = [(_rand(rng, rng.randint(0, 40), alpha), _rand(rng, rng.randint(0, 60), alpha)) for _ in range(30)]
    for (p, t), r in zip(pairs, GO.align_many(pairs, mode, table, go, ge)):
        assert GO.op_score(p, t, r["ops"], r["start"], table, go, ge) == r["score"]


def test_the_matrix_row_is_the_pattern():
    """s(a, b) != s(b, a): the oracle reads M[pattern code, text code], not the transpose"""
    table = load_pkg().subst_table(b"AB", [[1, 5], [-7, 1]])
    assert GO.align(b"A", b"B", "nw", table, -20, -1)["score"] == 5
    assert GO.align(b"B", b"A", "nw", table, -20, -1)["score"] == -7


def test_subst_table():
    pkg = load_pkg()
    code, n_sym, submat = pkg.subst_table("ACGTN", np.arange(25).reshape(5, 5), unknown=4, fold_case=True)
    assert n_sym == 5 and code.dtype == np.uint8 and code.shape == (256,) and submat.dtype == np.int32
    assert submat.tolist() == list(range(25))
    assert [code[b] for b in b"ACGTNacgtn"] == [0, 1, 2, 3, 4] * 2
    assert code[0] == code[ord("-")] == code[ord("x")] == 4
    code, _, _ = pkg.subst_table(b"Aa", [[1, 0], [0, 1]], unknown=0, fold_case=True)   # both cases in the alphabet keep their own codes
    assert (code[ord("A")], code[ord("a")]) == (0, 1)
    code, _, _ = pkg.subst_table(b"AC", [[1, 0], [0, 1]])
    assert code[ord("A")] == 0 and code[ord("C")] == 1 and code[ord("G")] >= 2   # no code: the call that gets such a byte raises
    for bad in (lambda: pkg.subst_table(b"", []), lambda: pkg.subst_table(b"AA", [[1, 0], [0, 1]]),
                lambda: pkg.subst_table(b"AC", [[1, 0, 0], [0, 1, 0]]), lambda: pkg.subst_table(b"AC", [[1, 0], [0, 1]], unknown=2),
                lambda: pkg.subst_table(bytes(range(33)), np.zeros((33, 33), int))):
        with pytest.raises(ValueError):
            bad()
