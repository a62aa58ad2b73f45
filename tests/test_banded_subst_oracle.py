"""The banded oracle (banded_oracle.py) under a substitution table against a scalar three-matrix DP with a band mask, float -inf and the
table; against its own byte compare where the table is match on the diagonal and mismatch off it; and against gotoh_oracle under the
same table where the band covers the whole matrix."""
import random

import numpy as np
import pytest

import banded_oracle as BO
import gotoh_oracle as GO
from conftest import load_pkg
from gotoh_oracle import random_table

MODES = ["nw", "sw", "sg"]
GAPS = [(-5, -2), (-1, -1), (0, -3)]
ALPHA = b"ACGN"


def _rand(rng, n, alpha=ALPHA):
    return bytes(rng.choice(alpha) for _ in range(n))


def _pairs(rng, count, lo_len=1, alpha=ALPHA):
    out = []
    for _ in range(count):
        n = rng.randint(lo_len, 24)
        m = n if rng.random() < 0.3 else rng.randint(lo_len, 24)
        t = _rand(rng, m, alpha)
        p = bytes(x if rng.random() < 0.8 else rng.choice(alpha) for x in (t * 2)[:n]) if rng.random() < 0.7 else _rand(rng, n, alpha)
        out.append((p, t))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", GAPS)
def test_against_scalar_dp(mode, gaps):
    """150 tiny pairs with random valid bands (width 1 among them) under an asymmetric table with positive off-diagonal entries"""
    rng = random.Random(MODES.index(mode) * 10 + GAPS.index(gaps))
    table = random_table(7 + GAPS.index(gaps), ALPHA, lo=-5, hi=6)
    M = np.asarray(table[2]).reshape(4, 4)
    assert (M != M.T).any() and (M[~np.eye(4, dtype=bool)] > 0).any()
    pairs = _pairs(rng, 150, lo_len=0)
    bands = [BO.random_band(rng, mode, len(p), len(t)) for p, t in pairs]
    assert any(lo == hi for lo, hi in bands)
    got = BO.align_many(pairs, bands, mode, table, *gaps)
    for (p, t), b, g in zip(pairs, bands, got):
        assert g == BO.scalar_dp(p, t, b, mode, table, *gaps), (mode, p, t, b)
        if len(p) and len(t) and (mode != "sw" or g["ops"]):
            assert BO.ops_in_band(g["ops"], g["start"], b)
            assert GO.op_score(p, t, g["ops"], g["start"], table, *gaps) == g["score"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sc", [(1, -4, -6, -1), (2, 1, -3, -1), (0, 0, 0, 0)])
def test_match_mismatch_table_is_the_banded_oracle(mode, sc):
    match, mismatch, go, ge = sc
    table = load_pkg().subst_table(ALPHA, np.where(np.eye(4, dtype=bool), match, mismatch))
    rng = random.Random(3 + MODES.index(mode))
    pairs = _pairs(rng, 120, lo_len=0)
    bands = [BO.random_band(rng, mode, len(p), len(t)) for p, t in pairs]
    assert BO.align_many(pairs, bands, mode, table, go, ge) == BO.align_many(pairs, bands, mode, (match, mismatch), go, ge)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", GAPS)
def test_full_cover_is_the_subst_oracle(mode, gaps):
    table = random_table(11, ALPHA, lo=-5, hi=6)
    rng = random.Random(5 + MODES.index(mode))
    pairs = _pairs(rng, 120, lo_len=0)
    bands = [(-len(p), len(t)) for p, t in pairs]
    assert BO.align_many(pairs, bands, mode, table, *gaps) == GO.align_many(pairs, mode, table, *gaps)
