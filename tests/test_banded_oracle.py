"""The banded oracle (banded_oracle.py) against a scalar three-matrix DP with a band mask and float -inf, and against gotoh_oracle
wherever the band cannot matter: a band that covers the matrix, and the band spanned by the unbanded walk (the identity property of
include/pwalign.h)."""
import random

import pytest

import banded_oracle as BO
import gotoh_oracle as GO

SCORINGS = [((1, -1), -1, -1), ((2, -3), -5, -2)]   # ((match, mismatch), gap_open, gap_extend)
ALPHA = b"ACG"


def _rand(rng, n):
    return bytes(rng.choice(ALPHA) for _ in range(n))


def _pairs(seed, count, lo_len=1):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randint(lo_len, 24)
        m = n if rng.random() < 0.3 else rng.randint(lo_len, 24)
        t = _rand(rng, m)
        p = bytes(x if rng.random() < 0.8 else rng.choice(ALPHA) for x in (t * 2)[:n]) if rng.random() < 0.7 else _rand(rng, n)
        out.append((p, t))
    return out


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("sc", SCORINGS)
def test_against_scalar_dp(mode, sc):
    rng = random.Random(["nw", "sw", "sg"].index(mode) * 10 + SCORINGS.index(sc))
    pairs = _pairs(rng.randint(0, 1 << 30), 150, lo_len=0)
    bands = [BO.random_band(rng, mode, len(p), len(t)) for p, t in pairs]
    assert any(lo == hi for lo, hi in bands)
    got = BO.align_many(pairs, bands, mode, *sc)
    for (p, t), b, g in zip(pairs, bands, got):
        assert g == BO.scalar_dp(p, t, b, mode, *sc), (mode, p, t, b)
        if len(p) and len(t) and (mode != "sw" or g["ops"]):   # (SW without a positive in-band cell ends at (0, 0), in the band or not)
            assert BO.ops_in_band(g["ops"], g["start"], b)
            assert GO.op_score(p, t, g["ops"], g["start"], *sc) == g["score"]


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("sc", SCORINGS)
def test_full_cover_and_walk_band_equal_gotoh(mode, sc):
    pairs = _pairs(100 + ["nw", "sw", "sg"].index(mode) * 10 + SCORINGS.index(sc), 120)
    want = [GO.align(p, t, mode, *sc) for p, t in pairs]
    full = [(-len(p), len(t)) for p, t in pairs]
    assert BO.align_many(pairs, full, mode, *sc) == want
    tight = [BO.walk_diagonals(w["ops"], w["start"]) for w in want]
    if mode != "sw":   # (row 0 / column 0 reach (0, 0) for NW; SG's walk ends on row 0: its own diagonal is in the range)
        tight = [(min(lo, 0), max(hi, 0)) if mode == "nw" else (lo, max(hi, 0)) for lo, hi in tight]
    for (p, t), b in zip(pairs, tight):
        assert BO.band_valid(mode, len(p), len(t), *b)
    assert BO.align_many(pairs, tight, mode, *sc) == want
