"""CPU checks of the affine-gap (gotoh) numpy oracle: against a plain three-matrix DP, against the linear oracles at gap_open = 0,
and the affine score of every op list against the returned score."""
import random

import numpy as np
import pytest

import gotoh_oracle as GO
import oracle_lib as O
import sg_oracle as SG

SCORINGS = [(1, -4, -6, -1), (2, -3, -5, -2), (5, -4, -16, -4), (1, -1, -1, -1), (0, 0, 0, 0), (3, -1, 0, -2)]


def _rand(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("sc", SCORINGS)
def test_oracle_matches_scalar_dp(mode, sc):
    rng = random.Random(hash((mode, sc)) & 0xffff)
    match, mismatch, go, ge = sc
    for _ in range(12):
        n, m = rng.randint(1, 14), rng.randint(1, 14)
        p, t = _rand(rng, n, b"AC"), _rand(rng, m, b"ACG")
        tab = GO.fill(GO._arr(p)[None, :], GO._arr(t)[None, :], mode, match, mismatch, go, ge)
        H, src, eop, fop = GO.scalar_dp(p, t, mode, match, mismatch, go, ge)
        assert tab["H"][0].tolist() == H
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                assert tab["src"][0][i, j] == src[i][j], (i, j)
                assert bool(tab["eop"][0][i, j]) == eop[i][j], (i, j)
                assert bool(tab["fop"][0][i, j]) == fop[i][j], (i, j)


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("sc", SCORINGS)
def test_op_scores_equal_scores(mode, sc):
    rng = random.Random(7 + len(mode))
    match, mismatch, go, ge = sc
    pairs = [(_rand(rng, rng.randint(0, 40)), _rand(rng, rng.randint(0, 60))) for _ in range(40)]
    for (p, t), r in zip(pairs, GO.align_many(pairs, mode, match, mismatch, go, ge)):
        assert GO.op_score(p, t, r["ops"], r["start"], match, mismatch, go, ge) == r["score"]
        n_m = sum(1 for o in r["ops"] if o in (77, 68))
        assert r["start"][0] + n_m == r["end"][0]


@pytest.mark.parametrize("mode", ["nw", "sw"])
@pytest.mark.parametrize("sc", [(1, -1, -1), (2, -3, -2), (1, -4, -1), (0, 0, 0)])
def test_gap_open_zero_is_the_linear_mode(mode, sc):
    rng = random.Random(11)
    match, mismatch, gap = sc
    for _ in range(25):
        p, t = _rand(rng, rng.randint(1, 50)), _rand(rng, rng.randint(1, 70))
        want = O.align(mode, p, t, match, mismatch, gap)
        got = GO.align(p, t, mode, match, mismatch, 0, gap)
        assert got["score"] == want["score"]
        assert got["ops"] == want["ops"]
        assert got["end"] == tuple(want["end"])


@pytest.mark.parametrize("sc", [(1, -1, -1), (2, -3, -2), (0, 0, 0)])
def test_gap_open_zero_is_semiglobal(sc):
    rng = random.Random(12)
    match, mismatch, gap = sc
    for _ in range(25):
        p, t = _rand(rng, rng.randint(1, 40)), _rand(rng, rng.randint(1, 90))
        want = SG.align(p, t, match, mismatch, gap)
        got = GO.align(p, t, "sg", match, mismatch, 0, gap)
        assert (got["score"], got["end"], got["start"], got["ops"]) == (want["score"], want["end"], want["start"], want["ops"])


def test_prefixes_equal_own_fills():
    rng = random.Random(5)
    p, t = _rand(rng, 30), _rand(rng, 80)
    for mode in ("nw", "sw", "sg"):
        ms = [0, 1, 17, 50, 80]
        for m, r in zip(ms, GO.prefixes(p, t, ms, mode, 2, -3, -5, -2)):
            assert r == GO.align(p, t[:m], mode, 2, -3, -5, -2)


def test_one_event_is_one_gap():
    """12 text bases missing from a read come back as one 'I' run (text-only columns) under affine scoring."""
    rng = random.Random(3)
    region = _rand(rng, 400)
    read = region[100:160] + region[172:250]   # 12 bases deleted
    r = GO.align(read, region, "sg", 1, -4, -6, -1)
    ops = bytes(reversed(r["ops"]))
    assert b"I" * 12 in ops and ops.count(b"I") == 12 and b"D" not in ops
    assert r["score"] == len(read) - 6 - 12
