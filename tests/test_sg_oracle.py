"""The numpy semi-global oracle (sg_oracle.py) against the pinned C oracle of hw2.cpp's NW (CPU only).

Two facts tie the modes together (include/pwalign.h, PWA_MODE_SG): for gap <= 0 the SG score is the best NW score of the pattern
against any substring of the text, and for every scoring the walk's op scores sum to the SG score (dp[0][j0] = 0).  The tie-break
itself is checked cell by cell against the device's matrices in test_gpu_semiglobal.py."""
import random

import pytest

import oracle_lib as O
import sg_oracle as SG
from conftest import load_pkg
from test_gpu_cigar import SCORINGS


def test_mode_table_has_semiglobal():
    mode = load_pkg().MODE
    assert mode["sg"] == mode["semiglobal"] == 2
    assert (mode["nw"], mode["sw"]) == (0, 1)


def _pairs(seed, count, alpha=b"ACGT", n_max=9, m_max=12):
    rng = random.Random(seed)
    out = [(b"", b""), (b"", b"ACG"), (b"AC", b""), (b"A", b"A"), (b"A", b"C")]
    while len(out) < count:
        n, m = rng.randint(0, n_max), rng.randint(0, m_max)
        out.append((bytes(rng.choice(alpha) for _ in range(n)), bytes(rng.choice(alpha) for _ in range(m))))
    return out


@pytest.mark.parametrize("sc", [s for s in SCORINGS if s[2] <= 0])
def test_score_is_best_nw_over_substrings(sc):
    for p, t in _pairs(11, 60, alpha=b"AC-\x00G"):
        want = max(O.score("nw", p, t[a:b], *sc)[0] for a in range(len(t) + 1) for b in range(a, len(t) + 1))
        assert SG.align(p, t, *sc)["score"] == want, (p, t, sc)


@pytest.mark.parametrize("sc", SCORINGS)
def test_walk_scores_sum_to_score(sc):
    for p, t in _pairs(12, 80):
        r = SG.align(p, t, *sc, mats=True)
        n, m = len(p), len(t)
        assert r["score"] == SG.op_score(p, t, r["ops"], r["start"], *sc), (p, t, sc)
        assert r["end"][0] == n and r["start"][0] == 0 and r["start"][1] <= r["end"][1] <= m
        row = r["dp"][n] if n else [0]
        assert r["score"] == max(row) and (n == 0 or r["end"][1] == list(row).index(max(row)))
        if n:   # the ops cover the whole pattern and exactly text [j0, j*)
            assert r["ops"].count(b"M") + r["ops"].count(b"D") == n
            assert r["ops"].count(b"M") + r["ops"].count(b"I") == r["end"][1] - r["start"][1]


def test_edge_cases():
    assert SG.align(b"", b"ACGT", 1, -1, -1) == dict(score=0, end=(0, 0), start=(0, 0), ops=b"")
    r = SG.align(b"ACG", b"", 2, -3, -5)
    assert (r["score"], r["end"], r["start"], r["ops"]) == (-15, (3, 0), (0, 0), b"DDD")
    r = SG.align(b"ACG", b"TTACGTT", 1, -1, -1)
    assert (r["score"], r["end"], r["start"], r["ops"]) == (3, (3, 5), (0, 2), b"MMM")
    r = SG.align(b"ACG", b"TTT", 0, 0, 0)   # all ties: j* = 0, the walk goes down column 0
    assert (r["score"], r["end"], r["start"], r["ops"]) == (0, (3, 0), (0, 0), b"DDD")


def test_prefixes_match_single_fills():
    rng = random.Random(5)
    p = bytes(rng.choice(b"ACGT") for _ in range(20))
    t = bytes(rng.choice(b"ACGT") for _ in range(40))
    ms = [0, 1, 7, 19, 40]
    for sc in SCORINGS:
        assert SG.prefixes(p, t, ms, *sc) == [SG.align(p, t[:m], *sc) for m in ms]
