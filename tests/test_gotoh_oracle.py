"""CPU checks of the affine-gap (gotoh) numpy oracle: against a plain three-matrix DP, against the linear oracles at gap_open = 0,
and the affine score of every op list against the returned score."""
import random

import numpy as np
import pytest

import gotoh_oracle as GO
import oracle_lib as O
import sg_oracle as SG

SCORINGS = [(1, -4, -6, -1), (2, -3, -5, -2), (5, -4, -16, -4), (1, -1, -1, -1), (0, 0, 0, 0), (3, -1, 0, -2)]
# the edges the device kernels are tested at too (test_gpu_gotoh_edges.py): gap_extend = 0 (every open / extend choice ties), match <=
# mismatch, a positive mismatch (pad rows past n then outgrow the real ones), match = 0 with gaps, a gap open that never pays off,
# an extension dearer than the opening, a negative match
EDGE_SCORINGS = [(1, -4, -6, 0), (3, -2, -7, 0), (-1, 2, -3, 0), (-1, 2, -3, -1), (0, 1, -2, -1), (1, -1, -20, -1), (4, -1, -1, -3),
                 (-2, -1, -1, -1)]


def _rand(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("sc", SCORINGS + EDGE_SCORINGS)
def test_oracle_matches_scalar_dp(mode, sc):
    rng = random.Random(hash((mode, sc)) & 0xffff)
    match, mismatch, go, ge = sc
    for _ in range(12):
        n, m = rng.randint(1, 14), rng.randint(1, 14)
        p, t = _rand(rng, n, b"AC"), _rand(rng, m, b"ACG")
        tab = GO.fill(GO._arr(p)[None, :], GO._arr(t)[None, :], mode, (match, mismatch), go, ge)
        H, src, eop, fop = GO.scalar_dp(p, t, mode, (match, mismatch), go, ge)
        assert tab["H"][0].tolist() == H
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                assert tab["src"][0][i, j] == src[i][j], (i, j)
                assert bool(tab["eop"][0][i, j]) == eop[i][j], (i, j)
                assert bool(tab["fop"][0][i, j]) == fop[i][j], (i, j)


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("sc", SCORINGS + EDGE_SCORINGS)
def test_op_scores_equal_scores(mode, sc):
    rng = random.Random(7 + len(mode))
    match, mismatch, go, ge = sc
    pairs = [(_rand(rng, rng.randint(0, 40)), _rand(rng, rng.randint(0, 60))) for _ in range(40)]
    for (p, t), r in zip(pairs, GO.align_many(pairs, mode, (match, mismatch), go, ge)):
        assert GO.op_score(p, t, r["ops"], r["start"], (match, mismatch), go, ge) == r["score"]
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
        got = GO.align(p, t, mode, (match, mismatch), 0, gap)
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
        got = GO.align(p, t, "sg", (match, mismatch), 0, gap)
        assert (got["score"], got["end"], got["start"], got["ops"]) == (want["score"], want["end"], want["start"], want["ops"])


def test_prefixes_equal_own_fills():
    rng = random.Random(5)
    p, t = _rand(rng, 30), _rand(rng, 80)
    for mode in ("nw", "sw", "sg"):
        ms = [0, 1, 17, 50, 80]
        for m, r in zip(ms, GO.prefixes(p, t, ms, mode, (2, -3), -5, -2)):
            assert r == GO.align(p, t[:m], mode, (2, -3), -5, -2)


def test_one_event_is_one_gap():
    """12 text bases missing from a read come back as one 'I' run (text-only columns) under affine scoring."""
    rng = random.Random(3)
    region = _rand(rng, 400)
    read = region[100:160] + region[172:250]   # 12 bases deleted
    r = GO.align(read, region, "sg", (1, -4), -6, -1)
    ops = bytes(reversed(r["ops"]))
    assert b"I" * 12 in ops and ops.count(b"I") == 12 and b"D" not in ops
    assert r["score"] == len(read) - 6 - 12


def _rule_walk(p, t, mode, match, mismatch, go, ge):
    """pwalign.h's end cell and three-state walk, written from the stated rules over scalar_dp's H alone: E and F are recomputed
    from H, every choice is made from values (no source or open codes) -> (score, end, start, ops)"""
    n, m = len(p), len(t)
    H = GO.scalar_dp(p, t, mode, (match, mismatch), go, ge)[0]
    oe, inf = go + ge, float("-inf")
    E = [[inf] * (m + 1) for _ in range(n + 1)]
    F = [[inf] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i][j] = max(H[i][j - 1] + oe, E[i][j - 1] + ge)
            F[i][j] = max(H[i - 1][j] + oe, F[i - 1][j] + ge)
    if mode == "nw":
        end = (n, m)
    elif mode == "sg":
        end = (n, min(j for j in range(m + 1) if H[n][j] == max(H[n])))
    else:
        best = max(max(r) for r in H)
        end = (0, 0) if best <= 0 else next((i, j) for i in range(n + 1) for j in range(m + 1) if H[i][j] == best)
    i, j = end
    ops, st = [], "H"
    while i > 0 and j > 0:
        if st == "H":
            d = H[i - 1][j - 1] + (match if p[i - 1] == t[j - 1] else mismatch)
            h = H[i][j]
            if mode == "sw" and h == 0:
                break
            order = ["D", "F", "E"] if mode == "sw" else ["D", "E", "F"]   # SW: zero > diag > F > E; NW, SG: diag >= E >= F
            st = next(s for s in order if {"D": d, "E": E[i][j], "F": F[i][j]}[s] == h)
            if st == "D":
                ops.append("M")
                i, j, st = i - 1, j - 1, "H"
                continue
        if st == "E":   # a tie opens
            ops.append("I")
            st = "H" if H[i][j - 1] + oe >= E[i][j - 1] + ge else "E"
            j -= 1
        else:
            ops.append("D")
            st = "H" if H[i - 1][j] + oe >= F[i - 1][j] + ge else "F"
            i -= 1
    if mode != "sw":
        ops += ["D"] * i
        i = 0
        if mode == "nw":
            ops += ["I"] * j
            j = 0
    return H[end[0]][end[1]], end, (i, j), "".join(ops).encode()


def _homopolymer_cases():
    """runs with one gap that can sit at any of several places (all of them tie), on both sides and in the middle"""
    out = []
    for a, b in [(b"ACG", b"CA"), (b"", b"GC"), (b"TG", b""), (b"G", b"C")]:
        for run, d in [(b"T", 5), (b"TT", 3), (b"A", 4)]:
            for k in (1, 2, 3):
                short, long_ = a + run * d + b, a + run * (d + k) + b
                out += [(short, long_), (long_, short)]
    out += [(b"AAAA", b"AA"), (b"AA", b"AAAA"), (b"A", b"AAAAA"), (b"CAAAC", b"CAC"), (b"ACACAC", b"ACAC"), (b"ACAC", b"ACACAC")]
    return out


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("sc", [(1, -4, -6, -1), (2, -3, -5, -2), (1, -4, -6, 0), (1, -1, -1, -1), (-1, 2, -3, 0), (0, 1, -2, -1)])
def test_walk_tie_breaks_follow_the_stated_rules(mode, sc):
    """gap placement in homopolymer and tandem runs, open vs extend (gap_extend = 0 ties them), first maxima: the oracle's walk equals
    the rule walk above, field for field"""
    match, mismatch, go, ge = sc
    for p, t in _homopolymer_cases():
        r = GO.align(p, t, mode, (match, mismatch), go, ge)
        score, end, start, ops = _rule_walk(p, t, mode, match, mismatch, go, ge)
        assert (r["score"], r["end"], r["start"], r["ops"]) == (score, end, start, ops), (p, t)


def test_homopolymer_gap_sits_at_the_run_start():
    """the walk runs backwards and prefers the diagonal, so a gap in a run lands at its first base (forward order); global and
    semi-global (a local alignment of these drops the gap)"""
    for mode in ("nw", "sg"):
        r = GO.align(b"ACGTTTTTCA", b"ACGTTTTTTTCA", mode, (1, -4), -6, -1)
        assert bytes(reversed(r["ops"])) == b"MMMIIMMMMMMM", mode
        r = GO.align(b"ACGTTTTTTTCA", b"ACGTTTTTCA", mode, (1, -4), -6, -1)
        assert bytes(reversed(r["ops"])) == b"MMMDDMMMMMMM", mode
