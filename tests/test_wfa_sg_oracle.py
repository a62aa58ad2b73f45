"""The semi-global WFA oracle (wfa_sg_oracle.py) against the affine-gap DP oracle (gotoh_oracle.py, mode sg): the per-pattern-symbol
penalties, the sweep over the free text start, the end rule (lowest diagonal = first maximum of row n), the backtrace to a start cell
(0, k), the planned span and the bound, without a GPU."""
import random

import pytest

import gotoh_oracle as GO
import wfa_sg_oracle as SO

SCORINGS = [(1, -4, -6, -1), (0, -1, 0, -1), (2, -3, -5, -2), (1, -1, 0, -1), (5, -4, -16, -4), (3, -3, -9, -3)]
NS = (0, 1, 2, 5, 17, 40, 70)
MS = (0, 1, 3, 20, 64, 65, 130)


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet=b"ACGT"):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice(alphabet))
            out.append(c)
        elif r < rate:
            out.append(rng.choice(alphabet))
        else:
            out.append(c)
    return bytes(out)


def pairs(seed):
    """every (n, m) of NS x MS, random and planted (a mutated read cut out of the text, or hanging over one of its ends)"""
    rng = random.Random(seed)
    out = []
    for n in NS:
        for m in MS:
            t = rand_seq(rng, m)
            kind = rng.randint(0, 3)
            if kind == 0 or m == 0:
                p = rand_seq(rng, n)
            else:
                at = rng.randint(0, max(0, m - n))
                core = mutate(rng, t[at:at + n], rng.choice([0.0, 0.05, 0.2]))
                if kind == 3:   # hangs over an end
                    core = rand_seq(rng, 3) + core if rng.random() < 0.5 else core + rand_seq(rng, 3)
                p = (core + rand_seq(rng, n))[:n]
            out.append((p, t))
    return out


def consumed(ops):
    return ops.count(b"M") + ops.count(b"D"), ops.count(b"M") + ops.count(b"I")


@pytest.mark.parametrize("sc", SCORINGS)
def test_score_end_and_ops_against_the_dp(sc):
    match, mismatch, go, ge = sc
    x, o, ei, ed, g = SO.penalties(*sc)
    same = 0
    for p, t in pairs(sum(sc) + 31):
        n, m = len(p), len(t)
        want = GO.align(p, t, "sg", (match, mismatch), go, ge)
        got = SO.align(p, t, *sc)
        assert got["score"] == want["score"], (p, t)
        assert got["end"] == want["end"], (p, t)
        (i0, j0), (i1, j1) = got["start"], got["end"]
        assert i0 == 0 and 0 <= j0 <= j1 <= m
        assert consumed(got["ops"]) == (n, j1 - j0), (p, t)
        assert GO.op_score(p, t, got["ops"], got["start"], (match, mismatch), go, ge) == want["score"], (p, t, got["ops"])
        assert got["cells"] == SO.cells_to(got["penalty"], n, m, o, ed)
        assert got["penalty"] <= SO.p_worst(n, m, x, o, ed)
        P, k_end, W = SO.sweep(p, t, (x, o, ei, ed), got["penalty"])
        assert (P, n + k_end) == (got["penalty"], j1)
        assert SO.offsets_inside_the_span(W, (x, o, ei, ed), n, m), (p, t)
        same += got["ops"] == want["ops"] and got["start"] == want["start"]
    assert same > len(NS) * len(MS) // 2   # ties apart, the two walks agree


@pytest.mark.parametrize("sc", SCORINGS[:4])
def test_bound_at_the_optimum_one_above_and_one_below(sc):
    for p, t in pairs(sum(sc) + 7)[::2]:
        best = SO.align(p, t, *sc)
        assert SO.align(p, t, *sc, min_score=best["score"]) == best
        assert SO.align(p, t, *sc, min_score=best["score"] - 1) == best
        assert SO.align(p, t, *sc, min_score=-(1 << 20)) == best
        above = SO.align(p, t, *sc, min_score=best["score"] + 1)
        p_max, cells = SO.plan(len(p), len(t), *sc, best["score"] + 1)
        assert above == dict(SO.NOT_FOUND, cells=cells)   # 0 when the host decides, the whole plan when the sweep runs out


def test_penalties_and_invalid_scorings():
    assert SO.penalties(1, -4, -6, -1) == (5, 6, 1, 2, 1)
    assert SO.penalties(0, -1, 0, -1) == (1, 0, 1, 1, 1)
    assert SO.penalties(0, -4, -6, -2) == (2, 3, 1, 1, 2)
    assert SO.penalties(3, -3, -9, -3) == (2, 3, 1, 2, 3)
    assert SO.penalties(1, -40, -6, -1) == (41, 6, 1, 2, 1)
    for bad in [(1, 1, -1, -1), (2, 3, -1, -1), (1, 0, 1, -1), (1, 0, -1, 1), (1, -1, -1, 0), (-2, -3, 0, -1), (-1, -3, 0, -1)]:
        with pytest.raises(ValueError):
            SO.penalties(*bad)


def test_widths_cells_and_host_side_not_found():
    # 1/-4/-6/-1: x, o, eI, eD = 5, 6, 1, 2
    assert [SO.khd(s, 6, 2) for s in (0, 7, 8, 9, 10, 20)] == [0, 0, 1, 1, 2, 7]
    assert SO.span(20, 3, 9, 6, 2) == (-3, 9) and SO.span(9, 3, 9, 6, 2) == (-1, 9)
    assert SO.width(0, 5, 0, 6, 2) == 1 and SO.width(16, 5, 0, 6, 2) == 6
    assert SO.plan(5, 9, 1, -4, -6, -1) == (16, SO.cells_to(16, 5, 9, 6, 2))          # min(o + 5 eD, 5 x) = min(16, 25)
    assert SO.plan(2, 9, 1, -40, -6, -1)[0] == 10                                       # all 'D' is cheaper than two mismatches? no: 6 + 4
    assert SO.plan(5, 3, 1, -4, -6, -1)[0] == 16                                        # n > m: all 'D' only
    assert SO.plan(0, 9, 1, -4, -6, -1) == (0, 10)
    assert SO.plan(5, 9, 1, -4, -6, -1, 6) == (None, 0)                                 # above the score of an exact occurrence
    assert SO.plan(5, 9, 1, -4, -6, -1, 5)[0] == 0
    assert SO.plan(5, 3, 1, -4, -6, -1, -4) == (None, 0)                                # two 'D' at least: 10, the bound leaves 9
    assert SO.plan(5, 3, 1, -4, -6, -1, -5)[0] == 10
