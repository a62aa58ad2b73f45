"""The claim the codes form of the wavefront alignments rests on, without a GPU: one code byte per cell (taken from the comparisons
of the sweep) and a greedy extend over the sequences rebuild the op list of the walk over the stored offsets, byte for byte
(wfa_codes_oracle.py against wfa_oracle.py), on random and mutated pairs under four scorings and on crafted ties."""
import random

import numpy as np
import pytest

import wfa_codes_oracle as CO
import wfa_oracle as WO

SCORINGS = [(1, -1, 0, -1), (5, -4, -16, -4), (0, -4, -6, -2), (1, -40, -6, -1)]
SC = (1, -4, -6, -1)


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
            out.append(rng.choice([a for a in alphabet if a != c]))
        else:
            out.append(c)
    return bytes(out)[:120]


def same(p, t, sc, bound=None):
    got, want = CO.align(p, t, *sc, min_score=bound)
    assert got["ops"] == want["ops"], (p, t, sc)
    return want


@pytest.mark.parametrize("sc", SCORINGS)
def test_random_and_mutated_pairs(sc):
    """80 pairs per scoring, 320 in all, of 0 .. 120 symbols"""
    rng = random.Random(100 + sum(sc))
    kinds = set()
    for k in range(80):
        n = rng.choice([0, 1, 2, 3, 7, 8, 9, 33, 64, 65, 120]) if k % 4 == 0 else rng.randint(0, 120)
        p = rand_seq(rng, n, b"ACGT" if k % 3 else b"AC")
        t = rand_seq(rng, rng.randint(0, 120), b"AC") if k % 5 == 0 else mutate(rng, p, 0.3 * (k % 8) / 7)
        ops = same(p, t, sc)["ops"]
        kinds |= set(ops)
    assert kinds == set(b"MID")


@pytest.mark.parametrize("sc", SCORINGS + [SC])
def test_homopolymers_of_unequal_length(sc):
    """every extend runs to an end of the pair, so the sources of M tie all over the wavefronts and the tie order decides the list"""
    for n, m in [(10, 13), (13, 9), (1, 6), (6, 1), (40, 41), (7, 7)]:
        want = same(b"A" * n, b"A" * m, sc)
        assert want["ops"].count(b"M") == min(n, m) and len(want["ops"]) == max(n, m)
    x, o, e, g = WO.penalties(*sc)
    srcs = set()
    for n, m in [(10, 13), (13, 10)]:
        P, W = WO.sweep(b"A" * n, b"A" * m, (x, o, e), 10 ** 6)
        srcs |= {int(c) & 3 for c in CO.code_plane(W, (x, o, e), P, n, m) if c != CO.JUNK}
    assert srcs >= {CO.SRC_I, CO.SRC_D, CO.SRC_NONE}


def test_an_insertion_run_next_to_a_deletion_run():
    """1/-40/-6/-1: a block of three against a block of two is cheaper as 'DDD' + 'II' than as any mismatch"""
    sc = (1, -40, -6, -1)
    rng = random.Random(3)
    seen = False
    for a, b in [(b"TTT", b"GG"), (b"GG", b"TTT"), (b"T", b"G"), (b"TTTTT", b"GGGGG")]:
        left, right = rand_seq(rng, 30, b"AC"), rand_seq(rng, 25, b"AC")
        ops = same(left + a + right, left + b + right, sc)["ops"]
        seen = seen or b"ID" in ops or b"DI" in ops
        assert b"M" * 20 in ops
    assert seen


@pytest.mark.parametrize("sc", [SC, (5, -4, -16, -4), (1, -1, 0, -1)])
def test_a_gap_next_to_a_mismatch(sc):
    rng = random.Random(4)
    left, right = rand_seq(rng, 30, b"AC"), rand_seq(rng, 25, b"AC")
    for p, t in [(left + b"T" + right, left + b"GGGG" + right), (left + b"TGGG" + right, left + b"C" + right),
                 (left + b"TT" + right, left + b"G" + right), (b"T" + right, b"GGG" + right), (left + b"T", left + b"GGG")]:
        ops = same(p, t, sc)["ops"]
        assert ops.count(b"I") + ops.count(b"D") >= 1
        same(t, p, sc)


def open_extend_ties(p, t, sc):
    """cells of the sweep at which M[s-o-e][k-1] == I[s-e][k-1] or M[s-o-e][k+1] == D[s-e][k+1], both offsets real"""
    x, o, e, g = WO.penalties(*sc)
    P, W = WO.sweep(p, t, (x, o, e), 10 ** 6)
    count = 0
    for s in W:
        wo, we = W.get(s - o - e), W.get(s - e)
        if wo is not None and we is not None:
            count += int(((wo[0] == we[1]) & (wo[0] >= 0)).sum() + ((wo[0] == we[2]) & (wo[0] >= 0)).sum())
    return count


def test_a_gap_whose_open_and_extend_tie():
    """linear gaps (gap_open 0): going on in I costs what opening from M costs, so wherever M came from I without a match behind it
    the two offsets are equal and the tie has to open; repeats do the same under an affine scoring"""
    rng = random.Random(5)
    left, right = rand_seq(rng, 20, b"AC"), rand_seq(rng, 20, b"AC")
    cases = [((1, -1, 0, -1), left + right, left + b"GGGG" + right), ((1, -1, 0, -1), left + b"TTTTT" + right, left + right),
             ((1, -1, 0, -1), b"ACACACACAC", b"ACACACACACACAC"), (SC, b"ACACACACACACACAC" * 2, b"ACACACACAC" * 2),
             (SC, b"AAAA", b"CCCCCCCCC"), ((5, -4, -16, -4), b"ACAA", b"CCGGCGCCC"),
             ((1, -40, -6, -1), b"ACAA", b"CCGGCGCCC"), ((0, -4, -6, -2), b"GTGTGTGTGTGTGTGTGT", b"GTGTGTGTGT")]
    for sc, p, t in cases:
        assert open_extend_ties(p, t, sc) > 0
        same(p, t, sc)
        same(t, p, sc)


def test_bounds_and_empty_sides():
    for p, t in [(b"", b""), (b"ACGT", b""), (b"", b"AC"), (b"A", b"C"), (b"A", b"A")]:
        for sc in SCORINGS:
            same(p, t, sc)
    rng = random.Random(6)
    p = rand_seq(rng, 90)
    t = mutate(rng, p, 0.1)
    best = WO.align(p, t, *SC)["score"]
    assert same(p, t, SC, best)["score"] == best and same(p, t, SC, best + 1)["score"] is None


def test_a_walk_over_junk_codes_faults_and_ends():
    """the guards of pass A: a plane of junk, or codes that lead off the wavefronts, end in a fault, never in a loop"""
    rng = random.Random(7)
    p = rand_seq(rng, 60)
    t = mutate(rng, p, 0.15) + b"GG"
    x, o, e, g = WO.penalties(*SC)
    P, W = WO.sweep(p, t, (x, o, e), 10 ** 6)
    n, m = len(p), len(t)
    assert n != m   # (so that a plane of "mismatch" codes cannot end on the main diagonal by chance)
    plane = CO.code_plane(W, (x, o, e), P, n, m)
    for junk in (0x00, 0xFF, CO.JUNK, CO.SRC_I, CO.SRC_D | CO.OPEN_D, CO.SRC_I | CO.OPEN_I):
        with pytest.raises(CO.Fault):
            CO.pass_a(np.full(len(plane), junk, dtype=np.uint8), (x, o, e), P, n, m, bytearray(n + m))
