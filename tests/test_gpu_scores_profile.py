"""Profile form of the packed f16 strip cells (batch_scores.hip.h, PROF16): one pattern against 128 texts per wave task, the
row's score read through VGPR index mode.  Every case is checked element for element against the CELL16 form of the same list
(PWA_PROF16=0) and against the oracle.  The CPU test at the end checks the G = h + g recurrence itself in numpy."""
import random

import numpy as np
import pytest

import oracle_lib as O
from conftest import switched_context


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def run(env, seqs, pa, pb, scoring):
    with switched_context(PWA_SCORES_ROUTE="0", PWA_FORCE_LANES="0", PWA_CELL16="1", **env) as c:   # (small lists: packed cells, shared texts)
        b = c.batch("sw", seqs, pa, pb, *scoring)
        form, bits, kern = b.profile_form(), b.cell_bits(), b.info()["kernel"]
        b.run()
        got = b.fetch()
        b.close()
    return got, form, bits, kern


def check(seqs, pa, pb, scoring, want_form=1, sample=None, seed=0):
    prof, form, bits, kern = run({"PWA_PROF16": "1"}, seqs, pa, pb, scoring)
    cell, form0, bits0, kern0 = run({"PWA_PROF16": "0"}, seqs, pa, pb, scoring)
    assert form == want_form, (scoring, form, bits, kern)
    assert form0 == 0
    assert kern == kern0   # the reported name stays the CELL16 entry's
    assert prof == cell, (scoring, [k for k in range(len(pa)) if prof[k] != cell[k]][:5])
    ks = range(len(pa)) if sample is None else random.Random(seed).sample(range(len(pa)), sample)
    bad = [k for k in ks if prof[k] != O.score("sw", seqs[pa[k]], seqs[pb[k]], *scoring)[0]]
    assert not bad, (scoring, bad[:5])


@pytest.mark.gpu
def test_pattern_lengths_and_ragged_texts(ctx):
    """patterns of 1..152 rows (153 falls back), texts of every length residue mod 8, partial tasks, several scorings"""
    rng = random.Random(505)
    lens = list(range(1, 153, 7)) + [150, 151, 152]
    pats = [rand_seq(rng, n) for n in lens]
    txts = [rand_seq(rng, m) for m in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257, 1001, 1002, 1003)]
    seqs = pats + txts
    pa = [i for i in range(len(pats)) for _ in range(len(txts))]
    pb = [len(pats) + j for _ in range(len(pats)) for j in range(len(txts))]
    for scoring in [(1, -1, -1), (2, -3, -5), (5, -4, -4), (13, -20, -2), (1, 0, 0), (0, -1, -1)]:
        check(seqs, pa, pb, scoring)
    long_pats = pats + [rand_seq(rng, 153)]
    seqs2 = long_pats + txts
    pa2 = [len(long_pats) - 1] * len(txts) + pa
    pb2 = [len(long_pats) + j for j in range(len(txts))] + [p + 1 for p in pb]
    got, form, _, _ = run({"PWA_PROF16": "1"}, seqs2, pa2, pb2, (1, -1, -1))
    assert form == 0   # a pattern of 153 rows: CELL16
    assert got == [O.score("sw", seqs2[a], seqs2[b], 1, -1, -1)[0] for a, b in zip(pa2, pb2)]


@pytest.mark.gpu
def test_many_pairs_per_pattern_equal_maxima_and_boundaries(ctx):
    """> 128 texts per pattern (several tasks of one pattern), repeated texts (many equal maxima), scores at the 2047 boundary,
    +-127 scorings"""
    rng = random.Random(506)
    base = rand_seq(rng, 150)
    pats = [base, rand_seq(rng, 150), b"A" * 150, rand_seq(rng, 89)]
    txts = [base * 3, base[:75] + base[:75], b"A" * 400] + [rand_seq(rng, rng.randint(100, 700)) for _ in range(140)]
    seqs = pats + txts
    pa = [i for i in range(len(pats)) for _ in range(len(txts))]
    pb = [len(pats) + j for _ in range(len(pats)) for j in range(len(txts))]
    for scoring in [(13, -1, -1), (13, -127, -127), (1, -127, -127), (127, -127, -127)]:
        n = 2047 // scoring[0]
        p2 = [p[:n] for p in pats]
        check(p2 + txts, pa, pb, scoring)


@pytest.mark.gpu
def test_fallbacks_and_default(ctx):
    """a non-DNA alphabet runs CELL16 or int32 whatever the knob; C3's shape (256 patterns x 128 texts of 2000) takes the profile
    form by default, under the CELL16 entry's name"""
    rng = random.Random(507)
    pats = [rand_seq(rng, 60) for _ in range(8)]
    txts = [rand_seq(rng, 300, b"ACGTN") for _ in range(130)]
    seqs = pats + txts
    pa = [i for i in range(8) for _ in range(130)]
    pb = [8 + j for _ in range(8) for j in range(130)]
    got, form, _, _ = run({"PWA_PROF16": "1"}, seqs, pa, pb, (1, -1, -1))
    assert form == 0
    assert got == [O.score("sw", seqs[a], seqs[b], 1, -1, -1)[0] for a, b in zip(pa, pb)]
    pats = [O.gen(1, 0, p, 150) for p in range(256)]
    txts = [O.gen(1, 1, t, 2000) for t in range(128)]
    seqs = pats + txts
    pa = np.repeat(np.arange(256, dtype=np.uint32), 128)
    pb = np.tile(np.arange(128, dtype=np.uint32) + np.uint32(256), 256)
    with switched_context(PWA_SCORES_ROUTE="0") as c:
        b = c.batch("sw", seqs, pa, pb, 1, -1, -1)
        assert b.profile_form() == 1 and b.cell_bits() == 16
        assert b.info()["kernel"] == "batch_scores_kernel<R=76,BM_SWS,SC_PERM>", b.info()
        b.run()
        prof = b.fetch(numpy_out=True)
        b.close()
    with switched_context(PWA_PROF16="0", PWA_SCORES_ROUTE="0") as c:
        b = c.batch("sw", seqs, pa, pb, 1, -1, -1)
        assert b.profile_form() == 0
        b.run()
        cell = b.fetch(numpy_out=True)
        b.close()
    assert np.array_equal(prof, cell), int(np.count_nonzero(prof != cell))
    for k in random.Random(8).sample(range(len(pa)), 16):
        assert prof[k] == O.score("sw", seqs[pa[k]], seqs[pb[k]], 1, -1, -1)[0], k


def g_form_sw(p, t, match, mismatch, gap):
    """the kernel's recurrence in integers: G = h + g per cell, t' = max(0, G_diag + s - g), h = max(t', G_up, G_left)"""
    n, m = len(p), len(t)
    G = np.full(m + 1, gap, dtype=np.int64)   # row 0 (H = 0)
    best = 0
    for i in range(n):
        new = np.empty_like(G)
        new[0] = gap                           # column 0 (H = 0)
        for j in range(1, m + 1):
            s = match if p[i] == t[j - 1] else mismatch
            tp = max(0, G[j - 1] + s - gap)
            h = max(tp, G[j], new[j - 1])
            best = max(best, h)
            new[j] = h + gap
        G = new
    return best


def test_g_form_recurrence_matches_oracle():
    rng = random.Random(508)
    for _ in range(40):
        p = rand_seq(rng, rng.randint(1, 40))
        t = rand_seq(rng, rng.randint(1, 60))
        for scoring in [(1, -1, -1), (2, -3, -5), (5, -4, 0), (3, 0, -2)]:
            assert g_form_sw(p, t, *scoring) == O.score("sw", p, t, *scoring)[0], (p, t, scoring)
