"""The column-block loop of the packed profile form's integer row on the device (batch_scores.hip.h, scores16p_body): its leading
blocks prefetch their texts with plain loads, the rest clamp and pad (word()); the bound between them goes by the task's shortest
text, the loop's length by its longest.  Every pair of every batch is compared with the CPU oracle.

A wave task is one pattern against 128 texts, longest first (pwalign.hip, group_by_pattern): lane l runs the texts of rank l and
64 + l.  Every batch has 128 patterns, so that each text is shared by 128 pairs."""
import random

import numpy as np
import pytest

import oracle_lib as O
from conftest import switched_context

INT_SCORING = (1, -1, -1)    # mismatch >= gap: the integer row
F16_SCORING = (2, -3, -1)    # mismatch < gap: the f16 row, which keeps word() in every block
EDGES = [1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 255, 256, 257]
MIXED = [1, 2, 3, 75, 76, 149, 150, 151, 152]

# text lengths of a batch, by name.  "lane_pairs": ranks 0..63 are 257 long, rank 64 + l is shorter by 0, 1, 7, 8, 9 and by several
# blocks -- the shortest has 57 columns: 6 interior blocks of 33.
_LANE_DIFFS = [0] * 8 + [1] * 8 + [7] * 8 + [8] * 8 + [9] * 8 + [40] * 8 + [120] * 8 + [200] * 8
TEXT_SETS = {
    "edges": EDGES * 7,                                    # 133 texts: a full task and one of 5 texts (123 empty slots)
    "lane_pairs": [257] * 64 + [257 - d for d in _LANE_DIFFS],
    "around_8k": [255, 256, 257, 256] * 32,                # 8k - 1, 8k, 8k + 1: 30 interior blocks of 33
    "no_interior": [1, 2, 3, 4, 5, 6, 7, 7] * 16,          # every text shorter than a block
    "no_tail": [64] * 128,                                 # all equal, a multiple of 8: no masked column
    "one_empty_slot": [24 + (i % 17) for i in range(127)], # 127 texts: slot 127 empty (slot_out = 0xffffffff)
}
PATTERN_SETS = {"mixed": MIXED, "150": [150], "152": [152], "149_150": [149, 150], "151_152": [151, 152]}


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


@pytest.fixture(scope="module")
def forced():
    """a context that takes the profile form wherever the batch admits it (the cost model is not what is tested here)"""
    with switched_context(PWA_SCORES_ROUTE="0", PWA_FORCE_LANES="0", PWA_CELL16="1", PWA_PROF16="1") as c:
        yield c


_texts, _pool, _want = {}, {}, {}


def texts_of(name):
    if name not in _texts:
        rng = random.Random(sum(name.encode()))
        ts = [rand_seq(rng, m) for m in TEXT_SETS[name]]
        _texts[name] = ts
    return _texts[name]


def patterns_of(name):
    """128 patterns over the lengths of the set, drawn from two sequences per length (the oracle then runs once per content)"""
    if name not in _pool:
        rng = random.Random(7000 + sum(name.encode()))
        lens = PATTERN_SETS[name]
        pool = {n: [rand_seq(rng, n) for _ in range(2)] for n in lens}
        _pool[name] = [pool[lens[i % len(lens)]][(i // len(lens)) % 2] for i in range(128)]
    return _pool[name]


def want(p, t, scoring):
    key = (p, t, scoring)
    if key not in _want:
        _want[key] = O.score("sw", p, t, *scoring)[0]
    return _want[key]


def run_and_check(c, pset, tset, scoring):
    pats, txts = patterns_of(pset), texts_of(tset)
    if tset in ("lane_pairs", "around_8k"):   # long diagonal runs across the bound between the two kinds of block
        txts = [pats[5][:40] + t[40:] if i % 3 == 0 and len(t) >= 80 else t for i, t in enumerate(txts)]
    seqs = pats + txts
    pa = [i for i in range(len(pats)) for _ in range(len(txts))]
    pb = [len(pats) + j for _ in range(len(pats)) for j in range(len(txts))]
    b = c.batch("sw", seqs, pa, pb, *scoring)
    integer = 1 if scoring[1] - scoring[2] >= 0 and scoring[0] - scoring[2] >= 0 else 0
    forms = (b.profile_form(), b.cell_bits(), b.profile_int())
    assert forms == (1, 16, integer), (pset, tset, scoring, forms, b.info())   # (no other kernel can pass for this one)
    b.run()
    got = b.fetch()
    b.close()
    bad = [(k, got[k], want(seqs[pa[k]], seqs[pb[k]], scoring)) for k in range(len(pa)) if got[k] != want(seqs[pa[k]], seqs[pb[k]], scoring)]
    assert not bad, (pset, tset, scoring, len(bad), [(len(seqs[pa[k]]), len(seqs[pb[k]]), g, w) for k, g, w in bad[:8]])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("tset", sorted(TEXT_SETS))
def test_mixed_pattern_lengths_on_both_rows(forced, tset):
    """patterns of 1, 2, 3, 75, 76, 149..152 rows in one batch (pairs of pad rows skipped); the integer row and the f16 row"""
    run_and_check(forced, "mixed", tset, INT_SCORING)
    run_and_check(forced, "mixed", tset, F16_SCORING)


@pytest.mark.gpu
@pytest.mark.parametrize("pset", ["150", "152", "149_150", "151_152"])
def test_single_row_counts(forced, pset):
    """every task runs 150 (152) rows, a pad row last where the pattern is odd: no pair is skipped"""
    for tset in ("lane_pairs", "around_8k", "no_tail", "one_empty_slot", "edges", "no_interior"):
        run_and_check(forced, pset, tset, INT_SCORING)


@pytest.mark.gpu
def test_full_size_c3_by_default(ctx):
    """no forcing switches, the benchmark's list (4096 patterns of 150 rows against 256 texts of 10 000 columns; 1249 interior blocks
    of 1250 per task): the profile form and its integer row, the bench line's checksum and a seeded sample against the oracle"""
    pats = [O.gen(1, 0, p, 150) for p in range(4096)]
    txts = [O.gen(1, 1, t, 10000) for t in range(256)]
    seqs = pats + txts
    pa = np.repeat(np.arange(4096, dtype=np.uint32), 256)
    pb = np.tile(np.arange(256, dtype=np.uint32) + np.uint32(4096), 4096)
    b = ctx.batch("sw", seqs, pa, pb, *INT_SCORING)
    assert (b.profile_form(), b.cell_bits(), b.profile_int()) == (1, 16, 1), b.info()
    b.run()
    s = b.fetch(numpy_out=True)
    b.close()
    assert int(s.astype(np.int64).sum()) == 35376135
    for k in np.random.default_rng(7).choice(len(pa), 64, replace=False):
        assert int(s[k]) == want(seqs[pa[k]], seqs[pb[k]], INT_SCORING), k
