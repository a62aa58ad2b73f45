"""Packed f16 strip cells (batch_scores.hip.h, CELL16): two local-alignment pairs per lane.  Every case is checked against the
oracle (all pairs, or a seeded sample on the larger lists) and, where the packed form runs, element for element against the
int32 cells of the same list (PWA_CELL16=0).  pwa_batch_cell_bits says which form a batch runs.
Every test here needs a real MI355X: run with `pytest -m gpu`."""
import random

import numpy as np
import pytest

import oracle_lib as O
from conftest import switched_context

pytestmark = pytest.mark.gpu


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def run(env, seqs, pa, pb, scoring):
    with switched_context(PWA_SCORES_ROUTE="0", **env) as c:
        b = c.batch("sw", seqs, pa, pb, *scoring)
        bits, kern = b.cell_bits(), b.info()["kernel"]
        b.run()
        got = b.fetch()
        b.close()
    return got, bits, kern


def check(seqs, pa, pb, scoring, want_bits=16, sample=None, seed=0):
    """auto / forced packed / forced int32 against each other and against the oracle"""
    auto, bits_auto, _ = run({}, seqs, pa, pb, scoring)
    packed, bits16, kern16 = run({"PWA_CELL16": "1"}, seqs, pa, pb, scoring)
    plain, bits32, _ = run({"PWA_CELL16": "0"}, seqs, pa, pb, scoring)
    assert bits16 == want_bits, (scoring, bits16, kern16)
    assert bits32 == 32
    assert bits_auto in (16, 32)
    assert packed == plain, (scoring, [k for k in range(len(pa)) if packed[k] != plain[k]][:5])
    assert auto == plain
    ks = range(len(pa)) if sample is None else random.Random(seed).sample(range(len(pa)), sample)
    bad = [k for k in ks if plain[k] != O.score("sw", seqs[pa[k]], seqs[pb[k]], *scoring)[0]]
    assert not bad, (scoring, bad[:5])
    return packed, kern16


def test_ragged_odd_counts_and_text_only_symbols(ctx):
    """ragged pattern lengths inside a task (pad rows), odd pattern counts per text (an empty or partial B half), texts with a
    symbol no pattern has (N), several scorings including match >= 10, every text length residue mod 4"""
    rng = random.Random(1601)
    pats = [rand_seq(rng, rng.randint(1, 152)) for _ in range(201)]
    txts = [rand_seq(rng, m, b"ACGTN") for m in (1, 2, 3, 4, 5, 63, 64, 65, 66, 257, 1001, 1002)]
    seqs = pats + txts
    pa, pb = [], []
    for j in range(len(txts)):
        cnt = [1, 63, 64, 65, 127, 129, 201, 7, 131, 200, 99, 150][j]
        for i in rng.sample(range(len(pats)), cnt):
            pa.append(i)
            pb.append(len(pats) + j)
    for scoring in [(1, -1, -1), (2, -3, -5), (5, -4, -4), (10, -7, -3), (13, -20, -2), (1, 0, 0), (0, -1, -1)]:
        check(seqs, pa, pb, scoring)


def test_multi_strip_patterns_through_the_packed_hand_off(ctx):
    """patterns of 8 and more strips (560-620 rows): the bottom rows cross the HBM hand-off as f16 pairs"""
    rng = random.Random(1602)
    pats = [rand_seq(rng, rng.randint(560, 620)) for _ in range(130)] + [rand_seq(rng, rng.randint(1, 40)) for _ in range(3)]
    txts = [rand_seq(rng, m, b"ACGTN") for m in (5, 700, 1403)]
    seqs = pats + txts
    pa = [i for j in range(3) for i in range(len(pats))]
    pb = [len(pats) + j for j in range(3) for _ in range(len(pats))]
    check(seqs, pa, pb, (3, -2, -3), sample=60, seed=2)


def test_range_boundary_2047_packed_2048_falls_back(ctx):
    """longest pattern * match = 2047 runs packed and scores 2047 exactly; 2048 must take the int32 cells"""
    rng = random.Random(1603)
    for n, match, want_bits in [(2047, 1, 16), (2048, 1, 32), (89, 23, 16), (128, 16, 32)]:
        p = rand_seq(rng, n)
        seqs = [p, p, rand_seq(rng, n)] + [p + rand_seq(rng, 7), rand_seq(rng, 50) + p]
        pa = [0, 1, 2, 0, 2]
        pb = [3, 4, 4, 4, 3]
        scoring = (match, -1, -2)
        got, bits, _ = run({"PWA_CELL16": "1", "PWA_FORCE_LANES": "0"}, seqs, pa, pb, scoring)   # (5 pairs: not the per-lane-text kernels)
        assert bits == want_bits, (n, match, bits)
        assert got[0] == n * match and got[1] == n * match, (n, match, got)
        want = [O.score("sw", seqs[a], seqs[b], *scoring)[0] for a, b in zip(pa, pb)]
        assert got == want, (n, match)


@pytest.mark.parametrize("case", ["five pattern symbols", "pattern symbol absent from texts", "positive gap", "positive mismatch",
                                  "score 128"])
def test_ineligible_batches_fall_back(ctx, case):
    rng = random.Random(1604)
    alpha_p, alpha_t, scoring = b"ACGT", b"ACGT", (2, -1, -1)
    if case == "five pattern symbols":
        alpha_p = alpha_t = b"ACGTN"
    elif case == "pattern symbol absent from texts":
        alpha_p = b"ACGTX"
    elif case == "positive gap":
        scoring = (2, -1, 1)
    elif case == "positive mismatch":
        scoring = (2, 1, -1)
    else:
        scoring = (128, -1, -1)
    pats = [rand_seq(rng, rng.randint(1, 15), alpha_p) for _ in range(70)]
    txts = [rand_seq(rng, rng.randint(20, 90), alpha_t) for _ in range(3)]
    seqs = pats + txts
    pa = [i for j in range(3) for i in range(70)]
    pb = [70 + j for j in range(3) for _ in range(70)]
    got, bits, _ = run({"PWA_CELL16": "1"}, seqs, pa, pb, scoring)
    assert bits != 16, case
    want = [O.score("sw", seqs[a], seqs[b], *scoring)[0] for a, b in zip(pa, pb)]
    assert got == want, case


def test_reduced_c3_packed_equals_int32(ctx):
    """C3's shape at 512 patterns x 32 texts: the default picks the packed cells under the int32 form's name, and every score
    equals the int32 cells' (and the oracle on a sample)"""
    pats = [O.gen(1, 0, p, 150) for p in range(512)]
    txts = [O.gen(1, 1, t, 10000) for t in range(32)]
    seqs = pats + txts
    pa = np.repeat(np.arange(512, dtype=np.uint32), 32)
    pb = np.tile(np.arange(32, dtype=np.uint32) + np.uint32(512), 512)
    with switched_context(PWA_SCORES_ROUTE="0") as c:   # (128 wave tasks: the route model would move some off the strips)
        b = c.batch("sw", seqs, pa, pb, 1, -1, -1)
        assert b.cell_bits() == 16
        assert b.info()["kernel"] == "batch_scores_kernel<R=76,BM_SWS,SC_PERM>", b.info()
        b.run()
        packed = b.fetch(numpy_out=True)
        b.close()
    with switched_context(PWA_CELL16="0", PWA_SCORES_ROUTE="0") as c:
        b = c.batch("sw", seqs, pa, pb, 1, -1, -1)
        assert b.cell_bits() == 32
        b.run()
        plain = b.fetch(numpy_out=True)
        b.close()
    assert np.array_equal(packed, plain), int(np.count_nonzero(packed != plain))
    for k in random.Random(5).sample(range(len(pa)), 24):
        assert packed[k] == O.score("sw", seqs[pa[k]], seqs[pb[k]], 1, -1, -1)[0], k


def test_hand_off_past_a_32_bit_block_offset(ctx):
    """a text of more than 2^23 columns: its hand-off row is more than 2^31 bytes long, so a 32-bit byte offset of the packed
    kernel's blocks would overflow there.  Patterns of 80 rows (two strips) planted near the text's end score only through the
    hand-off beyond that point: packed == int32 == oracle"""
    rng = np.random.default_rng(1605)
    m = (1 << 23) + 11_403   # (a residue of 3 mod 4: the last columns take the one-column path)
    text = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, m)].tobytes())
    pats = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 80)].tobytes() for _ in range(100)]
    for k, pos in enumerate([m - 80, m - 2_000, (1 << 23) + 100, (1 << 23) - 40]):   # the last one straddles column 2^23
        text[pos:pos + 80] = pats[k]
    seqs = pats + [bytes(text)]
    pa = list(range(len(pats)))
    pb = [len(pats)] * len(pats)
    packed, bits16, _ = run({"PWA_CELL16": "1"}, seqs, pa, pb, (2, -3, -5))
    plain, bits32, _ = run({"PWA_CELL16": "0"}, seqs, pa, pb, (2, -3, -5))
    assert bits16 == 16 and bits32 == 32
    assert packed == plain, [k for k in range(len(pa)) if packed[k] != plain[k]][:5]
    assert packed[:4] == [160] * 4, packed[:4]
    for k in (0, 1, 2, 3, 50):
        assert packed[k] == O.score("sw", seqs[pa[k]], seqs[pb[k]], 2, -3, -5)[0], k
