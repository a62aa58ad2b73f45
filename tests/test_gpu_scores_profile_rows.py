"""The packed profile form's rows on the device (batch_scores.hip.h, PROF16): the integer row's deferred last-column subtract with
col[] written in place, and the pad rows past the pattern's end that neither row runs.  Every list is compared element for element
with the oracle, between the two rows (PWA_PROF16_INT 1 and 0) and with the strip kernel (PWA_PROF16=0)."""
import random

import pytest

import oracle_lib as O
from conftest import switched_context

KNOBS = dict(PWA_SCORES_ROUTE="0", PWA_FORCE_LANES="0", PWA_CELL16="1")


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def admitted(scoring):
    match, mismatch, gap = scoring
    return mismatch - gap >= 0 and match - gap >= 0


def run(seqs, pa, pb, scoring, **knobs):
    with switched_context(**KNOBS, **knobs) as c:
        b = c.batch("sw", seqs, pa, pb, *scoring)
        forms = (b.profile_form(), b.profile_int())
        b.run()
        got = b.fetch()
        b.close()
    return got, forms


def check(seqs, pa, pb, scoring):
    got1, forms1 = run(seqs, pa, pb, scoring, PWA_PROF16="1", PWA_PROF16_INT="1")
    got0, forms0 = run(seqs, pa, pb, scoring, PWA_PROF16="1", PWA_PROF16_INT="0")
    gots, formss = run(seqs, pa, pb, scoring, PWA_PROF16="0")
    assert forms1 == (1, 1 if admitted(scoring) else 0) and forms0 == (1, 0) and formss == (0, 0), (scoring, forms1, forms0, formss)
    want = [O.score("sw", seqs[a], seqs[b], *scoring)[0] for a, b in zip(pa, pb)]
    for name, got in (("integer row", got1), ("f16 row", got0), ("strip kernel", gots)):
        bad = [k for k in range(len(pa)) if got[k] != want[k]]
        assert not bad, (name, scoring, [(len(seqs[pa[k]]), len(seqs[pb[k]]), got[k], want[k]) for k in bad[:5]])
    assert got1 == got0 == gots


def all_pairs(n_p, n_t):
    return [i for i in range(n_p) for _ in range(n_t)], [n_p + j for _ in range(n_p) for j in range(n_t)]


@pytest.mark.gpu
def test_every_pattern_length_back_to_back(ctx):
    """every length 1..152 in one batch, long and short alternating (152, 1, 151, 2, ...): a wave runs tasks of different n back to
    back, so a stale col[r >= n] or a pending subtract carried over would show"""
    rng = random.Random(2611)
    lens = [x for k in range(76) for x in (152 - k, 1 + k)]
    assert sorted(lens) == list(range(1, 153))
    pats = [rand_seq(rng, n) for n in lens]
    txts = [rand_seq(rng, m) for m in (1, 7, 8, 9, 16, 17, 64, 257)]
    txts[7] = txts[7][:100] + pats[0][:120] + txts[7][220:]   # long runs of the diagonal in the longest text
    pa, pb = all_pairs(len(pats), len(txts))
    for scoring in [(1, -1, -1), (5, -4, -4), (2, -3, -1), (2, -3, -5)]:   # (the last: mismatch < gap, the f16 row both times)
        check(pats + txts, pa, pb, scoring)


@pytest.mark.gpu
def test_deferred_subtract_at_block_and_text_edges(ctx):
    """patterns of 1, 2, 3 and 149..152 rows; 72 texts per pattern, the six lengths 1001, 17, 16, 15, 9, 8 twelve times over.  A task
    takes its texts longest first, slot l in the low half of lane l and slot 64 + l in the high half: lanes 0..7 hold a 1001-column
    text below and an 8-column one above, both real and both checked, so one half's text ends 124 blocks before its partner's;
    lanes 8..63 hold one text and an empty partner.  gap 0 and gap -127"""
    rng = random.Random(2612)
    pats = [rand_seq(rng, n) for n in (1, 2, 3, 149, 150, 151, 152)]
    txts = [rand_seq(rng, m) for _ in range(12) for m in (8, 9, 15, 16, 17, 1001)]
    for k in range(5, len(txts), 12):   # every other long text holds the longest pattern
        txts[k] = txts[k][:500] + pats[6] + txts[k][652:]
    assert sorted(len(t) for t in txts)[:12] == [8] * 12 and len(txts) == 72
    pa, pb = all_pairs(len(pats), len(txts))
    for scoring in [(1, -1, -1), (3, 0, 0), (5, -4, 0), (13, -127, -127), (1, -5, -127)]:
        check(pats + txts, pa, pb, scoring)


@pytest.mark.gpu
def test_the_bound_with_a_pad_row_after_the_maximum(ctx):
    """match 23, an 89-row pattern against a text containing it: 89 is odd, so a pad row runs after the maximum; exactly 2047"""
    rng = random.Random(614)
    base = rand_seq(rng, 150)
    for knob in ("1", "0"):
        got, forms = run([base[:89], base], [0], [1], (23, -1, -1), PWA_PROF16="1", PWA_PROF16_INT=knob)
        assert forms == (1, int(knob)) and got == [2047], (knob, forms, got)


@pytest.mark.gpu
def test_padded_cells_count_the_rows_that_run(ctx):
    """100-row patterns: padded_cells = rows run x padded columns x lanes, below the 152-row figure and not below cells"""
    rng = random.Random(2613)
    n_p, n_t, m = 3, 128, 500
    pats = [rand_seq(rng, 100) for _ in range(n_p)]
    txts = [rand_seq(rng, m) for _ in range(n_t)]
    pa, pb = all_pairs(n_p, n_t)
    for n, rows in ((100, 100), (99, 100), (1, 2)):
        with switched_context(**KNOBS, PWA_PROF16="1") as c:
            b = c.batch("sw", [p[:n] for p in pats] + txts, pa, pb, 1, -1, -1)
            assert b.profile_form() == 1
            info = b.info()
            b.close()
        cols = (m + 7) // 8 * 8
        assert info["padded_cells"] == n_p * rows * cols * 128, (n, info)
        assert info["padded_cells"] < n_p * 152 * cols * 128
        assert info["padded_cells"] >= info["cells"] == n_p * n_t * n * m, (n, info)
