"""Banded affine-gap scores on the device (pwa_scores_banded, include/pwalign.h): score and end cell of every pair against the numpy
oracle banded_oracle.py and against pwa_align_banded_batch on the device, which the header says they equal; ties whose answer is
known by construction; the error paths; and a list that PWA_RANGE_BYTES must not cut.  Every comparison is on (score, end)."""
import ctypes as C
import random

import pytest

import banded_oracle as BO
import gotoh_oracle as GO
from conftest import switched_context
from test_gpu_banded import ALPHABETS, HEIGHTS, MAX_WIDTH, SCORINGS, _mixed_pairs, _random_valid_band, _shape_cases, _text_for
from test_gpu_gotoh import _rand

pytestmark = pytest.mark.gpu


def _lists(pairs):
    seqs = [x for pt in pairs for x in pt]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


def _scores(c, mode, pairs, bands, sc, want_end=True):
    seqs, pa, pb = _lists(pairs)
    out = c.scores_banded(mode, seqs, pa, pb, *sc, bands, want_end=want_end)
    if not want_end:
        return out
    s, ei, ej = out
    return [(s[k], (ei[k], ej[k])) for k in range(len(pairs))]


def _want(results):
    return [(w["score"], tuple(w["end"])) for w in results]


def _align(c, mode, pairs, bands, sc):
    seqs, pa, pb = _lists(pairs)
    return _want(c.align_banded_batch(mode, seqs, pa, pb, *sc, bands))


@pytest.fixture(scope="module", params=[4, 8])
def hctx(request):
    with switched_context(PWA_BANDED_RL=str(request.param)) as c:
        c.rl = request.param
        yield c


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("alpha,sc", [("dna", SCORINGS[0]), ("dna", SCORINGS[1]), ("bytes", SCORINGS[0])])
def test_shapes_against_oracle(hctx, mode, alpha, sc):
    """n in {1, 2, 63, 64, 65, S - 1, S, S + 1, 2 S, 2 S + 1, 3001}, m = n + {-37, 0, 50}, half-widths {0, 1, 7, 64, 300}: stripe
    boundaries, the hand-off row, the 16-byte window start and the edge chunks, at both stripe heights"""
    pairs, bands = _shape_cases(mode, HEIGHTS[hctx.rl], ALPHABETS[alpha], 7 * hctx.rl + len(alpha))
    want = _want(BO.align_many(pairs, bands, mode, sc[:2], *sc[2:], group=24))
    got = _scores(hctx, mode, pairs, bands, sc)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (mode, hctx.rl, k, len(pairs[k][0]), len(pairs[k][1]), bands[k])


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
def test_equals_the_alignment_call(ctx, mode):
    """300 mixed pairs, n <= 3000, random valid bands: score and end cell of align_banded_batch, with and without end cells"""
    rng = random.Random(71)
    sc = (2, -3, -5, -2)
    pairs = _mixed_pairs(73, 300, 3000, 3000)
    bands = [_random_valid_band(rng, mode, len(p), len(t)) for p, t in pairs]
    want = _align(ctx, mode, pairs, bands, sc)
    got = _scores(ctx, mode, pairs, bands, sc)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (mode, k, len(pairs[k][0]), len(pairs[k][1]), bands[k])
    assert _scores(ctx, mode, pairs, bands, sc, want_end=False) == [w[0] for w in want]


def test_ties(hctx):
    """|X| = S + 10: the end row lies in the second stripe.  X is random DNA and match = 1, so |X| is the largest score any cell can
    hold and it is reached exactly where a whole copy of X ends on a whole copy of X."""
    S = HEIGHTS[hctx.rl]
    rng = random.Random(79)
    sc = (1, -4, -6, -1)
    X, Y, Z = _rand(rng, S + 10, b"ACGT"), _rand(rng, 30, b"ACGT"), _rand(rng, 45, b"ACGT")
    x = len(X)
    cases = [
        ("sw", X + Y + X, X, (-(x + 30), 0), (x, (x, x))),       # two rows tie: the first row-major one
        ("sw", X, X + Z + X, (0, x + 45), (x, (x, x))),          # the same row, two columns: the smaller j
        ("sg", X, X + Z + X, (0, x + 45), (x, (x, x))),          # row n: the smallest j
    ]
    for mode, p, t, band, want in cases:
        assert band[1] - band[0] + 1 <= MAX_WIDTH
        assert _scores(hctx, mode, [(p, t)], [band], sc) == [want], (mode, hctx.rl, band)
        assert _want([BO.align(p, t, band, mode, sc[:2], *sc[2:])]) == [want], (mode, band)


def test_widest_band(ctx):
    """test_gpu_banded.py's 2200 x 2150 pair under exactly MAX_WIDTH diagonals: the largest hand-off row, NW and SW"""
    rng = random.Random(67)
    p = _rand(rng, 2200, b"ACGT")
    t = _text_for(rng, p, 2150, b"ACGT")
    band = (-2100, MAX_WIDTH - 2101)
    assert band[1] - band[0] + 1 == MAX_WIDTH
    sc = (1, -4, -6, -1)
    for mode in ("nw", "sw"):
        assert _scores(ctx, mode, [(p, t)], [band], sc) == _want([BO.align(p, t, band, mode, sc[:2], *sc[2:])]), mode


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
def test_empty_sides_and_empty_list(ctx, mode):
    sc = (1, -1, -2, -1)
    pairs = [(b"ACG", b""), (b"", b"ACGTA"), (b"", b""), (b"ACGT", b"ACGA")]
    bands = [(-3, 0), (0, 5), (0, 0), (-4, 4)]
    want = [(w["score"], tuple(w["end"])) for w in (GO.result(None, mode, len(p), len(t), sc[2], sc[3]) for p, t in pairs[:3])]
    got = _scores(ctx, mode, pairs, bands, sc)
    assert got[:3] == want
    assert got == _align(ctx, mode, pairs, bands, sc)
    assert ctx.scores_banded(mode, [b"ACG", b"ACGT"], [], [], *sc, [], want_end=True) == ([], [], [])
    assert ctx.scores_banded(mode, [b"ACG", b"ACGT"], [], [], *sc, []) == []


def test_errors(pkg, ctx):
    """test_gpu_banded.py::test_errors through the scores call: the same codes, the first offending pair decides; an invalid list
    leaves the stats of the last valid call as they were"""
    A, Bq = b"ACGTACGTAC", b"ACGTTACGTACG"   # 10 x 12
    def run(mode, band, sc=(1, -1, -2, -1), seqs=(A, Bq)):
        s, ei, ej = ctx.scores_banded(mode, list(seqs), [0], [1], *sc, [band], want_end=True)
        return s[0], (ei[0], ej[0])
    assert run("sw", (3, 5))[0] >= 0
    stats = ctx.scores_banded_stats()
    assert stats["in_band_cells"] == sum(min(10, 12 - d) for d in (3, 4, 5))
    for mode in ("nw", "sw", "sg"):
        with pytest.raises(pkg.PwaError, match="band_lo > band_hi"):
            run(mode, (1, 0))
    for band in [(-1, 1), (1, 3), (-3, -1)]:   # (n, m) = diagonal 2, or (0, 0), outside
        with pytest.raises(pkg.PwaError, match="NW"):
            run("nw", band)
    with pytest.raises(pkg.PwaError, match="SG"):
        run("sg", (3, 5))          # n + lo > m
    with pytest.raises(pkg.PwaError, match="SG"):
        run("sg", (-5, -1))        # band_hi < 0
    with pytest.raises(pkg.PwaError, match="wider"):
        run("nw", (-1, MAX_WIDTH - 1))
    with pytest.raises(pkg.PwaError, match="INVALID|invalid|gap"):
        run("nw", (-2, 4), sc=(1, -1, 1, -1))
    with pytest.raises(pkg.PwaError, match="range"):
        run("nw", (-2, 4), sc=(1 << 24, -1, -2, -1))
    with pytest.raises(pkg.PwaError, match="NW"):
        run("nw", (0, 0), seqs=(b"ACG", b""))
    # the first offending pair decides: pair 0 too wide (CAPACITY) before pair 1's lo > hi (INVALID), and the reverse
    L, h = pkg.lib(), ctx._h
    blob, off, _ = pkg.pack_sequences([A, Bq])
    pa, pb = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 2)(1, 1)
    sc, ei, ej = (C.c_int32 * 2)(), (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
    def raw(lo, hi):
        blo, bhi = (C.c_int32 * 2)(*lo), (C.c_int32 * 2)(*hi)
        return L.pwa_scores_banded(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 2, sc, ei, ej, blo, bhi)
    assert raw((-1, 1), (MAX_WIDTH - 1, 0)) == -5   # PWA_E_CAPACITY
    assert raw((1, -1), (0, MAX_WIDTH - 1)) == -1   # PWA_E_INVALID
    four = (C.c_int32 * 2)(4, 4)
    assert L.pwa_scores_banded(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 2, sc, ei, ej, None, four) == -1   # null band_lo
    assert L.pwa_scores_banded(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 2, sc, ei, ej, (C.c_int32 * 2)(-4, -4), None) == -1
    assert L.pwa_scores_banded(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 2, None, ei, ej, (C.c_int32 * 2)(-4, -4), four) == -1
    assert ctx.scores_banded_stats() == stats
    assert run("nw", (-1, MAX_WIDTH - 2)) == (lambda w: (w["score"], tuple(w["end"])))(GO.align(A, Bq, "nw", (1, -1), -2, -1))
    assert run("nw", (-3, 0), seqs=(b"ACG", b"")) == (lambda w: (w["score"], tuple(w["end"])))(GO.result(None, "nw", 3, 0, -2, -1))


def _cells(n, m, lo, hi):
    """cells (i, j), 1 <= i <= n, 1 <= j <= m, lo <= j - i <= hi (include/pwalign.h: pwa_scores_banded_last_stats)"""
    return sum(max(0, min(m, i + hi) - max(1, i + lo) + 1) for i in range(1, n + 1))


def test_range_bytes_does_not_cut(pkg):
    """64 pairs 1500 x 1500 at half-width 32 under PWA_RANGE_BYTES = 4096, the smallest value the library takes (it raises anything
    lower to that) and one that align_banded_batch still accepts -- one pair per range.  The scores call has no band bytes to budget:
    same scores, and the stats of ONE pass over the whole list."""
    rng = random.Random(83)
    sc = (1, -4, -6, -1)
    pairs = []
    for k in range(64):
        p = _rand(rng, 1500, b"ACGT")
        pairs.append((p, _text_for(rng, p, 1500, b"ACGT")))
    bands = [pkg.band_around(1500, 1500, 32)] * 64
    with switched_context(PWA_RANGE_BYTES="4096") as c:
        want = _align(c, "nw", pairs, bands, sc)
        assert _scores(c, "nw", pairs, bands, sc) == want
        st = c.scores_banded_stats()
    assert st["in_band_cells"] == 64 * _cells(1500, 1500, *bands[0])
    assert st["fill_ms"] > 0
