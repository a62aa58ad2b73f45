"""Banded X-drop extension on the device (pwa_extend_banded_batch / _cigar, pwa_scores_extend_banded; include/pwalign.h: "EXT"):
scores, end cells, rows, op lists, CIGAR and MD:Z byte for byte against the numpy oracle banded_ext_oracle.py (tied to a scalar DP by
test_banded_ext_oracle.py), the scores call against the alignment call, and the error paths.

Stripe heights as in test_gpu_banded.py: PWA_BANDED_RL=4|8 forces 256- or 512-row stripes, so that the stripe-end test is run with
stop rows on both sides of every stripe boundary of either height."""
import ctypes as C
import random

import pytest

import banded_ext_oracle as XO
import banded_oracle as BO
from conftest import load_pkg, switched_context
from test_gpu_banded import ALPHABETS, DELTAS, HEIGHTS, MAX_WIDTH, SCORINGS, WIDTHS, _lengths, _mixed_pairs, _text_for
from test_gpu_cigar import fmt
from test_gpu_gotoh import _mutate, _rand

pytestmark = pytest.mark.gpu

SC = (1, -4, -6, -1)
INV, CAP = -1, -5   # PWA_E_INVALID, PWA_E_CAPACITY


def _seqs(pairs):
    seqs = [x for pt in pairs for x in pt]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


def _call(c, pairs, bands, sc, xdrop, cigar=False):
    seqs, pa, pb = _seqs(pairs)
    fn = c.extend_banded_batch_cigar if cigar else c.extend_banded_batch
    return fn(seqs, pa, pb, *sc, bands, xdrop)


def _scores(c, pairs, bands, sc, xdrop, want_end=True):
    seqs, pa, pb = _seqs(pairs)
    return c.scores_extend_banded(seqs, pa, pb, *sc, bands, xdrop, want_end=want_end)


def _whole(pairs, bands, sc, xdrop, **kw):
    """the oracle's results as pwa_extend_banded_batch returns them: every key but the pattern end, which that call does not have"""
    return [{k: v for k, v in w.items() if k != "pend"} for w in XO.extend_many(pairs, bands, sc[:2], *sc[2:], xdrop, **kw)]


def _check(c, pairs, bands, sc, xdrop, want, tag):
    """test_gpu_banded._check with start = (0, 0) and rows: the op-list call, the string call and the scores call"""
    got, gc = _call(c, pairs, bands, sc, xdrop), _call(c, pairs, bands, sc, xdrop, cigar=True)
    s, ei, ej, rw = _scores(c, pairs, bands, sc, xdrop)
    for k, (g, cg, w) in enumerate(zip(got, gc, want)):
        p, t = pairs[k]
        key = (tag, xdrop, k, len(p), len(t), bands[k])
        assert w["start"] == (0, 0), key
        assert (g["score"], g["end"], g["start"], g["rows"]) == (w["score"], w["end"], (0, 0), w["rows"]), key
        assert g["ops"] == w["ops"], key
        assert (cg["score"], cg["end"], cg["start"], cg["rows"]) == (w["score"], w["end"], (0, 0), w["rows"]), key
        assert (cg["cigar"], cg["mdz"]) == fmt(p, t, w["ops"], (0, 0)), key
        assert (s[k], (ei[k], ej[k]), rw[k]) == (w["score"], w["end"], w["rows"]), key
    return got


@pytest.fixture(scope="module", params=[4, 8])
def hctx(request):
    with switched_context(PWA_BANDED_RL=str(request.param)) as c:
        c.rl = request.param
        yield c


def _shape_cases(S, alpha, seed):
    pkg = load_pkg()
    rng = random.Random(seed)
    pairs, bands = [], []
    for n in _lengths(S):
        widths = WIDTHS if n <= 2 * S + 1 else [7, 300]
        p = _rand(rng, n, alpha)
        for d in DELTAS:
            m = max(1, n + d)
            t = _text_for(rng, p, m, alpha)
            for w in widths:
                pairs.append((p, t))
                bands.append(pkg.band_around(n, m, w, diag=0))
    return pairs, bands


@pytest.mark.parametrize("alpha,sc", [("dna", SCORINGS[0]), ("dna", SCORINGS[1]), ("bytes", SCORINGS[0])])
def test_shapes_against_oracle(hctx, alpha, sc):
    pairs, bands = _shape_cases(HEIGHTS[hctx.rl], ALPHABETS[alpha], 11 * hctx.rl + len(alpha))
    want = XO.extend_multi(pairs, bands, sc[:2], *sc[2:], [-1, 30], group=24)
    for xdrop in (-1, 30):
        _check(hctx, pairs, bands, sc, xdrop, want[xdrop], ("shapes", hctx.rl))
    assert any(w["rows"] < len(p) for w, (p, t) in zip(want[30], pairs))   # (the drop does stop some of them)


def test_stop_rows_at_the_stripe_edges(hctx):
    """X + A.. against X + C..: the best cell is (|X|, |X|), and the column-|X| deletion run falls 20 below it 15 rows later, so
    rows = |X| + 14 -- placed by the oracle on both sides of the first two stripe boundaries"""
    S = HEIGHTS[hctx.rl]
    targets = [S - 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1]
    rng = random.Random(71)
    pairs, bands, want = [], [], []
    for rows in targets:
        for tries in range(8):   # (a chance match at the seam can move the stop by a row: draw X again)
            x = _rand(rng, rows - 14, b"ACGT")
            pair, band = (x + b"A" * 600, x + b"C" * 600), (-32, 32)
            w = XO.extend(*pair, band, SC[:2], *SC[2:], 20)
            if w["rows"] == rows:
                break
        pairs.append(pair)
        bands.append(band)
        want.append(w)
    assert [w["rows"] for w in want] == targets
    assert all(w["end"] == (r - 14, r - 14) and w["score"] == r - 14 for w, r in zip(want, targets))
    _check(hctx, pairs, bands, SC, 20, want, ("edges", hctx.rl))


def test_the_drop_changes_the_answer(hctx):
    rng = random.Random(73)
    x, y = _rand(rng, 200, b"ACGT"), _rand(rng, 600, b"ACGT")
    pair, band = (x + _rand(rng, 60, b"AC") + y, x + _rand(rng, 60, b"GT") + y), (-40, 40)   # R1, R2 share no symbol
    want = XO.extend_multi([pair], [band], SC[:2], *SC[2:], [30, -1])
    stop, free = want[30][0], want[-1][0]
    assert (stop["score"], stop["end"]) == (200, (200, 200)) and 200 < stop["rows"] < 260
    assert free["end"] == (860, 860) and free["score"] > 200 and free["rows"] == 860
    got = {xd: _check(hctx, [pair], [band], SC, xd, want[xd], ("drop", hctx.rl))[0] for xd in (30, -1)}
    assert got[30] != got[-1]


def test_ties_and_the_anchor(hctx):
    rng = random.Random(79)
    x, z = _rand(rng, 300, b"ACGT"), _rand(rng, 77, b"ACGT")
    # the whole pattern twice in the text, on diagonals 0 and |X| + |Z|: equal maxima in row |X|, the first one wins
    pairs, bands = [(x, x + z + x)], [(0, 377)]
    # first symbols differ, then a copy: nothing reaches above the anchor's 0 before the drop
    pairs.append((b"G" + x, b"C" + x))
    bands.append((-5, 5))
    for xdrop in (-1, 3):
        want = XO.extend_many(pairs[:1], bands[:1], SC[:2], *SC[2:], xdrop)
        assert want[0]["end"] == (300, 300) and want[0]["score"] == 300
        _check(hctx, pairs[:1], bands[:1], SC, xdrop, want, ("ties", hctx.rl))
    want = XO.extend_many(pairs[1:], bands[1:], SC[:2], *SC[2:], 3)
    assert (want[0]["score"], want[0]["end"], want[0]["ops"]) == (0, (0, 0), b"")
    got = _check(hctx, pairs[1:], bands[1:], SC, 3, want, ("anchor", hctx.rl))
    assert _call(hctx, pairs[1:], bands[1:], SC, 3, cigar=True)[0]["cigar"] == b"" and got[0]["ops"] == b""
    # the best local hit is off the anchor: SW on the same band scores higher than the extension
    pairs, bands = [(b"G" * 20 + x, b"C" * 20 + x)], [(-10, 10)]
    seqs, pa, pb = _seqs(pairs)
    sw = hctx.scores_banded("sw", seqs, pa, pb, *SC, bands)
    for xdrop in (-1, 30):
        want = XO.extend_many(pairs, bands, SC[:2], *SC[2:], xdrop)
        got = _check(hctx, pairs, bands, SC, xdrop, want, ("off-anchor", hctx.rl))
        assert got[0]["score"] < sw[0] == 300


def _random_ext_band(rng):
    k1, k2 = rng.choice([(0, 0), (rng.randint(0, 40), rng.randint(0, 40)), (rng.randint(0, 400), rng.randint(0, 400))])
    return (-k1, k2)


@pytest.mark.parametrize("xdrop", [-1, 25])
def test_scores_equal_alignments(ctx, xdrop):
    sc = (2, -3, -5, -2)
    rng = random.Random(83)
    pairs = _mixed_pairs(85, 300, 3000, 3000)
    bands = [_random_ext_band(rng) for _ in pairs]
    got = _call(ctx, pairs, bands, sc, xdrop)
    s, ei, ej, rw = _scores(ctx, pairs, bands, sc, xdrop)
    assert [(g["score"], g["end"], g["rows"]) for g in got] == list(zip(s, zip(ei, ej), rw))
    assert _scores(ctx, pairs, bands, sc, xdrop, want_end=False) == s
    ks = list(range(0, 300, 13))
    want = _whole([pairs[k] for k in ks], [bands[k] for k in ks], sc, xdrop, group=8)
    for x, k in enumerate(ks):
        assert got[k] == want[x], (k, len(pairs[k][0]), len(pairs[k][1]), bands[k])


def test_widest_band(ctx):
    """test_gpu_banded.test_widest_band's 2200 x 2150 pair under MAX_WIDTH diagonals that hold diagonal 0"""
    rng = random.Random(67)
    p = _rand(rng, 2200, b"ACGT")
    t = _text_for(rng, p, 2150, b"ACGT")
    band = (-2100, MAX_WIDTH - 2101)
    assert band[1] - band[0] + 1 == MAX_WIDTH and band[0] <= 0 <= band[1]
    want = XO.extend_multi([(p, t)], [band], SC[:2], *SC[2:], [-1, 40])
    for xdrop in (-1, 40):
        _check(ctx, [(p, t)], [band], SC, xdrop, want[xdrop], "widest")


def test_empty_sides_and_empty_list(ctx):
    sc = (1, -1, -2, -1)
    pairs = [(b"ACG", b""), (b"", b"ACGTA"), (b"", b""), (b"ACGT", b"ACGA")]
    bands = [(-3, 0), (0, 5), (0, 0), (-4, 4)]
    zero = dict(score=0, ops=b"", end=(0, 0), start=(0, 0), rows=0)
    for xdrop in (-1, 5):
        want = _whole(pairs, bands, sc, xdrop)
        assert want[:3] == [zero] * 3 and want[3]["score"] == 3
        got = _check(ctx, pairs, bands, sc, xdrop, want, "empty")
        assert got[:3] == [zero] * 3
    seqs = [b"ACG", b"ACGT"]
    assert ctx.extend_banded_batch(seqs, [], [], *sc, [], 5) == []
    assert ctx.extend_banded_batch_cigar(seqs, [], [], *sc, [], 5) == []
    assert ctx.scores_extend_banded(seqs, [], [], *sc, [], 5, want_end=True) == ([], [], [], [])
    assert ctx.scores_extend_banded(seqs, [], [], *sc, [], 5) == []
    with pytest.raises(load_pkg().PwaError, match="EXT"):   # an empty side does not excuse the band
        ctx.extend_banded_batch([b"ACG", b""], [0], [1], *sc, [(1, 2)], 5)


def test_errors(pkg, ctx):
    A, Bq = b"ACGTACGTAC", b"ACGTTACGTACG"   # 10 x 12
    def run(band, sc=(1, -1, -2, -1), xdrop=10, seqs=(A, Bq)):
        return ctx.extend_banded_batch(list(seqs), [0], [1], *sc, [band], xdrop)
    good = run((-2, 4))
    assert good == _whole([(A, Bq)], [(-2, 4)], (1, -1, -2, -1), 10)
    stats = ctx.extend_banded_stats()
    assert stats["rows_considered"] == good[0]["rows"] and stats["fill_ms"] > 0 and stats["walk_ms"] > 0
    with pytest.raises(pkg.PwaError, match="band_lo > band_hi"):
        run((1, 0))
    for band in [(1, 3), (-3, -1)]:   # the anchor outside the band
        with pytest.raises(pkg.PwaError, match="EXT"):
            run(band)
    with pytest.raises(pkg.PwaError, match="wider"):
        run((-1, MAX_WIDTH - 1))
    assert run((-1, MAX_WIDTH - 2)) == _whole([(A, Bq)], [(-1, MAX_WIDTH - 2)], (1, -1, -2, -1), 10)
    with pytest.raises(pkg.PwaError, match="INVALID|invalid|gap"):
        run((-2, 4), sc=(1, -1, 1, -1))
    with pytest.raises(pkg.PwaError, match="xdrop"):
        run((-2, 4), xdrop=(1 << 27) + 1)
    assert run((-2, 4), xdrop=1 << 27) == _whole([(A, Bq)], [(-2, 4)], (1, -1, -2, -1), 1 << 27)
    # beyond EXT's 2^27 range rule, inside the banded rule's 2^28: 24 * 2^23 = 1.5 * 2^27
    with pytest.raises(pkg.PwaError, match="range"):
        run((-2, 4), sc=(1 << 23, -1, -2, -1))
    assert ctx.align_banded_batch("nw", [A, Bq], [0], [1], 1 << 23, -1, -2, -1, [(-2, 4)])[0]["end"] == (10, 12)
    run((-2, 4))
    stats = ctx.extend_banded_stats()   # of the last valid call; every failing call below must leave them alone
    # the first offending pair decides, and inside a pair lo > hi, then the anchor, then the width
    L, h = pkg.lib(), ctx._h
    blob, off, _ = pkg.pack_sequences([A, Bq])
    pa, pb = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 2)(1, 1)
    sc, nops, oo = (C.c_int32 * 2)(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)(0, 22)
    ops = C.create_string_buffer(64)
    def arr(v):
        return None if v is None else (C.c_int32 * 2)(*v)
    def raw(lo, hi, score=sc, xdrop=10):
        return L.pwa_extend_banded_batch(h, 1, -1, -2, -1, xdrop, blob, off, 2, pa, pb, 2, score, ops, oo, nops, None, None, arr(lo), arr(hi))
    def raw_scores(lo, hi, score=sc):
        return L.pwa_scores_extend_banded(h, 1, -1, -2, -1, 10, blob, off, 2, pa, pb, 2, score, None, None, None, arr(lo), arr(hi))
    assert raw((-1, 1), (MAX_WIDTH - 1, 0)) == CAP      # pair 0 too wide before pair 1's lo > hi
    assert raw((1, -1), (0, MAX_WIDTH - 1)) == INV      # ... and the reverse
    assert raw((-1, 1), (MAX_WIDTH - 1, 2)) == CAP      # ... before pair 1's anchor
    assert raw((1, -1), (MAX_WIDTH + 5, 1)) == INV      # pair 0: the anchor before the width
    assert raw((-1, -1), (1, 1), xdrop=(1 << 27) + 1) == INV
    assert raw((-1, -1), (1, 1), score=None) == INV and raw(None, (1, 1)) == INV and raw((-1, -1), None) == INV
    assert raw_scores((-1, -1), (1, 1), score=None) == INV and raw_scores(None, (1, 1)) == INV and raw_scores((-1, -1), None) == INV
    assert raw_scores((-1, 1), (MAX_WIDTH - 1, 0)) == CAP and raw_scores((1, -1), (0, MAX_WIDTH - 1)) == INV
    assert ctx.extend_banded_stats() == stats            # unchanged by every call that failed validation
    rows = sum(w["rows"] for w in XO.extend_many([(A, Bq)] * 2, [(-1, 1), (-2, 4)], (1, -1), -2, -1, 10))
    assert raw((-1, -2), (1, 4)) == 0
    assert ctx.extend_banded_stats()["rows_considered"] == rows
    assert raw_scores((-1, -2), (1, 4)) == 0
    st = ctx.extend_banded_stats()
    assert st["rows_considered"] == rows and st["walk_ms"] == 0 and st["fill_ms"] > 0
    # the existing calls still know three modes
    assert L.pwa_align_banded_batch(h, 3, 1, -1, -2, -1, blob, off, 2, pa, pb, 2, sc, ops, oo, nops, None, None, arr((-2, -2)), arr((4, 4))) == INV


def test_range_bytes(ctx):
    """64 pairs 1500 x 1500 cut into one pair per range: the uncut call's results, stats summed over the ranges"""
    rng = random.Random(89)
    pairs = []
    for k in range(64):
        p = _rand(rng, 1500, b"ACGT")
        t = _mutate(rng, p, b"ACGT", rate=0.05)[:900 + 9 * k] + _rand(rng, 1500, b"ACGT")
        pairs.append((p, t[:1500]))
    bands = [(-30, 30)] * 64
    got, gc = _call(ctx, pairs, bands, SC, 40), _call(ctx, pairs, bands, SC, 40, cigar=True)
    rows = sum(g["rows"] for g in got)
    assert ctx.extend_banded_stats()["rows_considered"] == rows and any(g["rows"] < 1500 for g in got)
    ks = list(range(0, 64, 9))
    assert [got[k] for k in ks] == _whole([pairs[k] for k in ks], [bands[k] for k in ks], SC, 40)
    with switched_context(PWA_RANGE_BYTES="4096") as c:
        assert _call(c, pairs, bands, SC, 40) == got
        assert c.extend_banded_stats()["rows_considered"] == rows
        assert _call(c, pairs, bands, SC, 40, cigar=True) == gc
