"""Banded X-drop extension under a substitution matrix on the device (pwa_extend_banded_subst_batch / _cigar,
pwa_scores_extend_banded_subst; include/pwalign.h): scores, end cells, rows, the pattern-end result, op lists, CIGAR and MD:Z byte for
byte against the numpy oracle banded_ext_oracle.py under the table (tied to a scalar DP, to its byte compare and to banded_oracle by
test_banded_ext_subst_oracle.py); the scores call against the alignment call; the byte-compare EXT calls under a match / mismatch
table; and the error paths, all of which are host-side refusals.

Stripe heights as in test_gpu_banded.py: PWA_BANDED_RL=4|8 forces 256- or 512-row stripes, so that the stripe-end test and the
pattern-end store run with row n and with stop rows on both sides of every stripe boundary of either height."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import banded_ext_oracle as XO
from conftest import load_pkg, switched_context
from test_gpu_banded import DELTAS, HEIGHTS, MAX_WIDTH, WIDTHS, _lengths, _mixed_pairs, _text_for
from test_gpu_banded_subst import _table
from test_gpu_cigar import fmt
from test_gpu_gotoh import _mutate, _rand

pytestmark = pytest.mark.gpu

INV, CAP = -1, -5   # PWA_E_INVALID, PWA_E_CAPACITY


def _seqs(pairs):
    seqs = [x for pt in pairs for x in pt]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


def _call(c, pairs, bands, table, go, ge, xdrop, cigar=False):
    seqs, pa, pb = _seqs(pairs)
    fn = c.extend_banded_subst_batch_cigar if cigar else c.extend_banded_subst_batch
    return fn(seqs, pa, pb, table, go, ge, bands, xdrop)


def _scores(c, pairs, bands, table, go, ge, xdrop, want_end=True):
    seqs, pa, pb = _seqs(pairs)
    return c.scores_extend_banded_subst(seqs, pa, pb, table, go, ge, bands, xdrop, want_end=want_end)


def _check(c, pairs, bands, table, go, ge, xdrop, want, tag):
    """the op-list call, the string call and the scores call of one list against the oracle's results"""
    got, gc = _call(c, pairs, bands, table, go, ge, xdrop), _call(c, pairs, bands, table, go, ge, xdrop, cigar=True)
    s, ei, ej, rw, pe = _scores(c, pairs, bands, table, go, ge, xdrop)
    assert len(got) == len(gc) == len(s) == len(want)
    for k, (g, cg, w) in enumerate(zip(got, gc, want)):
        p, t = pairs[k]
        key = (tag, xdrop, k, len(p), len(t), bands[k])
        assert w["start"] == (0, 0), key
        assert (g["score"], g["end"], g["start"], g["rows"], g["pend"]) == (w["score"], w["end"], (0, 0), w["rows"], w["pend"]), key
        assert g["ops"] == w["ops"], key
        assert (cg["score"], cg["end"], cg["start"], cg["rows"], cg["pend"]) == (w["score"], w["end"], (0, 0), w["rows"], w["pend"]), key
        assert (cg["cigar"], cg["mdz"]) == fmt(p, t, w["ops"], (0, 0)), key
        assert (s[k], (ei[k], ej[k]), rw[k], pe[k]) == (w["score"], w["end"], w["rows"], w["pend"]), key
    return got


@pytest.fixture(scope="module", params=[4, 8])
def hctx(request):
    with switched_context(PWA_BANDED_RL=str(request.param)) as c:
        c.rl = request.param
        yield c


def _small_table(name):
    """4-symbol tables: `asym` asymmetric with mixed signs, `pos` with positive off-diagonal entries, `neg` all negative"""
    pkg = load_pkg()
    rs = np.random.RandomState(5)
    if name == "asym":
        m = rs.randint(-5, 2, size=(4, 4))
        m[np.arange(4), np.arange(4)] = [3, 2, 4, 1]
        assert (m != m.T).any()
    elif name == "pos":
        m = np.full((4, 4), -3)
        m[np.arange(4), np.arange(4)] = 4
        m[0, 2] = m[2, 0] = 1
        m[1, 3] = 2
    else:
        m = -1 - rs.randint(0, 4, size=(4, 4))
    return pkg.subst_table(b"ACGT", m)


@functools.lru_cache(maxsize=None)
def _shape_set(S):
    """test_gpu_banded's lengths, deltas and widths around diagonal 0 under the DNA table (neutral N, folded lower case, transitions
    apart from transversions), and the oracle's results at two drops"""
    pkg = load_pkg()
    table, go, ge, alpha = _table("dna")
    rng = random.Random(13 * S)
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
    return pairs, bands, XO.extend_multi(pairs, bands, table, go, ge, [-1, 60], group=24)


def test_shapes_against_oracle(hctx):
    table, go, ge, _ = _table("dna")
    pairs, bands, want = _shape_set(HEIGHTS[hctx.rl])
    for xdrop in (-1, 60):
        _check(hctx, pairs, bands, table, go, ge, xdrop, want[xdrop], ("shapes", hctx.rl))
    assert any(w["rows"] < len(p) for w, (p, t) in zip(want[60], pairs))   # (the drop does stop some of them)
    assert any(w["pend"] is not None and w["pend"][0] < w["score"] for w in want[-1])


@pytest.mark.parametrize("n_sym", [1, 4, 5, 24, 32])
def test_alphabet_sizes(pkg, hctx, n_sym):
    """n_sym = 1: one entry; 4: an asymmetric table; 5: the DNA table; 24: the protein-like table (asymmetric, positive off-diagonal
    entries, a wildcard); 32: the full table at the even row stride"""
    if n_sym == 4:
        table, go, ge, alpha = _small_table("asym"), -5, -1, b"ACGT"
    elif n_sym == 5:
        table, go, ge, alpha = _table("dna")
    elif n_sym == 24:
        table, go, ge, alpha = _table("protein")
    else:
        alpha = bytes(range(65, 65 + n_sym))
        m = np.random.RandomState(n_sym).randint(-6, 9, size=(n_sym, n_sym))
        m[np.arange(n_sym), np.arange(n_sym)] = np.random.RandomState(n_sym + 1).randint(1, 9, size=n_sym)
        table, go, ge = pkg.subst_table(alpha, m), -3, -1
    rng = random.Random(137 + n_sym)
    S = HEIGHTS[hctx.rl]
    pairs, bands = [], []
    for n, d, w in [(S + 1, 0, 7), (70, 50, 64), (2 * S + 1, -37, 20), (5, 0, 1), (S, 20, 40)]:
        p = _rand(rng, n, alpha)
        pairs.append((p, _text_for(rng, p, n + d, alpha)))
        bands.append(pkg.band_around(n, n + d, w, diag=0))
    want = XO.extend_multi(pairs, bands, table, go, ge, [-1, 25])
    for xdrop in (-1, 25):
        _check(hctx, pairs, bands, table, go, ge, xdrop, want[xdrop], ("n_sym", n_sym, hctx.rl))


@pytest.mark.parametrize("name", ["pos", "neg"])
def test_positive_off_diagonal_and_all_negative_tables(hctx, name):
    """`pos`: mismatches that raise the score; `neg`: the extension never leaves the anchor -- score 0 at (0, 0), no ops, yet rows and
    the pattern end say how far the sweep went"""
    pkg = load_pkg()
    table = _small_table(name)
    rng = random.Random(139)
    S = HEIGHTS[hctx.rl]
    pairs, bands = [], []
    for n, d, w in [(S + 2, 5, 9), (90, 0, 3), (2 * S, 0, 30), (40, 0, 40)]:
        p = _rand(rng, n, b"ACGT")
        pairs.append((p, _text_for(rng, p, n + d, b"ACGT")))
        bands.append(pkg.band_around(n, n + d, w, diag=0))
    want = XO.extend_multi(pairs, bands, table, -4, -1, [-1, 15, 1 << 27])
    for xdrop in (-1, 15, 1 << 27):
        got = _check(hctx, pairs, bands, table, -4, -1, xdrop, want[xdrop], (name, hctx.rl))
        if name == "neg":
            assert all((g["score"], g["end"], g["ops"]) == (0, (0, 0), b"") for g in got)
    if name == "neg":
        assert all(w["rows"] < len(p) and w["pend"] is None for w, (p, t) in zip(want[15], pairs))
        assert all(w["rows"] == len(p) and w["pend"][0] < 0 for w, (p, t) in zip(want[-1], pairs))


def _stop_at(rng, table, go, ge, rows, tail):
    """X + A.. against X + C..: the best cell is (|X|, |X|), and the column-|X| deletion run falls 20 below it 15 rows later, so the
    sweep keeps |X| + 14 rows -- X drawn again until the oracle places `rows` exactly (a chance match at the seam can move the stop)"""
    for tries in range(40):
        x = _rand(rng, rows - 14, b"ACGT")
        pair, band = (x + b"A" * tail, x + b"C" * 600), (-32, 32)
        w = XO.extend(*pair, band, table, go, ge, 20)
        if w["rows"] == min(rows, len(pair[0])) and w["end"] == (rows - 14, rows - 14):
            return pair, band, w
    raise AssertionError("no X places the stop at row %d" % (rows + 1))


def test_stop_rows_at_the_stripe_edges(hctx):
    S = HEIGHTS[hctx.rl]
    table = load_pkg().subst_table(b"ACGTN", np.where(np.eye(5, dtype=bool), 1, -4) * np.array([1, 1, 1, 1, 0])[None, :], unknown=4)
    targets = [S - 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1]
    rng = random.Random(71)
    pairs, bands, want = [], [], []
    for rows in targets:
        pair, band, w = _stop_at(rng, table, -6, -1, rows, 600)
        pairs.append(pair)
        bands.append(band)
        want.append(w)
    assert [w["rows"] for w in want] == targets and all(w["pend"] is None for w in want)
    _check(hctx, pairs, bands, table, -6, -1, 20, want, ("edges", hctx.rl))


def test_the_drop_changes_the_answer_and_equal_maxima(hctx):
    table, go, ge, _ = _table("dna")
    rng = random.Random(73)
    x, y = _rand(rng, 200, b"ACGT"), _rand(rng, 600, b"ACGT")
    pair, band = (x + _rand(rng, 60, b"AC") + y, x + _rand(rng, 60, b"GT") + y), (-40, 40)
    want = XO.extend_multi([pair], [band], table, go, ge, [30, -1])
    stop, free = want[30][0], want[-1][0]
    assert stop["end"][0] < 260 and stop["rows"] < 300 and stop["pend"] is None
    assert free["end"] == (860, 860) and free["score"] > stop["score"] and free["rows"] == 860 and free["pend"] == (free["score"], 860)
    got = {xd: _check(hctx, [pair], [band], table, go, ge, xd, want[xd], ("drop", hctx.rl))[0] for xd in (30, -1)}
    assert got[30] != got[-1]
    # the whole pattern twice in the text, on diagonals 0 and |X| + |Z|: equal maxima in row |X| = n -- the first one wins, in the
    # best cell and in the pattern end alike
    x, z = _rand(rng, 300, b"ACGT"), _rand(rng, 77, b"ACGT")
    for xdrop in (-1, 3):
        want = XO.extend_many([(x, x + z + x)], [(0, 377)], table, go, ge, xdrop)
        assert want[0]["end"] == (300, 300) and want[0]["score"] == 900 and want[0]["pend"] == (900, 300)
        _check(hctx, [(x, x + z + x)], [(0, 377)], table, go, ge, xdrop, want, ("ties", hctx.rl))


def test_pattern_end_rows(hctx):
    """row n in the first and in the last row slot of a lane, in lane 0 and in lane 63, n = S, S + 1, 2 S (the last row of a stripe,
    the first row of the next, the last row of the second): every pair reaches its pattern's end"""
    table, go, ge, alpha = _table("dna")
    RL, S = hctx.rl, HEIGHTS[hctx.rl]
    ns = [1, 2, RL, RL + 1, S - RL, S - RL + 1, S - 1, S, S + 1, S + RL, S + RL + 1, 2 * S - RL + 1, 2 * S, 2 * S + 1]
    rng = random.Random(149)
    pairs, bands = [], []
    for n in ns:
        p = _rand(rng, n, alpha)
        pairs.append((p, _text_for(rng, p, n + 40, alpha)))
        bands.append((-20, 20))
    want = XO.extend_multi(pairs, bands, table, go, ge, [-1, 1 << 27])
    for xdrop in (-1, 1 << 27):   # (the largest drop: only a row without a cell would stop)
        assert all(w["pend"] is not None and w["rows"] == n for w, n in zip(want[xdrop], ns))
        _check(hctx, pairs, bands, table, go, ge, xdrop, want[xdrop], ("pend rows", hctx.rl))


def test_pattern_end_below_the_best_and_stopped_at_row_n(hctx):
    pkg = load_pkg()
    S = HEIGHTS[hctx.rl]
    table = pkg.subst_table(b"ACGTN", np.where(np.eye(5, dtype=bool), 1, -4) * np.array([1, 1, 1, 1, 0])[None, :], unknown=4)
    rng = random.Random(151)
    pairs, bands, want = [], [], []
    for n in (S, S + 1, 2 * S):
        # a tail of 14 rows keeps row n = |X| + 14: the pattern end lies 20 below the best, whose row is |X| < n ...
        pair, band, w = _stop_at(rng, table, -6, -1, n, 14)
        assert len(pair[0]) == n and w["rows"] == n and w["end"][0] == n - 14 and w["pend"][0] == w["score"] - 20
        pairs.append(pair), bands.append(band), want.append(w)
        # ... and one row more is the first to stop: exactly row n, so there is no pattern end
        pair, band, w = _stop_at(rng, table, -6, -1, n - 1, 15)
        assert len(pair[0]) == n and w["rows"] == n - 1 and w["pend"] is None
        pairs.append(pair), bands.append(band), want.append(w)
    _check(hctx, pairs, bands, table, -6, -1, 20, want, ("pend below / stopped", hctx.rl))


def test_pattern_end_none_and_empty_sides(hctx):
    table, go, ge, alpha = _table("dna")
    S = HEIGHTS[hctx.rl]
    rng = random.Random(157)
    x = _rand(rng, S + 40, alpha)
    # the band leaves the matrix before row n (rows = m - lo = S - 20 < n): no pattern end even when no row may stop
    pairs, bands = [(x, x[:S - 30])], [(-10, 10)]
    pairs += [(b"ACG", b""), (b"", b"ACGTN"), (b"", b""), (b"ACGT", b"ACGA")]
    bands += [(-3, 0), (0, 5), (0, 0), (-4, 4)]
    for xdrop in (-1, 50):   # (50: the ten rows below the text's end fall 16 at most; row S - 19 has no cell and stops)
        want = XO.extend_many(pairs, bands, table, go, ge, xdrop)
        assert want[0]["rows"] == S - 20 and want[0]["pend"] is None
        assert [w["pend"] for w in want[1:4]] == [None, (0, 0), (0, 0)] and all(w["rows"] == 0 and w["score"] == 0 for w in want[1:4])
        assert want[4]["pend"] is not None
        _check(hctx, pairs, bands, table, go, ge, xdrop, want, ("none", hctx.rl))
    seqs = [b"ACG", b"ACGT"]
    assert hctx.extend_banded_subst_batch(seqs, [], [], table, go, ge, [], 5) == []
    assert hctx.extend_banded_subst_batch_cigar(seqs, [], [], table, go, ge, [], 5) == []
    assert hctx.scores_extend_banded_subst(seqs, [], [], table, go, ge, [], 5, want_end=True) == ([], [], [], [], [])
    assert hctx.scores_extend_banded_subst(seqs, [], [], table, go, ge, [], 5) == []
    with pytest.raises(load_pkg().PwaError, match="EXT"):   # an empty side does not excuse the band
        hctx.extend_banded_subst_batch([b"ACG", b""], [0], [1], table, go, ge, [(1, 2)], 5)


def _random_ext_band(rng):
    k1, k2 = rng.choice([(0, 0), (rng.randint(0, 40), rng.randint(0, 40)), (rng.randint(0, 400), rng.randint(0, 400))])
    return (-k1, k2)


def test_match_mismatch_table_equals_the_byte_compare_calls_and_nw_on_the_prefix(pkg, ctx):
    """300 mixed DNA pairs, random bands that hold the anchor, match on the diagonal and mismatch off it: exactly the outputs of
    extend_banded_batch, extend_banded_batch_cigar and scores_extend_banded, plus the pattern end, on which the three table calls
    agree -- and which is scores_banded_subst("nw") of the pattern against the text's first pend_j symbols under the same band"""
    match, mismatch, go, ge = 2, -3, -5, -2
    table = pkg.subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), match, mismatch))
    rng = random.Random(163)
    pairs = _mixed_pairs(167, 300, 3000, 3000)
    bands = [_random_ext_band(rng) for _ in pairs]
    seqs, pa, pb = _seqs(pairs)
    for xdrop in (-1, 25):
        got, gc = _call(ctx, pairs, bands, table, go, ge, xdrop), _call(ctx, pairs, bands, table, go, ge, xdrop, cigar=True)
        pend = [g.pop("pend") for g in got]
        assert [g.pop("pend") for g in gc] == pend
        assert got == ctx.extend_banded_batch(seqs, pa, pb, match, mismatch, go, ge, bands, xdrop)
        assert gc == ctx.extend_banded_batch_cigar(seqs, pa, pb, match, mismatch, go, ge, bands, xdrop)
        s, ei, ej, rw, pe = _scores(ctx, pairs, bands, table, go, ge, xdrop)
        assert (s, ei, ej, rw) == ctx.scores_extend_banded(seqs, pa, pb, match, mismatch, go, ge, bands, xdrop, want_end=True)
        assert pe == pend and _scores(ctx, pairs, bands, table, go, ge, xdrop, want_end=False) == s
        assert [x is not None for x in pend] == [g["rows"] == len(p) for g, (p, t) in zip(got, pairs)]
        ks = [k for k, x in enumerate(pend) if x is not None and x[1] >= 1]
        assert len(ks) >= 20
        prefix = [(pairs[k][0], pairs[k][1][:pend[k][1]]) for k in ks]
        qs, qa, qb = _seqs(prefix)
        assert ctx.scores_banded_subst("nw", qs, qa, qb, table, go, ge, [bands[k] for k in ks]) == [pend[k][0] for k in ks]
        ko = list(range(0, 300, 17))
        want = XO.extend_many([pairs[k] for k in ko], [bands[k] for k in ko], table, go, ge, xdrop, group=8)
        for x, k in enumerate(ko):
            assert dict(got[k], pend=pend[k]) == want[x], (k, len(pairs[k][0]), len(pairs[k][1]), bands[k])


def test_widest_band(hctx):
    """a 2200 x 2150 pair under MAX_WIDTH diagonals that hold diagonal 0: the hand-off rows at their largest beside the static table"""
    table, go, ge, alpha = _table("protein")
    rng = random.Random(67)
    p = _rand(rng, 2200, alpha)
    t = _text_for(rng, p, 2150, alpha)
    band = (-2100, MAX_WIDTH - 2101)
    assert band[1] - band[0] + 1 == MAX_WIDTH and band[0] <= 0 <= band[1]
    want = XO.extend_multi([(p, t)], [band], table, go, ge, [-1, 40], group=1)
    for xdrop in (-1, 40):
        _check(hctx, [(p, t)], [band], table, go, ge, xdrop, want[xdrop], ("widest", hctx.rl))


def test_folded_case_is_a_match_that_mdz_reports_as_a_mismatch(ctx):
    table, go, ge, _ = _table("dna")
    p, t = b"ACGTACGTACGTACGTACGT", b"ACGTacgtACGTACGTACGTTT"
    want = XO.extend(p, t, (-3, 3), table, go, ge, 10)
    assert want["score"] == 60 and want["ops"] == b"M" * 20 and want["pend"] == (60, 20)
    got = _check(ctx, [(p, t)], [(-3, 3)], table, go, ge, 10, [want], "fold")
    cg = _call(ctx, [(p, t)], [(-3, 3)], table, go, ge, 10, cigar=True)[0]
    assert got[0]["score"] == 60 and cg["cigar"] == b"20M" and cg["mdz"] == b"4a0c0g0t12"


def test_range_bytes(ctx):
    """64 pairs 1500 x 1500 cut into one pair per range, every range launched with the table uploaded once for the call: the uncut
    call's results, the pattern ends among them, and its stats summed over the ranges"""
    table, go, ge, _ = _table("dna")
    rng = random.Random(89)
    pairs = []
    for k in range(64):
        p = _rand(rng, 1500, b"ACGT")
        t = _mutate(rng, p, b"ACGT", rate=0.05)[:900 + 10 * k] + _rand(rng, 1500, b"ACGT")
        pairs.append((p, t[:1500]))
    bands = [(-30, 30)] * 64
    got, gc = _call(ctx, pairs, bands, table, go, ge, 60), _call(ctx, pairs, bands, table, go, ge, 60, cigar=True)
    rows = sum(g["rows"] for g in got)
    assert ctx.extend_banded_stats()["rows_considered"] == rows
    assert any(g["pend"] is None for g in got) and any(g["pend"] is not None for g in got)
    ks = list(range(0, 64, 9))
    assert [got[k] for k in ks] == XO.extend_many([pairs[k] for k in ks], [bands[k] for k in ks], table, go, ge, 60)
    with switched_context(PWA_RANGE_BYTES="4096") as c:
        assert _call(c, pairs, bands, table, go, ge, 60) == got
        assert c.extend_banded_stats()["rows_considered"] == rows
        assert _call(c, pairs, bands, table, go, ge, 60, cigar=True) == gc


def test_errors(pkg, ctx):
    """every refusal with its code, before any device work and in the documented order: the table's own checks, then xdrop, then per
    pair in pair order lo > hi, the anchor, the width, the 2^27 range rule; a failing call leaves every stats record as it was"""
    L, h = pkg.lib(), ctx._h
    A, Bq = b"ACGTACGTAC", b"ACGTTACGTACG"   # 10 x 12
    table, go, ge, _ = _table("dna")
    good = ctx.extend_banded_subst_batch([A, Bq], [0], [1], table, go, ge, [(-2, 4)], 10)
    assert good == XO.extend_many([(A, Bq)], [(-2, 4)], table, go, ge, 10)
    st = ctx.extend_banded_stats()
    assert st["rows_considered"] == good[0]["rows"] and st["fill_ms"] > 0 and st["walk_ms"] > 0
    blob, off, _ = pkg.pack_sequences([A, Bq])
    pa, pb = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 2)(1, 1)
    sc, nops, oo = (C.c_int32 * 2)(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)(0, 22)
    ops, cg, md = C.create_string_buffer(64), C.create_string_buffer(256), C.create_string_buffer(256)
    co, mo = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    ei, ej, rw, pj = [(C.c_uint32 * 2)() for _ in range(4)]
    ps = (C.c_int32 * 2)()
    code_ok = (C.c_uint8 * 256)(*[int(x) for x in table[0]])
    sub_ok = (C.c_int32 * 25)(*[int(x) for x in np.asarray(table[2]).ravel()])

    def raw(code=code_ok, n_sym=5, submat=sub_ok, go=-6, ge=-1, xdrop=10, lo=(-2, -2), hi=(4, 4), null_lo=False, null_hi=False, score=sc):
        """the three C calls on the two-pair list -> their return codes"""
        blo, bhi = None if null_lo else (C.c_int32 * 2)(*lo), None if null_hi else (C.c_int32 * 2)(*hi)
        head = (h, code, n_sym, submat, go, ge, xdrop, blob, off, 2, pa, pb, 2)
        return (L.pwa_extend_banded_subst_batch(*head, score, ops, oo, nops, None, rw, ps, pj, blo, bhi),
                L.pwa_extend_banded_subst_batch_cigar(*head, score, cg, 256, co, md, 256, mo, None, rw, ps, pj, None, blo, bhi),
                L.pwa_scores_extend_banded_subst(*head, score, ei, ej, rw, ps, pj, blo, bhi))

    inv, cap, ok = (INV,) * 3, (CAP,) * 3, (0, 0, 0)
    banded_before = (ctx.align_banded_stats(), ctx.scores_banded_stats(), ctx.align_subst_stats())
    assert raw() == ok
    st = ctx.extend_banded_stats()
    assert st["walk_ms"] == 0 and st["fill_ms"] > 0    # (the scores call ran last)
    # 1. the table's own checks, gap signs and null band arrays
    assert raw(code=None) == inv and raw(submat=None) == inv
    assert raw(n_sym=0) == inv and raw(n_sym=33) == inv
    bad_code = (C.c_uint8 * 256)(*[int(x) for x in table[0]])
    bad_code[200] = 5
    assert raw(code=bad_code) == inv
    assert raw(go=1) == inv and raw(ge=1) == inv
    assert raw(null_lo=True) == inv and raw(null_hi=True) == inv and raw(score=None) == inv
    # 2. xdrop
    assert raw(xdrop=(1 << 27) + 1) == inv and raw(xdrop=1 << 27) == ok and raw(xdrop=-5) == ok
    # 3. per pair: lo > hi, the anchor, the width, the range
    assert raw(lo=(1, 1), hi=(0, 0)) == inv
    assert raw(lo=(1, 1), hi=(3, 3)) == inv and raw(lo=(-3, -3), hi=(-1, -1)) == inv
    assert raw(lo=(-1, -1), hi=(MAX_WIDTH - 1, MAX_WIDTH - 1)) == cap
    assert raw(lo=(-1, -1), hi=(MAX_WIDTH - 2, MAX_WIDTH - 2)) == ok
    big = (C.c_int32 * 25)(*[int(x) for x in np.asarray(table[2]).ravel()])
    big[7] = -(1 << 23)                                    # 24 * 2^23 = 1.5 * 2^27: beyond EXT's rule, inside the banded rule's 2^28
    assert raw(submat=big) == cap
    big[7] = -((1 << 27) // 24 - 1)
    assert raw(submat=big) == ok
    # the order: a bad table before a bad xdrop before a bad band; the width before the range; the first offending pair decides
    assert raw(n_sym=33, xdrop=(1 << 27) + 1, lo=(-1, -1), hi=(MAX_WIDTH - 1, MAX_WIDTH - 1)) == inv
    assert raw(xdrop=(1 << 27) + 1, lo=(-1, -1), hi=(MAX_WIDTH - 1, MAX_WIDTH - 1)) == inv
    big[7] = -(1 << 23)
    assert raw(submat=big, lo=(1, 1), hi=(3, 3)) == inv
    assert raw(lo=(1, -1), hi=(MAX_WIDTH + 5, 1)) == inv    # pair 0: the anchor before the width
    assert raw(lo=(-1, 1), hi=(MAX_WIDTH - 1, 0)) == cap    # pair 0 too wide before pair 1's lo > hi
    assert raw(lo=(1, -1), hi=(0, MAX_WIDTH - 1)) == inv    # ... and the reverse
    assert raw(lo=(-1, 1), hi=(MAX_WIDTH - 1, 2)) == cap    # ... before pair 1's anchor
    # failing calls left the stats of the last valid one alone; the other families' records were never touched
    assert raw() == ok
    st = ctx.extend_banded_stats()
    assert raw(n_sym=0) == inv and raw(xdrop=(1 << 27) + 1) == inv and raw(lo=(1, 1), hi=(0, 0)) == inv and raw(submat=big) == cap
    assert ctx.extend_banded_stats() == st
    assert (ctx.align_banded_stats(), ctx.scores_banded_stats(), ctx.align_subst_stats()) == banded_before
    # a 100 x 100 pair with max |submat| = 2^20: (n + m + 2) A = 202 * 2^20 lies in [2^27, 2^28) -- refused here, taken by the NW score call
    p = _rand(random.Random(173), 100, b"ACGT")
    m20 = np.where(np.eye(4, dtype=bool), 1 << 20, -3)
    t20 = pkg.subst_table(b"ACGT", m20)
    assert (1 << 27) <= 202 * (1 << 20) < (1 << 28)
    for fn in (ctx.extend_banded_subst_batch, ctx.extend_banded_subst_batch_cigar, ctx.scores_extend_banded_subst):
        with pytest.raises(pkg.PwaError, match="2\\^27"):
            fn([p, p], [0], [1], t20, -2, -1, [(-5, 5)], 10)
    assert ctx.scores_banded_subst("nw", [p, p], [0], [1], t20, -2, -1, [(-5, 5)]) == [100 << 20]
    assert ctx.extend_banded_stats() == st
    with pytest.raises(pkg.PwaError, match="band_lo > band_hi"):
        ctx.extend_banded_subst_batch([A, Bq], [0], [1], table, go, ge, [(1, 0)], 10)
    with pytest.raises(pkg.PwaError, match="wider"):
        ctx.scores_extend_banded_subst([A, Bq], [0], [1], table, go, ge, [(-1, MAX_WIDTH - 1)], 10)
    with pytest.raises(pkg.PwaError, match="xdrop"):
        ctx.extend_banded_subst_batch_cigar([A, Bq], [0], [1], table, go, ge, [(-2, 4)], (1 << 27) + 1)
