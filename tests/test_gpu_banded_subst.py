"""Banded affine-gap alignments and scores under a substitution matrix on the device (pwa_align_banded_subst_batch / _cigar,
pwa_scores_banded_subst, include/pwalign.h): scores, end and start cells, op lists and strings byte for byte against the numpy oracle
banded_oracle.py under the table (tied to a scalar banded DP, to its byte compare and to gotoh_oracle by test_banded_subst_oracle.py); against the
byte-compare banded calls under a match / mismatch table; against the unbanded table calls under a band that covers the matrix; and the
error paths, all of which are host-side refusals.

Stripe heights as in test_gpu_banded.py: PWA_BANDED_RL=4|8 forces one, so that both run over the lengths around their own stripe
boundaries with every width.  The oracle results of a case list are computed once and shared by the three forms that are checked
against them."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import banded_oracle as BO
import gotoh_oracle as GO
from conftest import load_pkg, switched_context
from test_gpu_banded import DELTAS, HEIGHTS, MAX_WIDTH, WIDTHS, _band, _random_valid_band
from test_gpu_cigar import fmt
from test_gpu_gotoh import _mutate, _rand

pytestmark = pytest.mark.gpu

MODES = ["nw", "sw", "sg"]
PWA_E_INVALID, PWA_E_CAPACITY = -1, -5
RANGE_BYTES = 1 << 20   # test_range_cut_keeps_the_table's PWA_RANGE_BYTES
PROTEIN = b"ARNDCQEGHILKMFPSTWYVBZX*"   # 24 symbols; X (index 22) is the wildcard that unknown bytes map to


@functools.lru_cache(maxsize=None)
def _table(name):
    """-> (table, gap_open, gap_extend, the bytes the sequences are drawn from)"""
    pkg = load_pkg()
    if name == "protein":   # entries in [-4, 11], asymmetric, positive off-diagonal entries; J, O, U, '-' and NUL go to the wildcard
        m = np.random.RandomState(24).randint(-4, 12, size=(24, 24))
        assert (m != m.T).any() and (m[~np.eye(24, dtype=bool)] > 0).any()
        return pkg.subst_table(PROTEIN, m, unknown=22), -11, -1, PROTEIN[:20] * 3 + b"BZX*JOU-\0"
    if name == "dna":       # N neutral, lower case folded, transitions (A <-> G, C <-> T) apart from transversions
        m = np.full((5, 5), -4)
        m[[0, 2, 1, 3], [2, 0, 3, 1]] = -2
        m[np.arange(4), np.arange(4)] = 3
        m[4, :] = m[:, 4] = 0
        return pkg.subst_table(b"ACGTN", m, unknown=4, fold_case=True), -6, -1, b"ACGT" * 4 + b"acgtN"
    raise KeyError(name)


def _lengths(S):
    return [1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1, 3001]


def _text_for(rng, p, m, alpha):
    core = _mutate(rng, p, alpha, rate=0.05)
    return (core + _rand(rng, m, alpha))[:m]


@functools.lru_cache(maxsize=None)
def _shape_set(mode, S, name):
    """the case list of one (mode, stripe height, table) and its oracle results"""
    table, go, ge, alpha = _table(name)
    rng = random.Random(11 * S + len(name) + MODES.index(mode))
    pairs, bands = [], []
    for n in _lengths(S):
        widths = WIDTHS if n <= 2 * S + 1 else [7, 300]
        p = _rand(rng, n, alpha)
        for d in DELTAS:
            m = max(1, n + d)
            t = _text_for(rng, p, m, alpha)
            for w in widths:
                pairs.append((p, t))
                bands.append(_band(mode, n, m, w))
    return pairs, bands, BO.align_many(pairs, bands, mode, table, go, ge, group=24)


def _lists(pairs):
    seqs = [x for pt in pairs for x in pt]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


def _call(c, mode, pairs, bands, table, go, ge, cigar=False):
    seqs, pa, pb = _lists(pairs)
    fn = c.align_banded_subst_batch_cigar if cigar else c.align_banded_subst_batch
    return fn(mode, seqs, pa, pb, table, go, ge, bands)


def _scores(c, mode, pairs, bands, table, go, ge):
    seqs, pa, pb = _lists(pairs)
    s, ei, ej = c.scores_banded_subst(mode, seqs, pa, pb, table, go, ge, bands, want_end=True)
    return [(s[k], (ei[k], ej[k])) for k in range(len(pairs))]


def _check_all(c, mode, pairs, bands, table, go, ge, want, tag):
    """the three forms of one list against the oracle's results"""
    got, gc = _call(c, mode, pairs, bands, table, go, ge), _call(c, mode, pairs, bands, table, go, ge, cigar=True)
    gs = _scores(c, mode, pairs, bands, table, go, ge)
    assert len(got) == len(gc) == len(gs) == len(want)
    for k, (g, s, w) in enumerate(zip(got, gc, want)):
        p, t = pairs[k]
        key = (tag, k, len(p), len(t), bands[k])
        assert (g["score"], g["end"], g["start"]) == (w["score"], tuple(w["end"]), tuple(w["start"])), key
        assert g["ops"] == w["ops"], key
        assert (s["score"], s["end"], s["start"]) == (w["score"], tuple(w["end"]), tuple(w["start"])), key
        assert (s["cigar"], s["mdz"]) == fmt(p, t, w["ops"], w["start"]), key
        assert gs[k] == (w["score"], tuple(w["end"])), key


@pytest.fixture(scope="module", params=[4, 8])
def hctx(request):
    with switched_context(PWA_BANDED_RL=str(request.param)) as c:
        c.rl = request.param
        yield c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["protein", "dna"])
def test_shapes_against_oracle(hctx, mode, name):
    """n in {1, 2, 63, 64, 65, S - 1, S, S + 1, 2 S + 1, 3001} (patterns above 1024 among them), m = n + {-37, 0, 50}, half-widths
    {0, 1, 7, 64, 300} ({7, 300} at 3001), at both stripe heights, under a 24-symbol protein-like table with a wildcard and under a
    DNA table with a neutral N and folded lower case (MD:Z byte identity and score sign disagree there)"""
    table, go, ge, _ = _table(name)
    pairs, bands, want = _shape_set(mode, HEIGHTS[hctx.rl], name)
    assert any(len(p) > 1024 for p, _ in pairs)
    _check_all(hctx, mode, pairs, bands, table, go, ge, want, (mode, hctx.rl, name))


def _mixed_pairs(seed, count, nmax, mmax, alpha=b"ACGT"):
    rng = random.Random(seed)
    pairs = []
    for k in range(count):
        n = rng.choice([rng.randint(1, 60), rng.randint(1, 300), rng.randint(257, nmax)])
        m = rng.randint(1, mmax)
        t = _rand(rng, m, alpha)
        p = _mutate(rng, t[:n], alpha)[:n] if n <= m and rng.random() < 0.7 else _rand(rng, n, alpha)
        pairs.append((p, t))
    return pairs


@pytest.mark.parametrize("mode", MODES)
def test_match_mismatch_table_equals_the_byte_compare_calls(pkg, ctx, mode):
    """256 mixed DNA pairs, n <= 1500, random valid bands, match on the diagonal and mismatch off it: exactly the outputs of
    align_banded_batch, align_banded_batch_cigar and scores_banded"""
    match, mismatch, go, ge = 2, -3, -5, -2
    table = pkg.subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), match, mismatch))
    rng = random.Random(101)
    pairs = _mixed_pairs(103, 256, 1500, 1500)
    bands = [_random_valid_band(rng, mode, len(p), len(t)) for p, t in pairs]
    seqs, pa, pb = _lists(pairs)
    assert _call(ctx, mode, pairs, bands, table, go, ge) == ctx.align_banded_batch(mode, seqs, pa, pb, match, mismatch, go, ge, bands)
    assert _call(ctx, mode, pairs, bands, table, go, ge, cigar=True) == ctx.align_banded_batch_cigar(mode, seqs, pa, pb, match, mismatch, go, ge, bands)
    s, ei, ej = ctx.scores_banded(mode, seqs, pa, pb, match, mismatch, go, ge, bands, want_end=True)
    assert _scores(ctx, mode, pairs, bands, table, go, ge) == [(s[k], (ei[k], ej[k])) for k in range(len(pairs))]
    assert ctx.scores_banded_subst(mode, seqs, pa, pb, table, go, ge, bands) == s


@pytest.mark.parametrize("mode", MODES)
def test_full_cover_equals_the_unbanded_table_calls(ctx, mode):
    """128 mixed pairs, n <= 1024, band = the whole matrix: exactly align_subst_batch's, align_subst_batch_cigar's and
    scores_subst(want_end=True)'s outputs"""
    table, go, ge, alpha = _table("protein")
    pairs = _mixed_pairs(107, 128, 1024, 1200, alpha)
    bands = [(-len(p), len(t)) for p, t in pairs]
    seqs, pa, pb = _lists(pairs)
    assert _call(ctx, mode, pairs, bands, table, go, ge) == ctx.align_subst_batch(mode, seqs, pa, pb, table, go, ge)
    assert _call(ctx, mode, pairs, bands, table, go, ge, cigar=True) == ctx.align_subst_batch_cigar(mode, seqs, pa, pb, table, go, ge)
    s, ei, ej = ctx.scores_subst(mode, seqs, pa, pb, table, go, ge, want_end=True)
    assert _scores(ctx, mode, pairs, bands, table, go, ge) == [(s[k], (ei[k], ej[k])) for k in range(len(pairs))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_sym", [32, 1])
def test_alphabet_edges(pkg, hctx, mode, n_sym):
    """n_sym = 32: the full table at the even row stride; n_sym = 1: one entry"""
    alpha = bytes(range(65, 65 + n_sym))
    m = np.random.RandomState(n_sym).randint(-6, 9, size=(n_sym, n_sym))
    m[np.arange(n_sym), np.arange(n_sym)] = np.random.RandomState(n_sym + 1).randint(1, 9, size=n_sym)
    table = pkg.subst_table(alpha, m)
    rng = random.Random(109 + n_sym)
    S = HEIGHTS[hctx.rl]
    pairs, bands = [], []
    for n, d, w in [(S + 1, 0, 7), (70, 50, 64), (2 * S + 1, -37, 20), (5, 0, 1)]:
        p = _rand(rng, n, alpha)
        t = _text_for(rng, p, n + d, alpha)
        pairs.append((p, t))
        bands.append(_band(mode, n, n + d, w))
    want = BO.align_many(pairs, bands, mode, table, -3, -1)
    _check_all(hctx, mode, pairs, bands, table, -3, -1, want, (mode, hctx.rl, n_sym))


@functools.lru_cache(maxsize=None)
def _widest_set(mode):
    table, go, ge, alpha = _table("protein")
    rng = random.Random(113)
    p = _rand(rng, 700, alpha)
    t = _rand(rng, 1900, alpha) + _text_for(rng, p, 2700, alpha)   # 700 x 4600; the pattern's copy starts at column 1901
    band = (-100, MAX_WIDTH - 101)
    assert band[1] - band[0] + 1 == MAX_WIDTH and -700 <= band[0] and band[1] <= 4600 and band[0] <= 3900 <= band[1]
    pairs, bands = [(p, t)], [band]
    for n, d, w in [(300, 0, 3), (64, 50, 1), (513, -37, 10)]:
        q = _rand(rng, n, alpha)
        pairs.append((q, _text_for(rng, q, n + d, alpha)))
        bands.append(_band(mode, n, n + d, w))
    return pairs, bands, BO.align_many(pairs, bands, mode, table, go, ge, group=1)


@pytest.mark.parametrize("mode", MODES)
def test_widest_band_with_the_table_resident(hctx, mode):
    """one 700 x 4600 pair under a band of exactly MAX_WIDTH diagonals that the matrix does not clip, and three narrow pairs in the same
    launch: the hand-off rows at their largest (128 KiB of dynamic LDS per workgroup) beside the static table, and rows that are reused
    by a narrower pair"""
    table, go, ge, _ = _table("protein")
    pairs, bands, want = _widest_set(mode)
    _check_all(hctx, mode, pairs, bands, table, go, ge, want, ("widest", mode, hctx.rl))


@pytest.mark.parametrize("mode", MODES)
def test_ties(pkg, hctx, mode):
    """an all-zero table with zero gaps: everything ties; all-equal symbols with s = -gap_extend and gap_open = 0: diag, E and F tie all
    over the band and every opening ties its extension.  Tie-breaks and `a tie opens` bits as the oracle has them"""
    S = HEIGHTS[hctx.rl]
    rng = random.Random(127)
    pairs, bands = [], []
    for n, m, w in [(40, 40, 5), (S + 3, S + 20, 30), (17, 60, 50)]:
        pairs.append((b"A" * n, b"A" * m))
        bands.append(_band(mode, n, m, w))
    for n, m, w in [(33, 30, 8), (S + 1, S + 1, 2)]:
        pairs.append((_rand(rng, n, b"AC"), _rand(rng, m, b"AC")))
        bands.append(_band(mode, n, m, w))
    for m, go, ge in [([[0, 0], [0, 0]], 0, 0), ([[2, 2], [2, 2]], 0, -2), ([[1, -1], [-1, 1]], -2, 0)]:
        table = pkg.subst_table(b"AC", m)
        want = BO.align_many(pairs, bands, mode, table, go, ge)
        _check_all(hctx, mode, pairs, bands, table, go, ge, want, ("ties", mode, hctx.rl, go, ge))


@pytest.mark.parametrize("mode", MODES)
def test_range_cut_keeps_the_table(ctx, mode):
    """64 pairs of about 600 x 600 at half-width 30: two or three stripes of 256 rows each, about (256 + 61 + 78) x 256 bytes of band a
    stripe, some 15 MB in all.  With PWA_RANGE_BYTES = 1 MiB that is more than eight ranges, every one launched with the table uploaded
    once for the call -- the outputs of the uncut call.  The scores form is not cut and agrees."""
    table, go, ge, alpha = _table("dna")
    rng = random.Random(131)
    pairs, bands = [], []
    for k in range(64):
        n = rng.randint(500, 700)
        p = _rand(rng, n, alpha)
        m = n + rng.randint(-20, 20)
        pairs.append((p, _text_for(rng, p, m, alpha)))
        bands.append(_band(mode, n, m, 30))
    got, gc = _call(ctx, mode, pairs, bands, table, go, ge), _call(ctx, mode, pairs, bands, table, go, ge, cigar=True)
    st = ctx.align_banded_stats()
    assert st["fill_ms"] > 0 and st["walk_ms"] > 0 and st["band_bytes"] > 8 * RANGE_BYTES
    with switched_context(PWA_RANGE_BYTES=str(RANGE_BYTES)) as c:
        assert _call(c, mode, pairs, bands, table, go, ge) == got
        assert _call(c, mode, pairs, bands, table, go, ge, cigar=True) == gc
        assert c.align_banded_stats()["band_bytes"] == st["band_bytes"]
        assert _scores(c, mode, pairs, bands, table, go, ge) == [(g["score"], g["end"]) for g in got]
    want = BO.align_many(pairs[:8], bands[:8], mode, table, go, ge)
    for k, w in enumerate(want):
        assert got[k] == dict(score=w["score"], ops=w["ops"], end=tuple(w["end"]), start=tuple(w["start"])), k


@pytest.mark.parametrize("mode", MODES)
def test_empty_sides_and_the_empty_list(ctx, mode):
    table, go, ge, _ = _table("dna")
    assert ctx.align_banded_subst_batch(mode, [b"ACGT"], [], [], table, go, ge, []) == []
    assert ctx.align_banded_subst_batch_cigar(mode, [b"ACGT"], [], [], table, go, ge, []) == []
    assert ctx.scores_banded_subst(mode, [b"ACGT"], [], [], table, go, ge, [], want_end=True) == ([], [], [])
    pairs = [(b"ACG", b""), (b"", b"ACGTN"), (b"", b""), (b"ACGT", b"AGGT")]
    bands = [(-3, 0), (0, 5), (0, 0), (-1, 1)]
    want = BO.align_many(pairs, bands, mode, table, go, ge)
    for k in range(3):
        assert want[k] == GO.result(None, mode, len(pairs[k][0]), len(pairs[k][1]), go, ge)
    _check_all(ctx, mode, pairs, bands, table, go, ge, want, ("empty", mode))


def test_errors(pkg, ctx):
    """every refusal with its code, before any device work and -- for the per-pair ones -- in pair order; a failing call leaves the
    stats of the last valid call as they were, and pwa_align_subst_last_stats is never touched"""
    L, h = pkg.lib(), ctx._h
    A, Bq = b"ACGTACGTAC", b"ACGTTACGTACG"   # 10 x 12
    table, go, ge, _ = _table("dna")
    subst_before = ctx.align_subst_stats()
    assert ctx.align_banded_subst_batch("sw", [A, Bq], [0], [1], table, go, ge, [(3, 5)])[0]["score"] >= 0
    assert ctx.scores_banded_subst("sw", [A, Bq], [0], [1], table, go, ge, [(3, 5)])[0] >= 0
    st_a, st_s = ctx.align_banded_stats(), ctx.scores_banded_stats()
    assert st_a["band_bytes"] > 0 and st_s["in_band_cells"] == sum(min(10, 12 - d) for d in (3, 4, 5))
    blob, off, _ = pkg.pack_sequences([A, Bq])
    pa, pb = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 2)(1, 1)
    sc, nops, oo = (C.c_int32 * 2)(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)(0, 22)
    ops, cg, md = C.create_string_buffer(64), C.create_string_buffer(256), C.create_string_buffer(256)
    co, mo = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    ei, ej = (C.c_uint32 * 2)(), (C.c_uint32 * 2)()
    code_ok = (C.c_uint8 * 256)(*[int(x) for x in table[0]])
    sub_ok = (C.c_int32 * 25)(*[int(x) for x in np.asarray(table[2]).ravel()])

    def raw(mode=0, code=code_ok, n_sym=5, submat=sub_ok, go=-6, ge=-1, lo=(-2, -2), hi=(4, 4), null_lo=False):
        """the three C calls on the two-pair list -> their return codes"""
        blo, bhi = None if null_lo else (C.c_int32 * 2)(*lo), (C.c_int32 * 2)(*hi)
        head = (h, mode, code, n_sym, submat, go, ge, blob, off, 2, pa, pb, 2)
        return (L.pwa_align_banded_subst_batch(*head, sc, ops, oo, nops, None, None, blo, bhi),
                L.pwa_align_banded_subst_batch_cigar(*head, sc, cg, 256, co, md, 256, mo, None, None, None, blo, bhi),
                L.pwa_scores_banded_subst(*head, sc, ei, ej, blo, bhi))

    inv, cap = (PWA_E_INVALID,) * 3, (PWA_E_CAPACITY,) * 3
    assert raw() == (0, 0, 0)
    st_a, st_s = ctx.align_banded_stats(), ctx.scores_banded_stats()
    # the call's own checks
    assert raw(code=None) == inv and raw(submat=None) == inv
    assert raw(n_sym=0) == inv and raw(n_sym=33) == inv
    bad_code = (C.c_uint8 * 256)(*[int(x) for x in table[0]])
    bad_code[200] = 5
    assert raw(code=bad_code) == inv
    assert raw(go=1) == inv and raw(ge=1) == inv
    assert raw(null_lo=True) == inv
    # ... before the per-pair ones: a bad table and a bad band together report the table
    assert raw(n_sym=33, lo=(-1, -1), hi=(MAX_WIDTH - 1, MAX_WIDTH - 1)) == inv
    # per pair
    for mode in range(3):
        assert raw(mode=mode, lo=(1, 1), hi=(0, 0)) == inv                    # band_lo > band_hi
    assert raw(lo=(-1, -1), hi=(1, 1)) == inv                                 # NW: m - n = 2 outside
    assert raw(lo=(1, 1), hi=(3, 3)) == inv                                   # NW: diagonal 0 outside
    assert raw(mode=1, lo=(1, 1), hi=(3, 3)) == (0, 0, 0)                     # SW takes any band
    assert raw(lo=(-1, -1), hi=(MAX_WIDTH - 1, MAX_WIDTH - 1)) == cap         # width 4097
    assert raw(lo=(-1, -1), hi=(MAX_WIDTH - 2, MAX_WIDTH - 2)) == (0, 0, 0)   # width 4096
    big = (C.c_int32 * 25)(*[int(x) for x in np.asarray(table[2]).ravel()])
    big[7] = -(1 << 24)                                                       # 24 * 2^24 >= 2^28: the range rule, by |submat|
    assert raw(submat=big) == cap
    big[7] = -((1 << 28) // 24 - 1)
    assert raw(submat=big) == (0, 0, 0)
    # the first offending pair decides
    assert raw(lo=(-1, 1), hi=(MAX_WIDTH - 1, 0)) == cap
    assert raw(lo=(1, -1), hi=(0, MAX_WIDTH - 1)) == inv
    # the valid calls in between changed the stats; failing ones do not
    st_a, st_s = ctx.align_banded_stats(), ctx.scores_banded_stats()
    assert raw(n_sym=0) == inv and raw(lo=(1, 1), hi=(0, 0)) == inv and raw(lo=(-1, -1), hi=(MAX_WIDTH - 1, MAX_WIDTH - 1)) == cap
    assert ctx.align_banded_stats() == st_a and ctx.scores_banded_stats() == st_s
    assert ctx.align_subst_stats() == subst_before
    with pytest.raises(pkg.PwaError, match="band_lo > band_hi"):
        ctx.align_banded_subst_batch("nw", [A, Bq], [0], [1], table, go, ge, [(1, 0)])
    with pytest.raises(pkg.PwaError, match="wider"):
        ctx.scores_banded_subst("nw", [A, Bq], [0], [1], table, go, ge, [(-1, MAX_WIDTH - 1)])
    with pytest.raises(pkg.PwaError, match="submat"):
        ctx.align_banded_subst_batch_cigar("nw", [A, Bq], [0], [1], (table[0], 5, np.asarray(big) * 2), go, ge, [(-2, 4)])
