"""Banded affine-gap alignments on the device (pwa_align_banded_batch / _cigar, include/pwalign.h): scores, end and start cells and op
lists byte for byte against the numpy oracle banded_oracle.py (tied to a scalar banded DP and to gotoh_oracle by
test_banded_oracle.py), against the unbanded device calls where the band cannot matter, and the error paths.

Stripe heights: 256 rows for bands narrower than 1024 diagonals, 512 rows from there on; PWA_BANDED_RL=4|8 forces one of them, so
that every height is run over the lengths around its own stripe boundaries with every width."""
import ctypes as C
import random

import pytest

import banded_oracle as BO
import gotoh_oracle as GO
from conftest import load_pkg, switched_context
from test_gpu_cigar import fmt
from test_gpu_gotoh import _mutate, _rand

pytestmark = pytest.mark.gpu

HEIGHTS = {4: 256, 8: 512}
WIDTHS = [0, 1, 7, 64, 300]
DELTAS = [-37, 0, 50]
SCORINGS = [(1, -4, -6, -1), (1, -1, -1, -1)]
ALPHABETS = {"dna": b"ACGT", "bytes": bytes(range(12)) + b"-"}   # 13 raw bytes with NUL and '-'
MAX_WIDTH = 4096


def _lengths(S):
    return [1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3001]


def _text_for(rng, p, m, alpha):
    """m bytes that hold a mutated copy of p from the start (cut or padded to m)"""
    core = _mutate(rng, p, alpha, rate=0.05)
    return (core + _rand(rng, m, alpha))[:m]


def _band(mode, n, m, w):
    pkg = load_pkg()
    if mode == "nw":
        return pkg.band_around(n, m, w)
    lo, hi = pkg.band_around(n, m, w, diag=0 if m >= n else (m - n) // 2)
    if mode == "sg":   # (a diagonal band, widened just enough to be valid where the text is shorter than the pattern)
        lo, hi = min(lo, m - n), max(hi, 0)
    return lo, hi


def _shape_cases(mode, S, alpha, seed):
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
                bands.append(_band(mode, n, m, w))
    return pairs, bands


def _call(c, mode, pairs, bands, sc, cigar=False):
    seqs = [x for pt in pairs for x in pt]
    pa, pb = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
    fn = c.align_banded_batch_cigar if cigar else c.align_banded_batch
    return fn(mode, seqs, pa, pb, *sc, bands)


def _check(got, gc, want, pairs, bands, tag):
    for k, (g, c, w) in enumerate(zip(got, gc, want)):
        p, t = pairs[k]
        key = (tag, k, len(p), len(t), bands[k])
        assert (g["score"], g["end"], g["start"]) == (w["score"], w["end"], w["start"]), key
        assert g["ops"] == w["ops"], key
        assert (c["score"], c["end"], c["start"]) == (w["score"], w["end"], w["start"]), key
        assert (c["cigar"], c["mdz"]) == fmt(p, t, w["ops"], w["start"]), key


@pytest.fixture(scope="module", params=[4, 8])
def hctx(request):
    with switched_context(PWA_BANDED_RL=str(request.param)) as c:
        c.rl = request.param
        yield c


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("alpha,sc", [("dna", SCORINGS[0]), ("dna", SCORINGS[1]), ("bytes", SCORINGS[0])])
def test_shapes_against_oracle(hctx, mode, alpha, sc):
    pairs, bands = _shape_cases(mode, HEIGHTS[hctx.rl], ALPHABETS[alpha], 7 * hctx.rl + len(alpha))
    want = BO.align_many(pairs, bands, mode, sc[:2], *sc[2:], group=24)
    _check(_call(hctx, mode, pairs, bands, sc), _call(hctx, mode, pairs, bands, sc, cigar=True), want, pairs, bands, (mode, hctx.rl))


def _mixed_pairs(seed, count, nmax, mmax):
    rng = random.Random(seed)
    pairs = []
    for k in range(count):
        n = rng.choice([rng.randint(1, 60), rng.randint(1, 300), rng.randint(257, nmax)])
        m = rng.randint(1, mmax)
        t = _rand(rng, m, b"ACGT")
        p = _mutate(rng, t[:n], b"ACGT")[:n] if n <= m and rng.random() < 0.7 else _rand(rng, n, b"ACGT")
        pairs.append((p, t))
    return pairs


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
def test_full_cover_is_the_unbanded_call(ctx, mode):
    """512 mixed pairs, n <= 1024, band = the whole matrix: exactly align_gotoh_batch's and align_gotoh_batch_cigar's outputs"""
    sc = (2, -3, -5, -2)
    pairs = _mixed_pairs(41, 512, 1024, 1500)
    bands = [(-len(p), len(t)) for p, t in pairs]
    seqs = [x for pt in pairs for x in pt]
    pa, pb = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
    assert _call(ctx, mode, pairs, bands, sc) == ctx.align_gotoh_batch(mode, seqs, pa, pb, *sc)
    assert _call(ctx, mode, pairs, bands, sc, cigar=True) == ctx.align_gotoh_batch_cigar(mode, seqs, pa, pb, *sc)


@pytest.fixture(scope="module")
def path_cover_set():
    """256 pairs 1500 x 1500 and their unbanded oracle alignments, per mode (computed once)"""
    rng = random.Random(43)
    pairs = []
    for k in range(256):
        p = _rand(rng, 1500, b"ACGT")
        t = _text_for(rng, p, 1500, b"ACGT")
        pairs.append((p, t))
    sc = (1, -4, -6, -1)
    return pairs, sc, {mode: GO.align_many(pairs, mode, sc[:2], *sc[2:]) for mode in ("nw", "sw", "sg")}


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
def test_path_cover(ctx, path_cover_set, mode):
    pairs, sc, unb = path_cover_set
    want = unb[mode]
    tight = []
    for w in want:
        lo, hi = BO.walk_diagonals(w["ops"], w["start"])
        tight.append((min(lo, 0), max(hi, 0)) if mode == "nw" else (lo, max(hi, 0)) if mode == "sg" else (lo, hi))
    got = _call(ctx, mode, pairs, tight, sc)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == dict(score=w["score"], ops=w["ops"], end=w["end"], start=w["start"]), (mode, k, tight[k])
    ks = [k for k, (lo, hi) in enumerate(tight) if BO.band_valid(mode, 1500, 1500, lo + 3, hi - 3)]
    assert len(ks) >= 16   # (how many bands can lose 3 diagonals a side and stay valid is a property of the data alone)
    sp, sb = [pairs[k] for k in ks], [(tight[k][0] + 3, tight[k][1] - 3) for k in ks]
    got = _call(ctx, mode, sp, sb, sc)
    wantb = BO.align_many(sp, sb, mode, sc[:2], *sc[2:])
    for x, k in enumerate(ks):
        g, (p, t) = got[x], sp[x]
        assert g["score"] <= want[k]["score"], (mode, k)
        assert GO.op_score(p, t, g["ops"], g["start"], sc[:2], *sc[2:]) == g["score"], (mode, k)
        assert mode == "sw" and not g["ops"] or BO.ops_in_band(g["ops"], g["start"], sb[x]), (mode, k)
        assert g == wantb[x], (mode, k, sb[x])


def test_stripe_and_edge_stress(hctx):
    """planted 40-row deletions that straddle rows S and 2 S, and planted insertions that push the path onto band_hi, then band_lo:
    each run comes back as one CIGAR run, and everything equals the oracle"""
    S = HEIGHTS[hctx.rl]
    rng = random.Random(47)
    sc = (1, -4, -6, -1)
    pairs, bands, toks = [], [], []
    for at in (S - 20, 2 * S - 20, S - 39, 2 * S - 1):   # the 40 deleted pattern rows at + 1 .. at + 40
        core = _rand(rng, 2 * S + 300, b"ACGT")
        p = core[:at] + _rand(rng, 40, b"ACGT") + core[at:]
        pairs.append((p, core))
        bands.append((-50, 10))
        toks.append([b"40D"])
    for w in (25, 40):                                    # + w columns (path on band_hi = w), later - w rows ... back on diagonal 0 = band_lo
        core = _rand(rng, 2 * S + 300, b"ACGT")
        ins = _rand(rng, w, b"ACGT")
        t = core[:S - 10] + ins + core[S - 10:]
        p = core[:2 * S - 5] + _rand(rng, w, b"ACGT") + core[2 * S - 5:]
        pairs.append((p, t))
        bands.append((0, w))
        toks.append([b"%dI" % w, b"%dD" % w])
    want = BO.align_many(pairs, bands, "nw", sc[:2], *sc[2:])
    got, gc = _call(hctx, "nw", pairs, bands, sc), _call(hctx, "nw", pairs, bands, sc, cigar=True)
    _check(got, gc, want, pairs, bands, ("stress", hctx.rl))
    for c, tk in zip(gc, toks):
        for tok in tk:
            assert tok in c["cigar"], (c["cigar"], tok)
        assert c["cigar"].count(b"I") + c["cigar"].count(b"D") == len(tk), c["cigar"]


def test_widest_band(ctx):
    """one 2200 x 2150 NW pair under a band of exactly MAX_WIDTH diagonals that the matrix does not clip: the largest hand-off row
    (32 KiB of LDS per wave, 128 KiB per workgroup)"""
    rng = random.Random(67)
    p = _rand(rng, 2200, b"ACGT")
    t = _text_for(rng, p, 2150, b"ACGT")
    band = (-2100, MAX_WIDTH - 2101)
    assert band[1] - band[0] + 1 == MAX_WIDTH and -2200 <= band[0] and band[1] <= 2150
    sc = (1, -4, -6, -1)
    want = BO.align(p, t, band, "nw", sc[:2], *sc[2:])
    assert _call(ctx, "nw", [(p, t)], [band], sc)[0] == want
    assert _call(ctx, "sw", [(p, t)], [band], sc)[0] == BO.align(p, t, band, "sw", sc[:2], *sc[2:])


def test_long_pair(ctx, pkg):
    """one 20 000 x 20 000 NW pair, w = 100, ~3 % mutations with indels of up to 30"""
    rng = random.Random(53)
    p = _rand(rng, 20000, b"ACGT")
    out, skip = bytearray(), 0
    for x in p:
        r = rng.random()
        if skip:                       # inside a deletion
            skip -= 1
            continue
        if r < 0.0005:
            skip = rng.randint(1, 30)
        elif r < 0.001:
            out += _rand(rng, rng.randint(1, 30), b"ACGT")
        out.append(rng.choice(b"ACGT") if r > 0.97 else x)
    t = bytes(out[:20000]) + _rand(rng, max(0, 20000 - len(out)), b"ACGT")
    band = pkg.band_around(20000, 20000, 100)
    sc = (1, -4, -6, -1)
    got = _call(ctx, "nw", [(p, t)], [band], sc)[0]
    assert got == BO.align(p, t, band, "nw", sc[:2], *sc[2:])


def test_seeded_semiglobal_reads(ctx, pkg):
    """2048 reads of 1500 against 4000-column texts, band = the planted diagonal +- 60"""
    rng = random.Random(59)
    sc = (1, -4, -6, -1)
    texts = [_rand(rng, 4000, b"ACGT") for _ in range(32)]
    pairs, bands = [], []
    for k in range(2048):
        t = texts[k % 32]
        d = rng.randint(0, 2400)
        read = _mutate(rng, t[d:d + 1500], b"ACGT", rate=0.04)[:1500]
        pairs.append((read, t))
        bands.append(pkg.band_around(len(read), 4000, 60, diag=d))
    got = _call(ctx, "sg", pairs, bands, sc)
    for k, g in enumerate(got):
        assert GO.op_score(pairs[k][0], pairs[k][1], g["ops"], g["start"], sc[:2], *sc[2:]) == g["score"], k
    ks = list(range(0, 2048, 37))
    want = BO.align_many([pairs[k] for k in ks], [bands[k] for k in ks], "sg", sc[:2], *sc[2:])
    for x, k in enumerate(ks):
        assert got[k] == want[x], (k, bands[k])


def _random_valid_band(rng, mode, n, m):
    d = m - n
    k1, k2 = rng.choice([(0, 0), (rng.randint(0, 40), rng.randint(0, 40)), (rng.randint(0, 400), rng.randint(0, 400))])
    if mode == "nw":
        return (min(0, d) - k1, max(0, d) + k2)
    if mode == "sg":
        lo = rng.randint(-n - 1, d)
        return (lo, max(lo, 0) + k2)
    lo = rng.randint(-n - 2, m + 2)
    return (lo, lo + k2)


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
def test_mixed_batch(ctx, mode):
    """4096 pairs with lengths 0 .. 3000 and random valid bands: every op list's affine score is its score, a sample equals the
    oracle, empty sides follow the gotoh conventions, and PWA_RANGE_BYTES changes nothing"""
    rng = random.Random(61)
    sc = (2, -3, -5, -2)
    pairs, bands = [], []
    for k in range(4096):
        if k % 16 == 0:
            n, m = rng.choice([(0, 0), (0, rng.randint(1, 50)), (rng.randint(1, 50), 0)])
        else:
            n = rng.choice([rng.randint(1, 100), rng.randint(1, 700), rng.randint(1, 3000)])
            m = max(1, n + rng.randint(-60, 60)) if rng.random() < 0.8 else rng.randint(1, 3000)
        t = _rand(rng, m, b"ACGT")
        p = _mutate(rng, t, b"ACGT", rate=0.05)[:n] if rng.random() < 0.8 else b""
        p = p + _rand(rng, n - len(p), b"ACGT")
        pairs.append((p, t))
        bands.append(_random_valid_band(rng, mode, n, m))
    got = _call(ctx, mode, pairs, bands, sc)
    for k, g in enumerate(got):
        p, t = pairs[k]
        if not (len(p) and len(t)):
            assert g == GO.result(None, mode, len(p), len(t), sc[2], sc[3]), k
        assert GO.op_score(p, t, g["ops"], g["start"], sc[:2], *sc[2:]) == g["score"], (k, bands[k])
    ks = list(range(1, 4096, 29))
    want = BO.align_many([pairs[k] for k in ks], [bands[k] for k in ks], mode, sc[:2], *sc[2:], group=16)
    for x, k in enumerate(ks):
        assert got[k] == want[x], (k, len(pairs[k][0]), len(pairs[k][1]), bands[k])
    st = ctx.align_banded_stats()
    assert st["fill_ms"] > 0 and st["walk_ms"] > 0 and st["band_bytes"] > 0
    gc = _call(ctx, mode, pairs, bands, sc, cigar=True)
    with switched_context(PWA_RANGE_BYTES="3145728") as c:
        assert _call(c, mode, pairs, bands, sc) == got
        assert _call(c, mode, pairs, bands, sc, cigar=True) == gc


def test_errors(pkg, ctx):
    A, Bq = b"ACGTACGTAC", b"ACGTTACGTACG"   # 10 x 12
    def run(mode, band, sc=(1, -1, -2, -1), seqs=(A, Bq)):
        return ctx.align_banded_batch(mode, list(seqs), [0], [1], *sc, [band])
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
    assert run("sw", (3, 5))[0]["score"] >= 0
    with pytest.raises(pkg.PwaError, match="wider"):
        run("nw", (-1, MAX_WIDTH - 1))
    assert run("nw", (-1, MAX_WIDTH - 2))[0] == GO.align(A, Bq, "nw", (1, -1), -2, -1)
    with pytest.raises(pkg.PwaError, match="INVALID|invalid|gap"):
        run("nw", (-2, 4), sc=(1, -1, 1, -1))
    with pytest.raises(pkg.PwaError, match="range"):
        run("nw", (-2, 4), sc=(1 << 24, -1, -2, -1))
    # the first offending pair decides: pair 0 too wide (CAPACITY) before pair 1's lo > hi (INVALID), and the reverse
    L, h = pkg.lib(), ctx._h
    blob, off, _ = pkg.pack_sequences([A, Bq])
    pa, pb = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 2)(1, 1)
    sc, nops, oo = (C.c_int32 * 2)(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)(0, 22)
    ops = C.create_string_buffer(64)
    def raw(lo, hi, n=2):
        blo, bhi = (C.c_int32 * 2)(*lo), (C.c_int32 * 2)(*hi)
        return L.pwa_align_banded_batch(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, n, sc, ops, oo, nops, None, None, blo, bhi)
    assert raw((-1, 1), (MAX_WIDTH - 1, 0)) == -5   # PWA_E_CAPACITY
    assert raw((1, -1), (0, MAX_WIDTH - 1)) == -1   # PWA_E_INVALID
    assert L.pwa_align_banded_batch(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 2, sc, ops, oo, nops, None, None, None, (C.c_int32 * 2)(4, 4)) == -1   # null band_lo
    assert ctx.align_banded_batch("nw", [A, Bq], [], [], 1, -1, -2, -1, []) == []
    assert ctx.align_banded_batch_cigar("sw", [A, Bq], [], [], 1, -1, -2, -1, []) == []
    # a pair with an empty side follows the gotoh conventions, provided its band is valid
    assert run("nw", (-3, 0), seqs=(b"ACG", b""))[0] == GO.result(None, "nw", 3, 0, -2, -1)
    with pytest.raises(pkg.PwaError, match="NW"):
        run("nw", (0, 0), seqs=(b"ACG", b""))
