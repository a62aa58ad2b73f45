"""Semi-global alignment (PWA_MODE_SG, include/pwalign.h): scores, end cells, alignments, CIGAR / MD:Z and matrices on the device,
every value compared exactly with the numpy oracle sg_oracle.py (tied to hw2.cpp's NW oracle by test_sg_oracle.py).

The same inputs run on every class the library can pick -- the mini-stripe fills (16 and 64 lanes per pair), the stripe engine with
and without table scoring, the plain int32 forms -- through the switches pwalign.h documents (conftest.switched_context)."""
import ctypes as C
import random

import numpy as np
import pytest

import sg_oracle as SG
from conftest import switched_context
from test_gpu_cigar import SCORINGS, fmt

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 150, 255, 256, 257, 1023, 1024, 1025, 2049]
TEXT_LENS = [0, 1, 2, 16, 17, 150, 257, 1025, 2049]
ALPHABETS = {"dna": b"ACGT", "bytes": bytes(range(12)) + b"-"}   # "bytes": 13 symbols with NUL and '-' -- the uncoded paths
BYTE_SCORINGS = [(1, -1, -1), (0, 0, 0), (-1, 2, 1)]
ENVS = {
    "default": {},
    "stripes": {"PWA_TB_ENGINE": "0"},                          # no mini-stripe classes
    "wide": {"PWA_TB_ENGINE": "2"},                             # 257 .. 1024 rows one pair per wave
    "plain": {"PWA_NO_KEYED_TB": "1"},                          # plain int32 fills
    "rl2": {"PWA_FORCE_RL": "2"},
    "rl4w1": {"PWA_FORCE_RL": "4", "PWA_FORCE_W": "1"},
    "no_shift": {"PWA_NO_GAP_SHIFT": "1"},
    "strip_route": {"PWA_SCORES_ROUTE": "0"},                   # asks for the strips: SG falls back to its own route
}
CASES = [(a, sc) for a in ALPHABETS for sc in (SCORINGS if a == "dna" else BYTE_SCORINGS)]


def _mutate(rng, s, alpha, rate):
    out = bytearray()
    for x in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice(alpha))
        out.append(rng.choice(alpha) if r < rate else x)
    return bytes(out)


_DATA = {}


def data(alpha_name):
    """one text of 2049 symbols and a pattern of every length in LENS (half cut from the text with edits): pairs (pattern n,
    text[:m]) for m in TEXT_LENS"""
    if alpha_name not in _DATA:
        rng = random.Random(7 + len(alpha_name))
        alpha = ALPHABETS[alpha_name]
        t = bytes(rng.choice(alpha) for _ in range(max(LENS)))
        pats = []
        for k, n in enumerate(LENS):
            if k % 2 and n:
                a = rng.randint(0, len(t) - n)
                p = _mutate(rng, t[a:a + n], alpha, 0.1)[:n]
                p += bytes(rng.choice(alpha) for _ in range(n - len(p)))
            else:
                p = bytes(rng.choice(alpha) for _ in range(n))
            pats.append(p)
        seqs = pats + [t[:m] for m in TEXT_LENS]
        pa = [i for i in range(len(LENS)) for _ in TEXT_LENS]
        pb = [len(LENS) + j for _ in LENS for j in range(len(TEXT_LENS))]
        _DATA[alpha_name] = (pats, t, seqs, pa, pb)
    return _DATA[alpha_name]


_WANT = {}


def want(alpha_name, sc):
    """oracle results in pair order"""
    key = (alpha_name, sc)
    if key not in _WANT:
        pats, t, _, _, _ = data(alpha_name)
        out = []
        for p in pats:
            out += SG.prefixes(p, t, TEXT_LENS, *sc)
        _WANT[key] = out
    return _WANT[key]


@pytest.fixture(scope="module", params=list(ENVS))
def sgctx(request):
    with switched_context(**ENVS[request.param]) as c:
        c.env_name = request.param
        yield c


@pytest.fixture(scope="module", params=[e for e in ENVS if e != "strip_route"])   # (a scores-route switch)
def alctx(request):
    with switched_context(**ENVS[request.param]) as c:
        c.env_name = request.param
        yield c


@pytest.mark.parametrize("case", CASES, ids=["%s-%d,%d,%d" % ((a,) + sc) for a, sc in CASES])
def test_scores_and_end_cells(sgctx, case):
    alpha, sc = case
    _, _, seqs, pa, pb = data(alpha)
    w = want(alpha, sc)
    ws = [r["score"] for r in w]
    s, ei, ej = sgctx.scores("sg", seqs, pa, pb, *sc, want_end=True)
    assert s == ws, sgctx.env_name
    assert list(zip(ei, ej)) == [r["end"] for r in w], sgctx.env_name
    assert sgctx.scores("sg", seqs, pa, pb, *sc) == ws, sgctx.env_name   # without end cells: the same route
    b = sgctx.batch("sg", seqs, pa, pb, *sc, want_end=True)
    try:
        for _ in range(2):   # a batch runs again with the same results
            b.run()
            s2, ei2, ej2 = b.fetch()
            assert (s2, ei2, ej2) == (ws, [r["end"][0] for r in w], [r["end"][1] for r in w]), sgctx.env_name
        assert "SG" in b.info()["kernel"] and b.cell_bits() == 0
    finally:
        b.close()


def test_batch_device_scores(ctx):
    import torch
    _, _, seqs, pa, pb = data("dna")
    ws = [r["score"] for r in want("dna", (2, -3, -5))]
    b = ctx.batch("sg", seqs, pa, pb, 2, -3, -5)
    try:
        b.run()
        assert b.fetch() == ws
        d = torch.full((len(pa),), -7, dtype=torch.int32, device="cuda")
        b.set_d_scores(d.data_ptr())
        b.run()
        assert b.fetch() == ws
        torch.cuda.synchronize()
        assert d.cpu().tolist() == ws
    finally:
        b.close()


@pytest.mark.parametrize("case", CASES, ids=["%s-%d,%d,%d" % ((a,) + sc) for a, sc in CASES])
def test_alignments(alctx, case):
    sgctx = alctx
    alpha, sc = case
    pats, t, seqs, pa, pb = data(alpha)
    w = want(alpha, sc)
    got = sgctx.align_batch("sg", seqs, pa, pb, *sc)
    for k, (g, r) in enumerate(zip(got, w)):
        assert (g["score"], g["end"], g["start"], g["ops"]) == (r["score"], r["end"], r["start"], r["ops"]), (sgctx.env_name, k)
    got = sgctx.align_batch_cigar("sg", seqs, pa, pb, *sc)
    for k, (g, r) in enumerate(zip(got, w)):
        p, tt = seqs[pa[k]], seqs[pb[k]]
        assert (g["score"], g["end"], g["start"]) == (r["score"], r["end"], r["start"]), (sgctx.env_name, k)
        assert (g["cigar"], g["mdz"]) == fmt(p, tt, r["ops"], r["start"]), (sgctx.env_name, k)
    for k in (0, 9 * 9 + 5, 9 * 10 + 8, len(pa) - 1):   # the single-pair entry point
        g = sgctx.align("sg", seqs[pa[k]], seqs[pb[k]], *sc, raw=True)
        assert (g["score"], g["end"], g["start"], g["ops"]) == (w[k]["score"], w[k]["end"], w[k]["start"], w[k]["ops"])


@pytest.mark.parametrize("env", ["default", "stripes", "plain"])
def test_matrices(env):
    rng = random.Random(3)
    with switched_context(**ENVS[env]) as c:
        for alpha in ALPHABETS.values():
            for sc in [(1, -1, -1), (0, 0, 0), (-1, 2, 1), (2, -3, -5), (1, 1, 1)]:
                for n, m in [(1, 1), (5, 9), (17, 40), (64, 33), (150, 200)]:
                    p = bytes(rng.choice(alpha) for _ in range(n))
                    t = bytes(rng.choice(alpha) for _ in range(m))
                    dp, tb = c.matrices("sg", p, t, *sc)
                    r = SG.align(p, t, *sc, mats=True)
                    assert np.array_equal(dp, r["dp"]), (env, sc, n, m)
                    assert np.array_equal(tb, r["tb"]), (env, sc, n, m)


def test_keyed_guard_both_sides(ctx):
    """(20000, -15000, -9000): keys in range up to n + m ~ 13 400 -- a call whose longest pair is shorter runs the keyed fills, one
    with a longer pair the plain int32 form (and both without table scoring: the key constants leave a byte)"""
    sc = (20000, -15000, -9000)
    rng = random.Random(9)
    t = bytes(rng.choice(b"ACGT") for _ in range(11000))
    small = [(_mutate(rng, t[a:a + n], b"ACGT", 0.05), t[:m]) for a, n, m in [(10, 100, 400), (300, 250, 2000), (50, 700, 3000)]]
    big = small + [(_mutate(rng, t[4000:7000], b"ACGT", 0.05), t)]
    for pairs in (small, big):
        seqs = [x for pt in pairs for x in pt]
        pa, pb = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
        w = [SG.align(p, tt, *sc) for p, tt in pairs]
        got = ctx.align_batch("sg", seqs, pa, pb, *sc)
        assert [(g["score"], g["end"], g["start"], g["ops"]) for g in got] == [(r["score"], r["end"], r["start"], r["ops"]) for r in w]
        s, ei, ej = ctx.scores("sg", seqs, pa, pb, *sc, want_end=True)
        assert (s, list(zip(ei, ej))) == ([r["score"] for r in w], [r["end"] for r in w])


def test_planted_reads(ctx):
    """512 reads of 150 cut from their 10k texts with a few edits: the alignment brackets the planted window, every pair exactly
    as the oracle"""
    rng = random.Random(2026)
    sc = (2, -3, -5)
    pairs, wins = [], []
    for _ in range(512):
        t = bytes(rng.choice(b"ACGT") for _ in range(10000))
        a = rng.randint(0, 10000 - 150)
        r = bytearray(t[a:a + 150])
        for _ in range(3):   # substitutions and one-symbol indels away from the ends
            x = rng.randint(10, 139)
            kind = rng.randint(0, 2)
            if kind == 0:
                r[x] = rng.choice(b"ACGT".replace(bytes([r[x]]), b""))
            elif kind == 1:
                del r[x]
                r.append(t[a + 150] if a + 150 < 10000 else 65)
            else:
                r.insert(x, rng.choice(b"ACGT"))
                del r[-1]
        pairs.append((bytes(r[:150]), t))
        wins.append((a, a + 150))
    seqs = [x for pt in pairs for x in pt]
    pa, pb = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
    w = SG.align_many(pairs, *sc)
    got = ctx.align_batch_cigar("sg", seqs, pa, pb, *sc)
    for k, (g, r) in enumerate(zip(got, w)):
        assert (g["score"], g["end"], g["start"]) == (r["score"], r["end"], r["start"]), k
        assert (g["cigar"], g["mdz"]) == fmt(*pairs[k], r["ops"], r["start"]), k
        assert abs(g["start"][1] - wins[k][0]) <= 4 and abs(g["end"][1] - wins[k][1]) <= 4, (k, g["start"], g["end"], wins[k])
    got = ctx.align_batch("sg", seqs, pa, pb, *sc)
    assert [g["ops"] for g in got] == [r["ops"] for r in w]


def test_long_pairs(ctx):
    """10k x 10k and 20k x 5k pairs on the stripe engine: score and end of all, the op list of one"""
    rng = random.Random(77)
    sc = (1, -1, -1)
    t1 = bytes(rng.choice(b"ACGT") for _ in range(10000))
    t3 = bytes(rng.choice(b"ACGT") for _ in range(5000))
    pairs = [(_mutate(rng, t1, b"ACGT", 0.1)[:10000], t1), (bytes(rng.choice(b"ACGT") for _ in range(10000)), t1),
             (_mutate(rng, t3, b"ACGT", 0.05) + bytes(rng.choice(b"ACGT") for _ in range(15000)), t3)]
    seqs = [x for pt in pairs for x in pt]
    pa, pb = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
    w = [SG.align(p, t, *sc, want_ops=(k == 0)) for k, (p, t) in enumerate(pairs)]
    s, ei, ej = ctx.scores("sg", seqs, pa, pb, *sc, want_end=True)
    assert (s, list(zip(ei, ej))) == ([r["score"] for r in w], [r["end"] for r in w])
    g = ctx.align("sg", *pairs[0], *sc, raw=True)
    assert (g["score"], g["end"], g["start"], g["ops"]) == (w[0]["score"], w[0]["end"], w[0]["start"], w[0]["ops"])


def test_errors(ctx, pkg):
    seqs = [b"ACGT", b"ACGTT"]
    with pytest.raises(pkg.PwaError, match="invalid"):
        ctx.overlaps("sg", seqs, [0], [1], 1, -1, -1)
    L, h = ctx._L, ctx._h
    score, n_ops = C.c_int32(0), C.c_uint64(0)
    ops = C.create_string_buffer(16)
    assert L.pwa_align(h, 3, 1, -1, -1, b"ACGT", 4, b"ACGTT", 5, C.byref(score), ops, 9, C.byref(n_ops), None, None) == -1
    dp = np.zeros((5, 6), dtype=np.int32)
    assert L.pwa_align_matrices(h, 3, 1, -1, -1, b"ACGT", 4, b"ACGTT", 5, dp.ctypes.data_as(C.c_void_p), None) == -1
    assert ctx.align("sg", b"ACGT", b"TTACGTT", 1, -1, -1)["score"] == 4   # the context is usable afterwards


@pytest.mark.parametrize("engine,n_class", [("stripes", (1, 63, 64)), ("stripes", (65, 127, 128)), ("stripes", (129, 200, 256)),
                                            ("stripes", (257, 300, 511, 512, 513)), ("stripes", (700, 1025, 1100, 1537)),
                                            ("mini", (1, 15, 16, 17, 63, 64)), ("mini", (65, 95, 96, 97, 127, 128)),
                                            ("mini", (129, 150, 159, 160, 161)), ("mini", (191, 192, 193, 255, 256, 257)),
                                            ("wide", (257, 300, 384, 385, 511, 512, 513)), ("wide", (700, 768, 769, 1023, 1024, 1025))])
def test_sg_shapes_around_every_boundary(engine, n_class):
    """test_gpu_parity.py's boundary grid in semi-global mode: pattern lengths around every stripe, mini-stripe (16 lanes x RL = 4 .. 16)
    and one-pair-per-wave (64 lanes x RL = 6, 8, 12, 16) class edge x text lengths around the 16-step chunks, the 15- and 63-step lane
    ramps and the 512-column LDS ring; table and compare scoring, with and without the score band: op lists, end and start cells and
    scores against sg_oracle (one fill per pattern, the texts are prefixes of one)."""
    rng = random.Random(sum(n_class) * 11 + len(n_class))
    ms = [0, 1, 2, 15, 16, 17, 31, 47, 48, 49, 62, 63, 64, 65, 79, 80, 81, 95, 127, 128, 129, 191, 255, 256, 257, 383, 384, 385, 511, 512,
          513, 520, 767, 768, 769, 1030]
    groups = []
    for n in n_class:
        p = bytes(rng.choice(b"ACGT") for _ in range(n))
        core = _mutate(rng, p, b"ACGT", 0.1)
        t = bytearray(rng.choice(b"ACGT") for _ in range(max(ms)))
        off = rng.randint(0, 60)
        t[off:off + len(core)] = core[:max(ms) - off]
        groups.append((p, bytes(t)))
    seqs, pa, pb = [], [], []
    for p, t in groups:
        for m in ms:
            seqs += [p, t[:m]]
            pa.append(len(seqs) - 2)
            pb.append(len(seqs) - 1)
    scorings = [(1, -1, -1), (2, -3, -5)]
    want = {sc: [w for p, t in groups for w in SG.prefixes(p, t, ms, *sc)] for sc in scorings}
    variants = [({}, False), ({"PWA_NO_PAIR_TABLE": "1"}, False), ({}, True)]
    for env, band in variants:
        if engine == "stripes":
            env = dict(env, PWA_TB_ENGINE="0")
        if engine == "wide":
            env = dict(env, PWA_TB_ENGINE="2")
        with switched_context(**env) as c:
            c.set_score_band(band)
            for sc in scorings:
                res = c.align_batch("sg", seqs, pa, pb, *sc)
                for k, (r, w) in enumerate(zip(res, want[sc])):
                    assert (r["score"], r["ops"], tuple(r["end"]), tuple(r["start"])) == \
                        (w["score"], w["ops"], tuple(w["end"]), tuple(w["start"])), (env, band, sc, len(seqs[pa[k]]), len(seqs[pb[k]]))
