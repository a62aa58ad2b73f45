"""Affine-gap (gotoh) batch alignments on the device (pwa_align_gotoh_batch / _cigar, include/pwalign.h): scores, end and start
cells and op lists byte for byte against the numpy oracle gotoh_oracle.py (tied to a scalar three-matrix DP and to the linear
oracles by test_gotoh_oracle.py); at gap_open = 0 against the linear engine itself."""
import ctypes as C
import random

import pytest

import gotoh_oracle as GO
from conftest import switched_context
from test_gpu_cigar import fmt

pytestmark = pytest.mark.gpu

PAT_LENS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 150, 255, 256, 257, 512, 1023, 1024]
TEXT_LENS = [0, 1, 2, 16, 17, 150, 257, 1025, 2049]
LONG_TEXT = 10000
SCORINGS = [(1, -4, -6, -1), (2, -3, -5, -2), (5, -4, -16, -4), (1, -1, -1, -1), (0, 0, 0, 0)]
ALPHABETS = {"dna": b"ACGT", "bytes": bytes(range(12)) + b"-"}   # 13 raw bytes with NUL and '-'
CASES = [(a, sc, a == "dna" and k == 0 or a == "bytes" and k == 0) for a in ALPHABETS
         for k, sc in enumerate(SCORINGS if a == "dna" else SCORINGS[:2])]


def _rand(rng, n, alpha):
    return bytes(rng.choice(alpha) for _ in range(n))


def _mutate(rng, s, alpha, rate=0.08):
    out = bytearray()
    for x in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out += _rand(rng, rng.randint(1, 4), alpha)
        out.append(rng.choice(alpha) if rate / 3 * 2 <= r < rate else x)
    return bytes(out)


def _shape_set(seed, alpha, long_text):
    """every pattern length against every text length: text t_n (one per pattern, its prefixes are the shorter texts) holds a
    mutated copy of the pattern near its start, so the alignments carry matches, mismatches and gaps of several lengths"""
    rng = random.Random(seed)
    tl = TEXT_LENS + ([LONG_TEXT] if long_text else [])
    pats, texts = [], []
    for n in PAT_LENS:
        t = bytearray(_rand(rng, max(tl), alpha))
        p = _rand(rng, n, alpha)
        core = _mutate(rng, p, alpha)
        off = rng.randint(0, 40)
        t[off:off + len(core)] = core
        pats.append(p)
        texts.append(bytes(t[:max(tl)]))
    return pats, texts, tl


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
@pytest.mark.parametrize("alpha,sc,long_text", CASES)
def test_shapes_against_oracle(ctx, mode, alpha, sc, long_text):
    match, mismatch, go, ge = sc
    pats, texts, tl = _shape_set(hash((alpha, sc)) & 0xffff, ALPHABETS[alpha], long_text)
    seqs = pats + [t[:m] for t in texts for m in tl]
    pa, pb = [], []
    for x in range(len(pats)):
        for y, m in enumerate(tl):
            pa.append(x)
            pb.append(len(pats) + x * len(tl) + y)
    got = ctx.align_gotoh_batch(mode, seqs, pa, pb, match, mismatch, go, ge)
    gc = ctx.align_gotoh_batch_cigar(mode, seqs, pa, pb, match, mismatch, go, ge)
    k = 0
    for x, p in enumerate(pats):
        want = GO.prefixes(p, texts[x], tl, mode, (match, mismatch), go, ge)
        for y, m in enumerate(tl):
            g, w, c = got[k], want[y], gc[k]
            t = texts[x][:m]
            key = (mode, len(p), m)
            assert (g["score"], g["end"], g["start"]) == (w["score"], w["end"], w["start"]), key
            assert g["ops"] == w["ops"], key
            assert (c["score"], c["end"], c["start"]) == (w["score"], w["end"], w["start"]), key
            assert (c["cigar"], c["mdz"]) == fmt(p, t, w["ops"], w["start"]), key
            k += 1


def _read_batch(seed, n_pairs, n, m):
    rng = random.Random(seed)
    refs = [_rand(rng, m, b"ACGT") for _ in range(64)]
    seqs, pa, pb = list(refs), [], []
    for k in range(n_pairs):
        r = refs[k % len(refs)]
        off = rng.randint(0, m - n)
        seqs.append(_mutate(rng, r[off:off + n], b"ACGT")[:n])
        pa.append(len(seqs) - 1)
        pb.append(k % len(refs))
    return seqs, pa, pb


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
def test_gap_open_zero_is_the_linear_engine(ctx, mode):
    """gap_open = 0: ops, cells and strings equal pwa_align_batch / _cigar with gap = gap_extend (4096 pairs 150 x 2000)"""
    seqs, pa, pb = _read_batch(17, 4096, 150, 2000)
    match, mismatch, gap = 2, -3, -2
    lin = ctx.align_batch(mode, seqs, pa, pb, match, mismatch, gap)
    got = ctx.align_gotoh_batch(mode, seqs, pa, pb, match, mismatch, 0, gap)
    assert got == lin
    assert ctx.align_gotoh_batch_cigar(mode, seqs, pa, pb, match, mismatch, 0, gap) == ctx.align_batch_cigar(mode, seqs, pa, pb, match, mismatch, gap)


def _mixed_batch(seed, n_pairs):
    rng = random.Random(seed)
    seqs, pa, pb = [], [], []
    for k in range(n_pairs):
        n = rng.choice([rng.randint(1, 300), rng.randint(1, 60), rng.randint(257, 600)] if k % 16 else [0, rng.randint(0, 5)])
        m = rng.randint(0, 700)
        t = _rand(rng, m, b"ACGT")
        p = _mutate(rng, t[:n], b"ACGT")[:n] if n <= m and rng.random() < 0.7 else _rand(rng, n, b"ACGT")
        seqs += [p, t]
        pa.append(2 * k)
        pb.append(2 * k + 1)
    return seqs, pa, pb


@pytest.mark.parametrize("mode", ["nw", "sw", "sg"])
def test_large_mixed_batch(ctx, mode):
    """8192 pairs of mixed lengths: every op list's affine score is its score_out, a sample against the oracle, and the same output
    when PWA_RANGE_BYTES cuts the list into several ranges"""
    match, mismatch, go, ge = 2, -3, -5, -2
    seqs, pa, pb = _mixed_batch(23, 8192)
    got = ctx.align_gotoh_batch(mode, seqs, pa, pb, match, mismatch, go, ge)
    for k, g in enumerate(got):
        p, t = seqs[pa[k]], seqs[pb[k]]
        assert GO.op_score(p, t, g["ops"], g["start"], (match, mismatch), go, ge) == g["score"], k
    for k in range(0, 8192, 61):
        w = GO.align(seqs[pa[k]], seqs[pb[k]], mode, (match, mismatch), go, ge)
        assert got[k] == w, k
    with switched_context(PWA_RANGE_BYTES="3145728") as c:
        assert c.align_gotoh_batch(mode, seqs, pa, pb, match, mismatch, go, ge) == got
        assert c.align_gotoh_batch_cigar(mode, seqs, pa, pb, match, mismatch, go, ge) == ctx.align_gotoh_batch_cigar(
            mode, seqs, pa, pb, match, mismatch, go, ge)
    st = ctx.align_gotoh_stats()
    assert st["fill_ms"] > 0 and st["walk_ms"] > 0 and st["band_bytes"] > 0


def test_planted_indels_are_one_gap(ctx):
    """SG reads of 150 with one planted 5..30-base deletion or insertion: the CIGAR holds it as one run of that length"""
    rng = random.Random(31)
    match, mismatch, go, ge = 1, -4, -6, -1
    seqs, pa, pb, plan = [], [], [], []
    for k in range(256):
        region = _rand(rng, 10000, b"ACGT")
        L, x, a = rng.randint(5, 30), rng.randint(40, 110), rng.randint(100, 9000)
        if k % 2 == 0:   # text bases missing from the read: an 'I' run (text-only columns)
            read = region[a:a + x] + region[a + x + L:a + 150 + L]
            want_score, tok = 150 * match + go + L * ge, b"%dI" % L
        else:            # read bases missing from the text: a 'D' run
            read = region[a:a + x] + _rand(rng, L, b"ACGT") + region[a + x:a + 150 - L]
            want_score, tok = (150 - L) * match + go + L * ge, b"%dD" % L
        seqs += [read, region]
        pa.append(2 * k)
        pb.append(2 * k + 1)
        plan.append((want_score, tok))
    got = ctx.align_gotoh_batch_cigar("sg", seqs, pa, pb, match, mismatch, go, ge)
    for g, (want_score, tok) in zip(got, plan):
        assert g["score"] >= want_score
        cig = g["cigar"]
        assert tok in cig, (cig, tok)
        assert cig.count(b"I") + cig.count(b"D") == 1, cig


def test_errors(pkg, ctx):
    seqs = [b"ACGT", b"ACGTT"]
    L = pkg.lib()
    for bad in [dict(go=1, ge=-1), dict(go=-1, ge=1)]:
        with pytest.raises(pkg.PwaError, match="INVALID|invalid|gap"):
            ctx.align_gotoh_batch("nw", seqs, [0], [1], 1, -1, bad["go"], bad["ge"])
    blob, off, _ = pkg.pack_sequences(seqs)
    pa, pb = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1)
    sc, nops, oo = (C.c_int32 * 1)(), (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    ops = C.create_string_buffer(16)
    h = ctx._h
    assert L.pwa_align_gotoh_batch(h, 3, 1, -1, -2, -1, blob, off, 2, pa, pb, 1, sc, ops, oo, nops, None, None) == -1   # unknown mode
    assert L.pwa_align_gotoh_batch(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 1, None, ops, oo, nops, None, None) == -1  # null scores
    assert L.pwa_align_gotoh_batch(h, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 1, sc, None, oo, nops, None, None) == -1   # null ops
    assert L.pwa_align_gotoh_batch(h, 0, 1, -1, -2, -1, blob, None, 2, pa, pb, 1, sc, ops, oo, nops, None, None) == -1   # null offsets
    assert L.pwa_align_gotoh_batch(None, 0, 1, -1, -2, -1, blob, off, 2, pa, pb, 1, sc, ops, oo, nops, None, None) == -1
    bad_b = (C.c_uint32 * 1)(2)
    assert L.pwa_align_gotoh_batch(h, 0, 1, -1, -2, -1, blob, off, 2, pa, bad_b, 1, sc, ops, oo, nops, None, None) == -1  # index
    with pytest.raises(pkg.PwaError, match="1024"):
        ctx.align_gotoh_batch("sg", [b"A" * 1025, b"ACGT"], [0], [1], 1, -1, -2, -1)
    with pytest.raises(pkg.PwaError, match="range"):
        ctx.align_gotoh_batch("nw", [b"A" * 10, b"A" * 10], [0], [1], 1 << 24, -1, -2, -1)
    assert ctx.align_gotoh_batch("nw", [b"A" * 10, b"A" * 10], [0], [1], (1 << 23) - 1, -1, -2, -1)[0]["score"] == 10 * ((1 << 23) - 1)
    assert ctx.align_gotoh_batch("nw", seqs, [], [], 1, -1, -2, -1) == []
    assert ctx.align_gotoh_batch_cigar("sw", seqs, [], [], 1, -1, -2, -1) == []
