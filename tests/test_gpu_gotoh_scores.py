"""Affine-gap (gotoh) score passes on the device (pwa_gotoh_batch_create / pwa_scores_gotoh, include/pwalign.h): scores and end cells
against the numpy oracle gotoh_oracle.py (want_ops=False), against pwa_align_gotoh_batch and, at gap_open = 0, against the linear score
pass.  want_end=False runs NW and SW on the register-strip kernels (batch_gotoh.hip.h), want_end=True everything on the band-less gotoh
mini-stripe fills: the same pairs go through both engines."""
import ctypes as C
import random

import pytest

import gotoh_oracle as GO
from conftest import switched_context
from test_gpu_gotoh import ALPHABETS, CASES, _mixed_batch, _mutate, _rand, _shape_set

pytestmark = pytest.mark.gpu

MODES = ["nw", "sw", "sg"]
PWA_E_INVALID, PWA_E_CAPACITY = -1, -5
STRIP = "batch_gotoh_kernel"


def _want(pairs, mode, sc):
    w = GO.align_many(pairs, mode, sc[:2], *sc[2:], want_ops=False)
    return [x["score"] for x in w], [x["end"][0] for x in w], [x["end"][1] for x in w]


def _batch(pairs):
    seqs = [x for pr in pairs for x in pr]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("alpha,sc,long_text", CASES)
def test_shapes_against_oracle(ctx, mode, alpha, sc, long_text):
    """test_gpu_gotoh.py's pattern x text grid: scores without end cells (strips for NW / SW) and with them (band-less mini form)"""
    pats, texts, tl = _shape_set(hash((alpha, sc)) & 0xffff, ALPHABETS[alpha], long_text)
    seqs = pats + [t[:m] for t in texts for m in tl]
    pa, pb = [], []
    for x in range(len(pats)):
        for y, m in enumerate(tl):
            pa.append(x)
            pb.append(len(pats) + x * len(tl) + y)
    plain = ctx.scores_gotoh(mode, seqs, pa, pb, *sc)
    s, ei, ej = ctx.scores_gotoh(mode, seqs, pa, pb, *sc, want_end=True)
    k = 0
    for x, p in enumerate(pats):
        want = GO.prefixes(p, texts[x], tl, mode, sc[:2], *sc[2:], want_ops=False)
        for y, m in enumerate(tl):
            key = (mode, len(p), m)
            assert plain[k] == want[y]["score"], key
            assert (s[k], (ei[k], ej[k])) == (want[y]["score"], want[y]["end"]), key
            k += 1


# ------------------------------------------------------------------ 2. beyond 1024 rows
def _long_pairs():
    """nested patterns of 40 .. 8193 rows against mutated copies of their prefixes: every text takes several patterns, so a wave task's
    lanes end in different strips; one pair about 8193 x 8000 (the oracle's memory bound)"""
    rng = random.Random(2049)
    base = _rand(rng, 8193, b"ACGT")
    t300 = _mutate(rng, base[:300], b"ACGT")[:300]
    t2100 = (_mutate(rng, base[:2049], b"ACGT") + _rand(rng, 100, b"ACGT"))[:2100]
    t5000 = (_mutate(rng, base[:4097], b"ACGT") + _rand(rng, 1200, b"ACGT"))[:5000]
    t8000 = _mutate(rng, base, b"ACGT")[:8000]
    pairs = [(base[:n], t) for t in (t300, t2100) for n in (1025, 2049, 40, 1500, 4097, 1024, 1057)]
    pairs += [(base[:4097], t5000), (base[:1025], t5000), (base[:2049], t5000), (base, t8000), (base[:1025], t8000[:1100])]
    return pairs


@pytest.mark.parametrize("mode", ["nw", "sw"])
def test_patterns_beyond_1024_rows(ctx, mode):
    pairs = _long_pairs()
    seqs, pa, pb = _batch(pairs)
    for sc in [(1, -4, -6, -1), (2, -3, -5, -2)]:
        want = _want(pairs, mode, sc)[0]
        if mode == "sw":
            assert min(w for w, (p, t) in zip(want, pairs) if len(p) > 1024) > 200   # (the texts are copies: no trivially small scores)
        b = ctx.batch_gotoh(mode, seqs, pa, pb, *sc)
        try:
            assert STRIP in b.info()["kernel"] and b.cell_bits() == 32 and b.profile_form() == 0
            b.run()
            assert b.fetch() == want, (mode, sc)
        finally:
            b.close()


def test_1025_rows_off_the_strips_is_capacity(pkg, ctx):
    seqs = [b"ACGT" * 256 + b"A", b"ACGTTGCA" * 150]
    for mode, want_end in [("sg", False), ("sg", True), ("nw", True), ("sw", True)]:
        with pytest.raises(pkg.PwaError, match="1024"):
            ctx.scores_gotoh(mode, seqs, [0], [1], 1, -4, -6, -1, want_end=want_end)
    assert ctx.scores_gotoh("nw", seqs, [0], [1], 1, -4, -6, -1) == _want([(seqs[0], seqs[1])], "nw", (1, -4, -6, -1))[0]


# ------------------------------------------------------------------ 3. equal to the alignment call and to the linear pass
@pytest.mark.parametrize("mode", MODES)
def test_equal_to_the_alignment_call(ctx, mode):
    sc = (2, -3, -5, -2)
    seqs, pa, pb = _mixed_batch(29, 2048)
    al = ctx.align_gotoh_batch(mode, seqs, pa, pb, *sc)
    assert ctx.scores_gotoh(mode, seqs, pa, pb, *sc) == [a["score"] for a in al]
    s, ei, ej = ctx.scores_gotoh(mode, seqs, pa, pb, *sc, want_end=True)
    assert s == [a["score"] for a in al]
    assert list(zip(ei, ej)) == [tuple(a["end"]) for a in al]


@pytest.mark.parametrize("mode", MODES)
def test_gap_open_zero_is_the_linear_pass(ctx, mode):
    seqs, pa, pb = _mixed_batch(31, 2048)
    match, mismatch, gap = 2, -3, -2
    assert ctx.scores_gotoh(mode, seqs, pa, pb, match, mismatch, 0, gap) == ctx.scores(mode, seqs, pa, pb, match, mismatch, gap)
    assert ctx.scores_gotoh(mode, seqs, pa, pb, match, mismatch, 0, gap, want_end=True) == ctx.scores(mode, seqs, pa, pb, match, mismatch, gap,
                                                                                                  want_end=True)


# ------------------------------------------------------------------ 4. ties and first maxima
def _copies(rng, p, k, junk=(3, 30)):
    t = bytearray(_rand(rng, rng.randint(*junk), b"ACGT"))
    for _ in range(k):
        t += p + _rand(rng, rng.randint(*junk), b"ACGT")
    return bytes(t)


@pytest.mark.parametrize("n", [16, 40, 100, 200, 256, 600, 1024])
def test_sw_first_row_major_maximum(ctx, n):
    """equal maxima in several columns (repeated copies of the pattern) and in several rows (X + X against separate copies of X)"""
    rng = random.Random(n + 9)
    x = _rand(rng, n // 2, b"ACGT")
    p = _rand(rng, n, b"ACGT")
    pairs = [(p, _copies(rng, p, 4)), (p, p * 3), (x + x, _copies(rng, x, 3)), (x + _rand(rng, n - 2 * len(x), b"ACGT") + x, _copies(rng, x, 2)),
             (p, _copies(rng, p[: n // 2], 2) + _copies(rng, p[n // 2:], 2))]
    seqs, pa, pb = _batch(pairs)
    for sc in [(1, -4, -6, -1), (2, -3, -5, 0), (2, 1, -3, -1)]:
        want = _want(pairs, "sw", sc)
        assert tuple(ctx.scores_gotoh("sw", seqs, pa, pb, *sc, want_end=True)) == want, (n, sc)
        assert ctx.scores_gotoh("sw", seqs, pa, pb, *sc) == want[0], (n, sc)


@pytest.mark.parametrize("n", [40, 256, 1024])
def test_sg_smallest_end_column(ctx, n):
    rng = random.Random(n + 19)
    p = _rand(rng, n, b"ACGT")
    pairs = [(p, _copies(rng, p, 4)), (p, p * 3), (p, _rand(rng, 50, b"ACGT") + p + p[: n // 2] + p)]
    seqs, pa, pb = _batch(pairs)
    for sc in [(1, -4, -6, -1), (2, -3, -5, 0)]:
        assert tuple(ctx.scores_gotoh("sg", seqs, pa, pb, *sc, want_end=True)) == _want(pairs, "sg", sc), (n, sc)


# ------------------------------------------------------------------ 5. routing rule
def _info_and_scores(ctx, mode, seqs, pa, pb, sc):
    b = ctx.batch_gotoh(mode, seqs, pa, pb, *sc)
    try:
        b.run()
        return b.info()["kernel"], b.cell_bits(), b.fetch()
    finally:
        b.close()


def test_routing_rule(ctx):
    rng = random.Random(77)
    texts = [_rand(rng, 700, b"ACGT") for _ in range(4)]
    pats = [_mutate(rng, texts[k % 4][30:30 + n], b"ACGT")[:n] for k, n in enumerate([5, 60, 150, 256, 300, 700, 1024, 17])]
    pairs = [(p, t) for p in pats for t in texts]
    seqs, pa, pb = _batch(pairs)
    for mode in ("nw", "sw"):   # the rule's strip side
        name, bits, got = _info_and_scores(ctx, mode, seqs, pa, pb, (1, -4, -6, -1))
        assert STRIP in name and " + " not in name and bits == 32
        assert got == _want(pairs, mode, (1, -4, -6, -1))[0]
    # SW with mismatch > 0: padding rows could win on the strips
    name, bits, got = _info_and_scores(ctx, "sw", seqs, pa, pb, (2, 1, -3, -1))
    assert STRIP not in name and bits == 0
    assert got == _want(pairs, "sw", (2, 1, -3, -1))[0]
    # SG never runs on the strips
    name, bits, got = _info_and_scores(ctx, "sg", seqs, pa, pb, (1, -4, -6, -1))
    assert STRIP not in name and bits == 0
    assert got == _want(pairs, "sg", (1, -4, -6, -1))[0]
    # texts that use all 256 byte values: no byte left to pad short patterns with
    all_bytes = bytes(range(256))
    texts = [bytes(rng.sample(list(all_bytes), 256)) + _rand(rng, 200, all_bytes) for _ in range(3)]
    pats = [_mutate(rng, texts[k % 3][10:10 + n], all_bytes)[:n] for k, n in enumerate([9, 100, 257, 400])]
    pairs = [(p, t) for p in pats for t in texts]
    seqs, pa, pb = _batch(pairs)
    for mode in ("nw", "sw"):
        name, bits, got = _info_and_scores(ctx, mode, seqs, pa, pb, (1, -4, -6, -1))
        assert STRIP not in name and bits == 0
        assert got == _want(pairs, mode, (1, -4, -6, -1))[0], mode


# ------------------------------------------------------------------ 6. the batch object
def _all_pairs_list(seed):
    rng = random.Random(seed)
    texts = [_rand(rng, m, b"ACGT") for m in (900, 901, 333, 2000)]
    pats = [_mutate(rng, texts[k % 4][k:k + n], b"ACGT")[:n] for k, n in enumerate([150] * 70 + [31, 32, 33, 52, 53, 104, 105, 0, 1, 260])]
    seqs = pats + texts + [b""]
    pa = [x for x in range(len(pats)) for _ in range(5)]
    pb = [len(pats) + y for _ in range(len(pats)) for y in range(5)]
    return seqs, pa, pb


@pytest.mark.parametrize("mode", MODES)
def test_batch_object(ctx, mode):
    import torch
    sc = (1, -4, -6, -1)
    seqs, pa, pb = _all_pairs_list(5)   # more than 64 patterns per text, empty sides, patterns of several strip heights
    want = _want([(seqs[a], seqs[b]) for a, b in zip(pa, pb)], mode, sc)[0]
    b = ctx.batch_gotoh(mode, seqs, pa, pb, *sc)
    try:
        assert b.info()["cells"] == sum(len(seqs[a]) * len(seqs[c]) for a, c in zip(pa, pb))
        assert b.cell_bits() == (0 if mode == "sg" else 32) and b.profile_form() == 0
        b.run()
        first = b.fetch()
        b.run()
        assert b.fetch() == first == want
        assert b.last_ms() > 0 and len(b.run_times()) == 2
        d = torch.full((len(pa),), -7, dtype=torch.int32, device="cuda")
        b.set_d_scores(d.data_ptr())
        stream = torch.cuda.Stream()
        b.run(stream.cuda_stream)   # asynchronous, on the caller's stream
        stream.synchronize()
        assert d.cpu().tolist() == want
        assert b.fetch() == want
    finally:
        b.close()


@pytest.mark.parametrize("mode", MODES)
def test_index_paired_list_and_arena_chunks(ctx, mode):
    """every lane its own text; and the one-shot call cutting the list into several arenas equals the single run"""
    sc = (2, -3, -5, -2)
    seqs, pa, pb = _mixed_batch(41, 600)
    pairs = [(seqs[a], seqs[b]) for a, b in zip(pa, pb)]
    want = _want(pairs, mode, sc)
    assert ctx.scores_gotoh(mode, seqs, pa, pb, *sc) == want[0]
    assert ctx.scores_gotoh_oneshot(mode, seqs, pa, pb, *sc) == want[0]
    with switched_context(PWA_ARENA_LIMIT="16384") as c:
        assert c.scores_gotoh_oneshot(mode, seqs, pa, pb, *sc) == want[0]
        assert tuple(c.scores_gotoh_oneshot(mode, seqs, pa, pb, *sc, want_end=True)) == want


@pytest.mark.parametrize("mode", MODES)
def test_empty_and_trivial_lists(ctx, mode):
    sc = (1, -4, -6, -1)
    seqs = [b"", b"ACGTAC", b"", b"GATTACA"]
    assert ctx.scores_gotoh(mode, seqs, [], [], *sc) == []
    assert ctx.scores_gotoh_oneshot(mode, seqs, [], [], *sc) == []
    assert ctx.scores_gotoh(mode, seqs, [], [], *sc, want_end=True) == ([], [], [])
    pa, pb = [0, 1, 0, 3, 2], [1, 0, 2, 2, 3]
    pairs = [(seqs[a], seqs[b]) for a, b in zip(pa, pb)]
    want = _want(pairs, mode, sc)
    for want_end in (False, True):
        b = ctx.batch_gotoh(mode, seqs, pa, pb, *sc, want_end=want_end)
        try:
            assert b.info()["kernel"] == "none" and b.cell_bits() == 0
            b.run()
            got = b.fetch()
        finally:
            b.close()
        assert (tuple(got) if want_end else got) == (want if want_end else want[0]), (mode, want_end)


# ------------------------------------------------------------------ 7. errors
def _raw_create(pkg, ctx, mode, sc, seqs, pa, pb, want_end=0):
    L = pkg.lib()
    blob, off, _ = pkg.pack_sequences(seqs)
    a, b = (C.c_uint32 * max(len(pa), 1))(*pa), (C.c_uint32 * max(len(pb), 1))(*pb)
    h = C.c_void_p()
    rc = L.pwa_gotoh_batch_create(ctx._h, mode, *sc, blob, off, len(seqs), a, b, len(pa), want_end, C.byref(h))
    if h.value:
        L.pwa_batch_destroy(h)
    return rc


def test_errors(pkg, ctx):
    seqs = [b"ACGT", b"ACGTT"]
    for go, ge in [(1, -1), (-1, 1)]:
        assert _raw_create(pkg, ctx, 0, (1, -1, go, ge), seqs, [0], [1]) == PWA_E_INVALID
        with pytest.raises(pkg.PwaError, match="INVALID|invalid|gap"):
            ctx.scores_gotoh_oneshot("nw", seqs, [0], [1], 1, -1, go, ge)
    assert _raw_create(pkg, ctx, 3, (1, -1, -2, -1), seqs, [0], [1]) == PWA_E_INVALID      # unknown mode
    assert _raw_create(pkg, ctx, 0, (1, -1, -2, -1), seqs, [0], [2]) == PWA_E_INVALID      # index
    assert _raw_create(pkg, ctx, 0, (1, -1, -2, -1), seqs, [0], [1]) == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_one_step_over_the_range_bound(pkg, ctx, mode):
    rng = random.Random(7)
    for n, m in [(1024, 1024), (1, 1), (100, 5000)]:
        mx = ((1 << 28) - 1) // (n + m + 2)
        assert (n + m + 2) * mx < 1 << 28 <= (n + m + 2) * (mx + 1)
        p, t = _rand(rng, n, b"ACGT"), _rand(rng, m, b"ACGT")
        seqs, pa, pb = _batch([(p, t), (p[:n // 2], t[:m // 2]), (b"", t[:1])])
        half = mx // 2
        for at, over in [((mx, -1, -1, -1), (mx + 1, -1, -1, -1)), ((1, -mx, -1, -1), (1, -mx - 1, -1, -1)),
                         ((1, -1, -half, half - mx), (1, -1, -half, half - mx - 1))]:
            for want_end in (0, 1):
                assert _raw_create(pkg, ctx, mode, at, seqs, pa, pb, want_end) == 0, (n, m, at)
                assert _raw_create(pkg, ctx, mode, over, seqs, pa, pb, want_end) == PWA_E_CAPACITY, (n, m, over)
                assert _raw_create(pkg, ctx, mode, over, seqs, [0], [1], want_end) == PWA_E_CAPACITY, (n, m, over)
    with pytest.raises(pkg.PwaError, match="range"):
        ctx.scores_gotoh(["nw", "sw", "sg"][mode], [b"A" * 10, b"A" * 10], [0], [1], 1 << 24, -1, -2, -1)
    assert ctx.scores_gotoh("nw", [b"A" * 10, b"A" * 10], [0], [1], (1 << 23) - 1, -1, -2, -1) == [10 * ((1 << 23) - 1)]
