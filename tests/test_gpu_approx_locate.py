"""From a k-edit hit to a placement on the GPU (Context.starts_approx / locate_approx / align_approx, pwa_approx_starts) against the
numpy oracle (approx_locate_oracle.py), at the word, lane, slice and text edges, and at its limits.

The oracle costs m x (m + d) cells per hit, so where a list is long every start is checked against its bounds and a spread sample of
the list (the first and the last hit always) against the oracle; the lists that are there for their edges are checked whole."""
import ctypes as C
import re

import numpy as np
import pytest

import approx_locate_oracle as LO
import approx_oracle as AO
from conftest import load_pkg, switched_context
from test_gpu_approx import DNA, expect, planted

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5


def spread(count, cap):
    if count <= cap:
        return list(range(count))
    return sorted({round(x * (count - 1) / (cap - 1)) for x in range(cap)})


def check_starts(c, text, pats, hits, whole=False, cells=3e7):
    """starts_approx of these lists: every start within its bounds, and a sample of each list (whole: all of it; else about `cells`
    oracle cells' worth, 40 hits at least) equal to the oracle's -> the starts"""
    got = c.starts_approx(text, pats, hits)
    assert [len(g) for g in got] == [len(h) for h in hits]
    for q, (p, h, g) in enumerate(zip(pats, hits, got)):
        m = len(p)
        for (e, d), s in zip(h, g):
            assert s is not None and m - d <= e - s <= min(e, m + d), (q, m, e, d, s)
        for x in spread(len(h), len(h) if whole else max(40, int(cells) // (m * m))):
            e, d = h[x]
            assert g[x] == LO.start_of(p, text, e, d), (q, m, e, d, g[x])
    return got


@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512])
def test_word_edges(ctx, m):
    rng = np.random.default_rng(3000 + m)
    p = AO.random_seq(rng, m, DNA)
    text = planted(rng, p, 2000, DNA, max(1, m // 4))
    ks = [0, 1, m // 4] + ([m] if m <= 65 else [])
    hits = expect(text, [p] * len(ks), ks)
    assert hits[0] and (m > 65 or len(hits[-1]) == len(text))
    got = check_starts(ctx, text, [p] * len(ks), hits)
    assert all(e - s == m for (e, _), s in zip(hits[0], got[0]))   # an exact occurrence starts m back
    if m <= 2:   # dist = m: the empty substring
        assert any(d == m and s == e for (e, d), s in zip(hits[-1], got[-1]))


@pytest.mark.parametrize("m", [64, 65, 128, 512])
def test_carry_chains_and_text_edges(ctx, m):
    p = b"A" * m
    for text in (b"A" * 600, b"A" * 300 + b"C" + b"A" * 299):
        n = len(text)
        ks = [0, 1, 2, m]
        hits = expect(text, [p] * 4, ks)
        assert len(hits[3]) == n and hits[3][-1][0] == n and hits[3][0] == (1, m - 1)   # a hit that ends at n; hits with e < m
        got = check_starts(ctx, text, [p] * 4, hits, cells=1e7)   # (the starts of hits[3] are also known in closed form, below)
        for (e, d), s in zip(hits[3], got[3]):
            if b"C" not in text[:e]:
                assert (d, s) == (max(m - e, 0), max(e - m, 0))   # e < m: on the j = e bound
    # no symbol of the text is in the pattern: every end is a hit of distance m whose start is the end
    text = b"C" * 100
    hits = expect(text, [p], [m])
    assert hits[0] == [(e, m) for e in range(1, 101)]
    assert ctx.starts_approx(text, [p], hits) == [list(range(1, 101))]


def seam_lists():
    """hit lists of 63 / 64 / 65 hits over the patterns of one, two and three words, and a pattern without a hit"""
    rng = np.random.default_rng(63)
    lens = [20, 64, 65, 128, 129, 150]
    pats = [AO.random_seq(rng, m, DNA) for m in lens]
    text = b"".join(AO.random_seq(rng, 60, DNA) + AO.mutate(rng, p, len(p) // 16, DNA) for p in pats * 3) + AO.random_seq(rng, 30, DNA)
    full = expect(text, pats, [m // 4 for m in lens])
    hits = []
    for c, want in enumerate((63, 64, 65)):
        a, b = full[2 * c], full[2 * c + 1]
        na = min(len(a), want // 2)
        assert len(b) >= want - na
        hits += [a[:na], b[len(b) - (want - na):]]
    pats.append(b"N" * 10)
    hits.append([])
    return text, pats, hits


def test_lane_and_slice_seams(ctx):
    text, pats, hits = seam_lists()
    assert [len(hits[0]) + len(hits[1]), len(hits[2]) + len(hits[3]), len(hits[4]) + len(hits[5])] == [63, 64, 65]
    got = check_starts(ctx, text, pats, hits, whole=True)
    assert got[6] == []
    # a subset in shuffled order with duplicates
    rng = np.random.default_rng(64)
    where = {(q, h): s for q in range(len(pats)) for h, s in zip(hits[q], got[q])}
    mixed = []
    for q, h in enumerate(hits):
        pick = [h[i] for i in rng.integers(0, len(h), size=len(h) // 2 + 3)] if h else []
        mixed.append(pick)
    assert any(len(set(x)) < len(x) for x in mixed)
    want_mixed = [[where[(q, h)] for h in x] for q, x in enumerate(mixed)]
    assert ctx.starts_approx(text, pats, mixed) == want_mixed
    with switched_context(PWA_OCC_CHUNK_HITS=100) as small:   # 192 records in slices of 100: a seam inside the two-word class
        assert small.starts_approx(text, pats, hits) == got
        assert small.approx_starts_stats["hits"] == 192
        assert small.starts_approx(text, pats, mixed) == want_mixed
    with switched_context(PWA_OCC_CHUNK_HITS=1) as one:
        assert one.starts_approx(text, pats, hits) == got


def test_alphabets_and_symbols_outside_the_patterns(ctx):
    rng = np.random.default_rng(25)
    protein = b"ACDEFGHIKLMNPQRSTVWYBZXUO"
    p = AO.random_seq(rng, 300, protein)
    text = planted(rng, p, 1500, protein + b"\x00\xff", 30, copies=3)
    pats, ks = [p, p, p[:90]], [0, 40, 9]
    hits = expect(text, pats, ks)
    assert hits[0] and len(hits[1]) > len(hits[0]) and hits[2]
    check_starts(ctx, text, pats, hits)
    rng = np.random.default_rng(32)
    alphabet = bytes(range(1, 33))
    p = bytearray(AO.random_seq(rng, 512, alphabet))
    p[:32] = alphabet
    p = bytes(p)
    text = planted(rng, p, 1800, alphabet + b"\x00\xfe", 40, copies=2)
    pats, ks = [p, p, p[100:165]], [0, 60, 5]
    hits = expect(text, pats, ks)
    assert hits[0] and hits[2]
    check_starts(ctx, text, pats, hits)


def raw_starts(c, text, patterns, hits, occ_off=None):
    pkg = load_pkg()
    blob, off, pats = pkg.pack_sequences(patterns)
    oo, occ = pkg._pack_hits(hits)
    if occ_off is not None:
        oo = (C.c_uint64 * len(occ_off))(*occ_off)
    out = (C.c_uint32 * max(len(occ), 1))()
    return c._L.pwa_approx_starts(c._h, text, len(text), blob, off, len(pats), oo, occ, out)


def test_understated_distance_and_limits(ctx):
    rng = np.random.default_rng(41)
    pats = [AO.random_seq(rng, m, DNA) for m in (30, 100, 200)]
    text = b"".join(AO.random_seq(rng, 80, DNA) + AO.mutate(rng, p, 3, DNA) for p in pats * 2)
    hits = expect(text, pats, [4, 10, 12])
    want = check_starts(ctx, text, pats, hits, whole=True)
    low = [list(h) for h in hits]
    changed = []
    for q, h in enumerate(hits):
        x = next(i for i, (e, d) in enumerate(h) if d >= 1)
        low[q][x] = (h[x][0], h[x][1] - 1)
        changed.append(x)
    got = ctx.starts_approx(text, pats, low)
    for q, x in enumerate(changed):
        assert got[q][x] is None
        assert got[q][:x] + got[q][x + 1:] == want[q][:x] + want[q][x + 1:]
    assert ctx.starts_approx(text, [pats[0]], [[(1, 0)]]) == [[None]]   # one column and no more: e bounds the scan
    # an overstated distance: the first column at which row m reaches it
    high = [[(e, min(d + 2, len(p))) for e, d in h[:20]] for p, h in zip(pats, hits)]
    got = ctx.starts_approx(text, pats, high)
    assert got == [[LO.start_of(p, text, e, d) for e, d in h] for p, h in zip(pats, high)]
    # the limits with their codes
    t = b"ACGTACGTAC"
    assert raw_starts(ctx, t, [bytes(range(33))], [[(5, 1)]]) == CAPACITY
    assert raw_starts(ctx, t, [b"A" * 513], [[(5, 1)]]) == CAPACITY
    assert raw_starts(ctx, t, [b"ACG", b""], [[(5, 1)], []]) == INVALID
    assert raw_starts(ctx, t, [b"ACG", b"AC"], [[(5, 1)], [(4, 1)]], occ_off=[0, 2, 1]) == INVALID   # offsets not ascending
    assert raw_starts(ctx, t, [b"ACG"], [[(5, 1), (0, 1)]]) == INVALID    # e = 0
    assert raw_starts(ctx, t, [b"ACG"], [[(5, 1), (11, 1)]]) == INVALID   # e > n
    assert raw_starts(ctx, t, [b"ACG"], [[(5, 1), (6, 4)]]) == INVALID    # dist > m
    assert raw_starts(ctx, t, [b"ACG"], [[(10, 3)]]) == 0
    assert raw_starts(ctx, b"", [b"ACG"], [[(1, 1)]]) == INVALID
    with pytest.raises(load_pkg().PwaError):
        ctx.starts_approx(t, [b"ACG"], [[(11, 0)]])
    assert ctx.starts_approx(t, [], []) == []
    assert ctx.starts_approx(t, [b"ACG", b"T"], [[], []]) == [[], []]
    assert ctx.approx_starts_stats == dict(ms=0.0, hits=0, columns=0)
    assert ctx.starts_approx(b"", [b"ACG"], [[]]) == [[]]


def locate_case():
    rng = np.random.default_rng(52)
    pats = [AO.random_seq(rng, m, DNA) for m in (12, 64, 150, 300)] + [b"AB", b"G" * 40]
    text = b"".join(AO.random_seq(rng, 70, DNA) + AO.mutate(rng, p, len(p) // 12, DNA) for p in pats[:4] * 2) + b"A" * 40
    return text, pats, [2, 8, 16, 30, 1, 3]


def test_locate_minima_all_and_best(ctx):
    text, pats, ks = locate_case()
    rows = [AO.last_row(p, text) for p in pats]
    full = expect(text, pats, ks)
    got = ctx.locate_approx(text, pats, ks)   # "minima" is the default
    for q, p in enumerate(pats):
        want = LO.minima_from_row(rows[q], ks[q])
        assert got[q] == [(LO.start_of(p, text, e, d), e, d) for e, d in want], q
        assert len(want) < len(full[q]) or not full[q]
    assert got[4] and not got[5]   # the A run at the text's end is one plateau of AB at distance 1; there is no run of G
    assert [e for _, e, _ in got[4]][-1] <= len(text) - 39
    assert ctx.locate_approx(text, pats, ks, select="minima") == got
    every = ctx.locate_approx(text, pats, ks, select="all")
    assert [[(e, d) for _, e, d in x] for x in every] == full
    for q, x in enumerate(every):
        for i in spread(len(x), 60):
            assert x[i][0] == LO.start_of(pats[q], text, x[i][1], x[i][2])
    best = ctx.locate_approx(text, pats, ks, select="best")
    _, named = ctx.count_approx(text, pats, ks)
    for q, p in enumerate(pats):
        if named[q] is None:
            assert best[q] == []
        else:
            d, e = named[q]
            assert best[q] == [(LO.start_of(p, text, e, d), e, d)]
    with pytest.raises(ValueError):
        ctx.locate_approx(text, pats, ks, select="first")


def test_locate_at_k0_is_the_exact_search(ctx):
    rng = np.random.default_rng(11)
    body = AO.random_seq(rng, 3000, DNA)
    pats = [body[s:s + m] for s, m in ((10, 8), (700, 33), (2000, 64), (2890, 12), (1000, 150))] + [b"ACG", b"TTTTTTTTTTTTTTTTTTTTTTTTTTTT"]
    text = body + b"$"   # one reference with its terminator last, as Context.find wants it
    exact = ctx.find(text, pats, refs=([0, len(text)], [0]))
    for select in ("all", "minima"):   # at k = 0 every hit is a minimum of its own
        got = ctx.locate_approx(text, pats, 0, select=select)
        for p, ex, g in zip(pats, exact, got):
            assert g == [(pos, pos + len(p), 0) for _, pos in ex]


def test_align_approx(ctx):
    text, pats, ks = locate_case()
    placed = ctx.locate_approx(text, pats, ks)
    got = ctx.align_approx(text, pats, ks)
    assert [[(a["start"], a["end"], a["dist"]) for a in x] for x in got] == placed
    assert sum(len(x) for x in got) > 10
    for q, x in enumerate(got):
        m = len(pats[q])
        for a in x:
            ops = [(int(c), o) for c, o in re.findall(rb"(\d+)([MDI])", a["cigar"])]
            assert b"".join(b"%d%s" % co for co in ops) == a["cigar"]
            n_m, n_d, n_i = (sum(c for c, o in ops if o == k) for k in (b"M", b"D", b"I"))
            tokens = re.findall(rb"\d+|\^[A-Z]+|[A-Z]", a["mdz"])
            assert b"".join(tokens) == a["mdz"]
            mism = sum(1 for t in tokens if len(t) == 1 and not t.isdigit())
            assert sum(len(t) - 1 for t in tokens if t[:1] == b"^") == n_d
            assert sum(int(t) for t in tokens if t.isdigit()) + mism == n_m
            assert n_d + n_i + mism == a["dist"], (q, a)
            assert (n_m + n_d, n_m + n_i) == (m, a["end"] - a["start"])
            assert a["score"] == -a["dist"]
    best = ctx.align_approx(text, pats, ks, select="best")
    assert [len(x) for x in best] == [1 if x else 0 for x in got]
    assert ctx.align_approx(text, [b"N" * 9], 2) == [[]]
    # hits of dist = m, start == end: the empty-text convention of the alignment call
    assert ctx.align_approx(b"CCCC", [b"AAA"], 3, select="all") == [[dict(start=e, end=e, dist=3, score=-3, cigar=b"3D", mdz=b"0^AAA0") for e in (1, 2, 3, 4)]]


def test_stats(ctx):
    text, pats, ks = locate_case()
    hits = expect(text, pats, ks)
    got = ctx.starts_approx(text, pats, hits)
    st = ctx.approx_starts_stats
    total = sum(len(h) for h in hits)
    assert total > 100 and st["hits"] == total and st["ms"] > 0
    assert st["columns"] == sum(e - s for h, g in zip(hits, got) for (e, _), s in zip(h, g))
    assert 0 < st["columns"] <= sum(min(e, len(p) + d) for p, h in zip(pats, hits) for e, d in h)
    ctx.count_approx(text, pats, ks)
    find_stats = dict(ctx.approx_stats)
    ctx.starts_approx(text, pats, hits)
    assert ctx.approx_stats == find_stats   # the search calls' stats are theirs alone
