"""k-edit approximate search on the GPU (Context.count_approx / find_approx, pwa_approx_*) against the numpy oracle
(approx_oracle.py), against the exact search and the semi-global scores that exist beside it, and at its limits."""
import ctypes as C

import numpy as np
import pytest

import approx_oracle as AO
from conftest import load_pkg, switched_context

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
DNA = b"ACGT"
DEFAULT_CHUNK = 4096


def expect(text, patterns, ks):
    """per pattern its (end, dist) list; the last row of a pattern is computed once however many bounds it comes with"""
    rows, out = {}, []
    for p, k in zip(patterns, ks):
        if p not in rows:
            rows[p] = AO.last_row(p, text)
        row = rows[p]
        e = np.nonzero(row[1:] <= k)[0] + 1
        out.append([(int(x), int(row[x])) for x in e])
    return out


def check(ctx, text, patterns, ks, want=None):
    want = expect(text, patterns, ks) if want is None else want
    got = ctx.find_approx(text, patterns, ks)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g == w, (q, len(patterns[q]), ks[q], g[:5], w[:5])
    counts, best = ctx.count_approx(text, patterns, ks)
    assert counts == [len(w) for w in want]
    assert best == [AO.best(w) for w in want]
    return want


def planted(rng, pattern, n, alphabet, edits, copies=4):
    """about n symbols of noise with mutated copies of pattern in it, an exact one among them"""
    gap = max(1, (n - copies * len(pattern)) // (copies + 1))
    parts = []
    for c in range(copies):
        parts.append(AO.random_seq(rng, gap, alphabet))
        parts.append(AO.mutate(rng, pattern, 0 if c == 1 else int(rng.integers(0, edits + 1)), alphabet))
    parts.append(AO.random_seq(rng, gap, alphabet))
    return b"".join(parts)


@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512])
def test_word_edges(ctx, m):
    rng = np.random.default_rng(1000 + m)
    p = AO.random_seq(rng, m, DNA)
    text = planted(rng, p, 2000, DNA, max(1, m // 4))
    ks = [0, 1, m // 4, m - 1, m, m + 3]
    want = check(ctx, text, [p] * len(ks), ks)
    assert len(want[0]) >= 1 and len(want[4]) == len(text)   # the exact copy; k >= m: every end


@pytest.mark.parametrize("m", [64, 65, 128, 512])
def test_carry_chains(ctx, m):
    p = b"A" * m
    for text in (b"A" * 700, b"A" * 300 + b"C" + b"A" * 300):
        check(ctx, text, [p] * 4, [0, 1, 2, m])


def test_seams_of_tasks_and_slices(ctx):
    """Chunks of 64 columns and slices of 100 staged hits: hits that end one before, on and one after a chunk boundary, whose
    alignments start inside the warm-up of their task, equal the default context's (one task per pattern here) and the oracle's."""
    rng = np.random.default_rng(77)
    pats = [AO.random_seq(rng, m, DNA) for m in (20, 70, 130, 5)]
    ks = [2, 5, 10, 1]
    text = bytearray(AO.random_seq(rng, 3000, DNA))
    where = ((0, 2), (1, 12), (2, 23), (3, 33))
    for q, c in where:   # copies with 0, 1, 1 edits that end at 64 c - 1, 64 (c + 4) and 64 (c + 8) + 1: no two overlap
        for x, d in enumerate((-1, 0, 1)):
            end = 64 * (c + 4 * x) + d
            copy = AO.mutate(rng, pats[q], min(x, 1), DNA)
            text[end - len(copy):end] = copy
    text = bytes(text)
    want = expect(text, pats, ks)
    for q, c in where:
        ends = {e for e, _ in want[q]}
        assert 64 * c - 1 in ends and 64 * (c + 4) in ends and 64 * (c + 8) + 1 in ends
    check(ctx, text, pats, ks, want)
    with switched_context(PWA_APPROX_CHUNK=64, PWA_OCC_CHUNK_HITS=100) as small:
        check(small, text, pats, ks, want)
        assert small.approx_stats["tasks"] == len(pats) * 47
        many = check(small, text, pats, [len(p) for p in pats], None)   # every end a hit: 3000 per pattern through slices of 100
        assert [len(w) for w in many] == [3000] * len(pats)


def lane_group_patterns():
    """201 patterns: 63 of one word, 64 of two, 65 of three, 9 over the classes above"""
    rng = np.random.default_rng(201)
    lens = [int(rng.integers(1, 65)) for _ in range(63)] + [int(rng.integers(65, 129)) for _ in range(64)]
    lens += [int(rng.integers(129, 193)) for _ in range(65)] + [200, 256, 257, 320, 384, 385, 448, 449, 512]
    order = rng.permutation(len(lens))
    lens = [lens[i] for i in order]
    pats = [AO.random_seq(rng, m, DNA) for m in lens]
    ks = [int(rng.choice([0, 1, m // 8, m // 3, m, 0xffffffff])) for m in lens]
    return rng, pats, ks


@pytest.mark.parametrize("n", [0, 1, 5, 63, 64, 65, 1001])
def test_lane_groups(ctx, n):
    rng, pats, ks = lane_group_patterns()
    assert len(pats) == 201
    pieces = b"".join(AO.mutate(rng, pats[q], 2, DNA) for q in rng.permutation(201)[:12])
    text = (pieces + AO.random_seq(rng, 1001, DNA))[:n]
    want = check(ctx, text, pats, ks)
    if n == 0:
        assert all(w == [] for w in want)
        assert ctx.approx_stats["tasks"] == 0 and ctx.approx_stats["columns"] == 0
    else:
        assert ctx.approx_stats["tasks"] == 201


def test_symbols_outside_the_patterns(ctx):
    rng = np.random.default_rng(5)
    pats = [AO.random_seq(rng, m, DNA) for m in (12, 40, 100)]
    noise = b"ACGTN\x00\xff"
    text = b"".join(AO.random_seq(rng, 150, noise) + AO.mutate(rng, p, 2, noise) for p in pats * 2)
    want = check(ctx, text, pats, [3, 6, 12])
    assert all(want)
    check(ctx, b"\x00\xffNN\x00", [b"ACG"], [3])   # no text symbol is a pattern symbol


def test_protein_alphabet(ctx):
    rng = np.random.default_rng(25)
    alphabet = b"ACDEFGHIKLMNPQRSTVWYBZXUO"
    assert len(set(alphabet)) == 25
    p = AO.random_seq(rng, 300, alphabet)
    text = planted(rng, p, 1500, alphabet, 30, copies=3)
    want = check(ctx, text, [p, p, p[:90]], [0, 40, 9])
    assert want[0] and len(want[1]) > len(want[0])


def test_thirty_two_symbols_at_full_length(ctx):
    rng = np.random.default_rng(32)
    alphabet = bytes(range(1, 33))
    p = bytearray(AO.random_seq(rng, 512, alphabet))
    p[:32] = alphabet   # all 32 are there
    p = bytes(p)
    text = planted(rng, p, 1800, alphabet + b"\x00\xfe", 40, copies=2)
    want = check(ctx, text, [p, p, p[100:165]], [0, 60, 5])
    assert want[0] and want[2]


def raw_find(ctx, text, patterns, ks):
    pkg = load_pkg()
    blob, off, pats = pkg.pack_sequences(patterns)
    n_pat = len(pats)
    cnt, kd = (C.c_uint32 * max(n_pat, 1))(), (C.c_uint32 * max(n_pat, 1))(*ks)
    return ctx._L.pwa_approx_find(ctx._h, text, len(text), blob, off, n_pat, kd, cnt, None, None)


def test_limits(ctx):
    text = b"ACGTACGTAC"
    assert raw_find(ctx, text, [bytes(range(33))], [1]) == CAPACITY                      # 33 distinct symbols
    assert raw_find(ctx, text, [bytes(range(20)), bytes(range(16, 36))], [1, 1]) == CAPACITY   # ... over all patterns of the call
    assert raw_find(ctx, text, [bytes(range(32))], [1]) == 0
    assert raw_find(ctx, text, [b"A" * 513], [1]) == CAPACITY
    assert raw_find(ctx, text, [b"A" * 512], [1]) == 0
    assert raw_find(ctx, text, [b"ACG", b""], [1, 1]) == INVALID
    assert raw_find(ctx, b"", [b"ACG", b""], [1, 1]) == INVALID
    assert raw_find(ctx, text, [], []) == 0
    with pytest.raises(load_pkg().PwaError):
        ctx.count_approx(text, [b"A" * 513], 1)
    assert ctx.count_approx(text, [], 0) == ([], [])
    assert ctx.count_approx(b"", [b"ACG"], 5) == ([0], [None])
    assert ctx.find_approx(b"", [b"ACG"], 5) == [[]]
    assert ctx.count_approx(b"TTTT", [b"ACG"], 1) == ([0], [None])                       # no hit: -1 / 0 at the C boundary


def test_k0_is_the_exact_search(ctx):
    rng = np.random.default_rng(11)
    body = AO.random_seq(rng, 5000, DNA)
    pats = [body[s:s + m] for s, m in ((10, 8), (700, 33), (2000, 64), (4090, 12), (3000, 150))] + [b"ACG", b"TTTTTTTTTTTTTTTTTTTTTTTTTTTT"]
    text = body + b"$"   # one reference with its terminator last, as Context.find wants it
    exact = ctx.find(text, pats, refs=([0, len(text)], [0]))
    counts_exact = ctx.find(text, pats)
    hits = ctx.find_approx(text, pats, 0)
    counts, _ = ctx.count_approx(text, pats, 0)
    assert counts == counts_exact
    for p, ex, h in zip(pats, exact, hits):
        assert h == [(pos + len(p), 0) for _, pos in ex]


def test_best_is_the_semi_global_score(ctx):
    rng = np.random.default_rng(12)
    pats = [AO.random_seq(rng, m, DNA) for m in (5, 64, 65, 150, 300, 512)]
    text = b"".join(AO.random_seq(rng, 100, DNA) + AO.mutate(rng, p, len(p) // 10, DNA) for p in pats)
    _, best = ctx.count_approx(text, pats, [len(p) for p in pats])
    seqs = pats + [text]
    sg = ctx.scores("sg", seqs, list(range(len(pats))), [len(pats)] * len(pats), 0, -1, -1)
    assert [b[0] for b in best] == [-s for s in sg]


def test_capacity_and_stats(ctx):
    pkg = load_pkg()
    rng = np.random.default_rng(13)
    pats = [AO.random_seq(rng, m, DNA) for m in (10, 100, 200)]
    ks = [2, 30, 4]
    text = planted(rng, pats[2], 9000, DNA, 4, copies=5)   # three tasks per pattern at the default chunk
    want = check(ctx, text, pats, ks)
    total = sum(len(w) for w in want)
    assert total > 2
    tasks = pkg.approx_plan(len(text), [len(p) for p in pats], ks, DEFAULT_CHUNK)
    assert ctx.approx_stats["tasks"] == len(tasks) == 9
    assert ctx.approx_stats["columns"] == sum(hi - scan_lo for _, scan_lo, _, hi in tasks)
    assert ctx.approx_stats["count_ms"] > 0 and ctx.approx_stats["fill_ms"] == 0   # check() ended with the count pass alone
    ctx.find_approx(text, pats, ks)
    assert ctx.approx_stats["tasks"] == 9 and ctx.approx_stats["count_ms"] > 0 and ctx.approx_stats["fill_ms"] > 0
    blob, off, _ = pkg.pack_sequences(pats)
    kd = (C.c_uint32 * 3)(*ks)
    occ_off, occ, need = (C.c_uint64 * 4)(), (C.c_uint64 * total)(), C.c_uint64(0)
    L = ctx._L
    assert L.pwa_approx_occurrences(ctx._h, text, len(text), blob, off, 3, kd, occ_off, occ, total - 1, C.byref(need)) == CAPACITY
    assert need.value == total
    need = C.c_uint64(0)
    assert L.pwa_approx_occurrences(ctx._h, text, len(text), blob, off, 3, kd, occ_off, None, 0, C.byref(need)) == CAPACITY
    assert need.value == total
    assert L.pwa_approx_occurrences(ctx._h, text, len(text), blob, off, 3, kd, occ_off, occ, total, C.byref(need)) == 0
    assert need.value == total and list(occ_off) == [0, len(want[0]), len(want[0]) + len(want[1]), total]
    assert [(x >> 32, x & 0xffffffff) for x in occ] == [h for w in want for h in w]
