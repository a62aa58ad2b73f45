"""The canonical minimizer calls on the GPU (Context.sketch(canonical=True), Context.index(minimizers=, canonical=True),
MinimizerIndex.entries / seed_strands): every result whole against canonical_oracle.py -- at every k that changes the number of
8-byte loads, every w that changes the halo, at the edges of a sequence, of a 256-slot tile and of the blob, on palindromes, on
invalid bytes, at max_occ over both strands, in the (t, q') order of the reverse lists, over ranges and over the reuse of one index."""
import ctypes as C
import random

import numpy as np
import pytest

import canonical_oracle as KO
import chain_oracle as CO
import minimizer_oracle as MO
from conftest import switched_context
from test_canonical_oracle import order_trap
from test_gpu_seed import repeat_text

pytestmark = pytest.mark.gpu

K, W = 13, 10
TILE = 256            # slots per workgroup of the sketch kernel
INVALID, CAPACITY = -1, -5
_cache = {}


def check_sketch(ctx, seqs, k, ws):
    """ctx.sketch(canonical=True) against the oracle at every w of ws, whole, in both result forms; -> the sketches at the last w"""
    hashed = [KO.hashes(s, k) for s in seqs]
    for w in ws:
        want = [KO.sketch(s, k, w, hashed=h) for s, h in zip(seqs, hashed)]
        got = ctx.sketch(seqs, k, w, canonical=True)
        assert got == want, (k, w)
        arrays = ctx.sketch(seqs, k, w, as_arrays=True, canonical=True)
        assert all(p.dtype == np.uint32 and h.dtype == np.uint64 and s.dtype == np.uint8 for p, h, s in arrays)
        assert [list(zip(p.tolist(), h.tolist(), s.tolist())) for p, h, s in arrays] == want
    return got


def check_entries(ix, want):
    h, p, s = ix.entries()
    assert h.dtype == np.uint64 and p.dtype == np.uint32 and s.dtype == np.uint8
    assert list(zip(h.tolist(), p.tolist(), s.tolist())) == want and ix.stats["minimizers"] == len(want)


def check_seed(ctx, ix, reads, max_occ=64, entries=None, budget=0):
    """ix.seed_strands against the oracle, whole, with the call's stats (budget: the context's PWA_OCC_CHUNK_HITS, where it has
    one), the byte-for-byte meaning of every anchor and chain()'s verdict on every list; -> the oracle's lists in the call's order
    (2 r, 2 r + 1)"""
    want, looked = KO.seed(ix.text, reads, ix.k, ix.w, max_occ, entries=entries)
    got = ix.seed_strands(reads, max_occ)
    assert got == KO.by_strand(want), (ix.k, ix.w, max_occ)
    n = len(reads)
    for i, lst in enumerate(got):
        seq = reads[i] if i < n else CO.revcomp(reads[i - n])
        assert all(ix.text[t:t + ln] == seq[q:q + ln] for t, q, ln in lst), i
    assert CO.validate(got) == (0, None)
    assert len(ctx.chain(got)) == 2 * n                                         # the call's own order check accepts every list
    st = ix.seed_stats
    assert set(st) == {"sketch_ms", "search_ms", "sort_ms", "slots", "minimizers", "hits", "ranges"}
    assert st["hits"] == sum(len(a) for a in want) and st["minimizers"] == looked
    assert st["slots"] == sum(max(len(r) - ix.k + 1, 0) for r in reads)
    assert st["ranges"] == len(MO.ranges(ix.stats["minimizers"], [len(r) for r in reads], ix.k, max_occ, budget))
    return want


@pytest.mark.parametrize("k", [1, 2, 15, 16, 31])
def test_sketch_and_entries_at_every_load_count_and_halo(ctx, k):
    rng = random.Random(300 + k)
    text = CO.random_text(rng, 1003)
    # reads that start at every offset mod 8 in the blob: lengths 8 m + 1 move each next read on by one
    reads = [text[100 + 40 * a:100 + 40 * a + 8 * (k + 9) + 1] for a in range(8)]
    got = check_sketch(ctx, [text] + reads, k, (1, 10, 64, 128))
    assert got[0] and all(got[1:]) and {s for _, _, s in got[0]} == {0, 1}
    for w in (1, 10, 128):
        with ctx.index(text, minimizers=(k, w), canonical=True) as ix:
            assert ix.canonical and (ix.k, ix.w) == (k, w)
            check_entries(ix, KO.index(text, k, w))


@pytest.mark.parametrize("w", [1, 10, 64, 128])
def test_sketch_kmer_counts_at_the_window_and_the_tile(ctx, w):
    rng = random.Random(400 + w)
    for k in (5, 6):
        counts = [0, 1, w - 1, w, w + 1, TILE - 1, TILE, TILE + 1, 0, 1]
        seqs = [CO.random_text(rng, n + k - 1) if n else b"ACG" for n in counts]
        got = check_sketch(ctx, seqs, k, (w,))
        assert got[0] == [] and len(got[1]) <= 1 and len(got[-1]) <= 1
        for n in (TILE - 1, TILE, TILE + 1):                       # ... and each alone, from slot 0
            check_sketch(ctx, [CO.random_text(rng, n + k - 1)], k, (w,))
        assert check_sketch(ctx, [], k, (w,)) == [] and check_sketch(ctx, [b"", b"AC"], k, (w,)) == [[], []]


def test_sketch_tile_edges(ctx):
    rng = random.Random(3)
    k, w = 7, 10
    seq = CO.random_text(rng, 700)
    picked = [(p, s) for p, _, s in KO.sketch(seq, k, w) if 20 <= p <= 200]
    assert len(picked) > 10 and {s for _, s in picked} == {0, 1}
    for p, _ in picked[:6]:
        # the minimizer on the last lane of tile 0, its windows reaching into tile 1; and on the first lane of tile 1
        for first in (TILE - 1 - p, TILE - p):
            got = check_sketch(ctx, [CO.random_text(rng, first + k - 1), seq], k, (w,))
            assert p in [x for x, _, _ in got[1]]
    # four tiles over many reads of fewer k-mers than w: a neighbouring read's adjacent k-mer is often the smaller one
    ragged = [CO.random_text(rng, rng.randint(k, k + 8)) for _ in range(150)] + [CO.random_text(rng, 40) for _ in range(20)]
    check_sketch(ctx, ragged, k, (w,))
    assert 3 * TILE < sum(max(len(r) - k + 1, 0) for r in ragged) <= 6 * TILE
    # the blob's last byte: a last sequence of one k-mer, of w k-mers, and an empty one behind it
    for tail in ([seq[:k]], [seq[:k + w - 1]], [seq[:k], b""]):
        got = check_sketch(ctx, ragged[:5] + tail, k, (w,))
        assert got[5] and got[5][-1][0] <= len(tail[0]) - k


def test_palindromes_are_never_selected(ctx):
    assert check_sketch(ctx, [b"AT" * 40, b"CG" * 40, b"ACGT"], 2, (1, 3, 128))[:2] == [[], []]   # every 2-mer its own reverse complement
    # of ACGT repeated at k = 4, ACGT and GTAC are palindromes and CGTA and TACG are not: the odd starts alone are ever selected
    got = check_sketch(ctx, [b"ACGT" * 40], 4, (1, 2, 5))
    assert got[0] and all(p % 2 == 1 for p, _, _ in got[0])
    assert [p for p, _, _ in ctx.sketch([b"ACGT" * 40], 4, 1, canonical=True)[0]] == list(range(1, 157, 2))
    pal12 = b"ACGGTCGACCGT"
    assert [p for p, _, _ in check_sketch(ctx, [b"GG" + pal12 + b"TT", pal12], 12, (1,))[0]] == [0, 1, 3, 4]
    for text in (b"AT" * 40, pal12):
        with ctx.index(text, minimizers=(len(text) if text == pal12 else 2, 3), canonical=True) as ix:
            check_entries(ix, [])
            assert check_seed(ctx, ix, [text, b"ACGTTGCA" * 4]) == [[]] * 4 and ix.seed_stats["ranges"] == 0


def test_a_read_that_is_its_own_reverse_complement(ctx):
    rng = random.Random(31)
    half = CO.random_text(rng, 150)
    own = half + CO.revcomp(half)
    assert CO.revcomp(own) == own
    text = CO.random_text(rng, 500) + own + CO.random_text(rng, 400) + half + CO.random_text(rng, 300)
    for k, w in [(11, 5), (12, 5), (7, 1)]:
        with ctx.index(text, minimizers=(k, w), canonical=True) as ix:
            want = check_seed(ctx, ix, [own, half, CO.revcomp(half)])
            # revcomp(own) is own: whatever matches forward matches reverse; the sketch's ties may differ, the chain may not
            fw, rv = (CO.chain(lst, want_dp=False) for lst in want[:2])
            assert abs(fw["t_begin"] - fw["q_begin"] - 500) <= 1 and abs(rv["t_begin"] - rv["q_begin"] - 500) <= 1
            assert want[2] and want[3] and want[4] and want[5]


def test_the_order_trap_and_several_t_per_q(ctx):
    text, read, x, w, t, (q1, q2) = order_trap()
    k, n = len(x), len(read)
    with ctx.index(text, minimizers=(k, w), canonical=True) as ix:
        want = check_seed(ctx, ix, [read, CO.revcomp(read), x])
        assert [a for a in want[1] if a[0] == t] == [(t, n - k - q2, k), (t, n - k - q1, k)]             # equal t: ascending q'
        assert [a for a in want[2] if a[0] == t] == [(t, n - k - q2, k), (t, n - k - q1, k)]             # ... and forward, of the reverse read
        assert want[4] == [] and want[5] == [(t, 0, k)]
    # x at three places forward and two reverse, a read with x at two starts: every t with both q, each list in (t, q) order
    rng = random.Random(32)
    fill = lambda m: bytes(rng.choice(b"ACGT") for _ in range(m))
    parts = [fill(50), x, fill(60), x, fill(70), CO.revcomp(x), fill(40), x, fill(30), CO.revcomp(x), fill(20)]
    rep = b"N".join(parts)
    at = [sum(len(p) + 1 for p in parts[:i]) for i in (1, 3, 5, 7, 9)]
    with ctx.index(rep, minimizers=(k, w), canonical=True) as ix:
        want = check_seed(ctx, ix, [read, b"N" + x + b"N"])
        assert [a for a in want[0] if a[0] in at] == [(a, q, k) for a in (at[0], at[1], at[3]) for q in (q1, q2)]
        assert [a for a in want[1] if a[0] in at] == [(a, n - k - q, k) for a in (at[2], at[4]) for q in (q2, q1)]
        # max_occ counts a minimizer's hits over both strands together: five
        sizes = {m: [len(lst) for lst in check_seed(ctx, ix, [b"N" + x + b"N"], m)] for m in (4, 5, 6)}
        assert sizes[4] == [0, 0] and sizes[5] == sizes[6] == [3, 2]


def test_invalid_bytes(ctx):
    rng = random.Random(5)
    k, w = 6, 8
    base = CO.random_text(rng, 400)
    put = lambda at, what: base[:at] + what + base[at + len(what):]
    seqs = [put(100, b"N"), put(100, b"a"), put(100, b"\0"), put(100, b"\x80"), put(100, b"\xff"), put(399, b"N"), put(0, b"N"),
            put(150, b"N" * (w + k + 5)),                 # an invalid run longer than w + k: windows with nothing valid
            b"N" * 50, b"acgt" * 20, put(0, b"N" * 394),  # nothing valid at all; ... but the last k-mer
            bytes(rng.choice(b"ACGTN") for _ in range(300))]
    got = check_sketch(ctx, seqs, k, (w, 1, 64, 128))
    assert got[8] == [] and got[9] == []
    assert all(not (100 - k < p <= 100) for s in got[:5] for p, _, _ in s)
    check_sketch(ctx, seqs, 31, (10,))
    text = base + b"N" + CO.revcomp(base)
    with ctx.index(text, minimizers=(k, w), canonical=True) as ix:
        check_entries(ix, KO.index(text, k, w))
        want = check_seed(ctx, ix, seqs + [CO.revcomp(s) for s in seqs[:8]], max_occ=1000)
        assert all(want[2 * i] and want[2 * i + 1] for i in range(8))


def test_empty_and_short_inputs(ctx):
    for n in (0, 4, 5):                                                        # n = 0, n < k, n = k
        with ctx.index(b"GATTA"[:n], minimizers=(5, 4), canonical=True) as ix:
            check_entries(ix, KO.index(b"GATTA"[:n], 5, 4))
            want = check_seed(ctx, ix, [b"GATTA", b"", b"GATT", b"TAATC", b"GATTACA"])
            assert want[:8] == [[(0, 0, 5)] if n == 5 else [], [], [], [], [], [], [], [(0, 0, 5)] if n == 5 else []]
            assert ix.seed_stats["ranges"] == (n == 5)
            assert ix.seed_strands([]) == [] and ix.seed_stats["ranges"] == 0
    with ctx.index(b"NNNNNNNNNN", minimizers=(3, 2), canonical=True) as ix:  # k-mers, but none valid
        assert ix.stats["minimizers"] == 0 and check_seed(ctx, ix, [b"ACGTACGT"]) == [[], []]
    with ctx.index(b"ACGTTGCATGCA" * 5, minimizers=(5, 3), canonical=True) as ix:
        assert check_seed(ctx, ix, [b"NNNNNNNN", b"acgttgca", b""]) == [[]] * 6    # reads without a valid k-mer


def ragged():
    if "ragged" not in _cache:
        text, _ = repeat_text()
        rng = random.Random(6)
        reads = []
        for i in range(300):
            ln = rng.choice([0, 5, K - 1, K, 40, 1500]) if i % 10 == 0 else rng.randint(0, 1500)
            at = rng.randrange(0, len(text) - ln + 1)
            r = CO.mutate(rng, text[at:at + ln], rng.choice([0.0, 0.05, 0.1]), alphabet=b"ACGTN" if i % 7 == 0 else b"ACGT")
            reads.append(CO.revcomp(r) if i % 2 else r)
        reads[17] = CO.revcomp(text[0:1500])             # the longest, and over the repeat unit
        entries = KO.index(text, K, W)
        hashed = [KO.hashes(r, K) for r in reads]
        _cache["ragged"] = reads, entries, KO.seed(text, reads, K, W, entries=entries), [KO.sketch(r, K, W, hashed=h) for r, h in zip(reads, hashed)]
    return _cache["ragged"]


@pytest.mark.parametrize("poison", [None, "0xA5"])
@pytest.mark.parametrize("budget", [None, "fourth", 1])
def test_ranges_give_one_result(ctx, budget, poison):
    text, _ = repeat_text()
    reads, entries, (want, looked), sketches = ragged()
    lens = [len(r) for r in reads]
    worst = [MO.worst_hits(ln, len(entries), K, 64) for ln in lens]
    hits = budget if budget != "fourth" else sum(worst) // 4 + max(worst)
    n_ranges = len(MO.ranges(len(entries), lens, K, 64, hits or 0))
    if budget is None:
        assert n_ranges == 1
    elif budget == 1:
        assert n_ranges == len([x for x in worst if x])            # every read with a k-mer runs alone
    else:
        assert 3 <= n_ranges <= 5
    assert sum(1 for lst in want[0::2] if lst) > 100 and sum(1 for lst in want[1::2] if lst) > 100

    def run(c):
        with c.index(text, minimizers=(K, W), canonical=True) as ix:
            check_entries(ix, entries)
            got = ix.seed_strands(reads)
            assert got == KO.by_strand(want) and CO.validate(got) == (0, None)
            st = ix.seed_stats
            assert (st["ranges"], st["hits"], st["minimizers"]) == (n_ranges, sum(len(a) for a in want), looked)
            arrays = ix.seed_strands(reads, as_arrays=True)
            assert all(a.dtype == np.uint32 and a.shape == (len(x), 3) for a, x in zip(arrays, got))
            assert [[tuple(x) for x in a.tolist()] for a in arrays] == got
            assert len(c.chain(arrays)) == 2 * len(reads)
        assert c.sketch(reads, K, W, canonical=True) == sketches     # cut into ranges of sequences by the same budget, over k-mers

    if budget is None and poison is None:
        run(ctx)
        return
    env = {}
    if budget is not None:
        env["PWA_OCC_CHUNK_HITS"] = hits
    if poison is not None:
        env["PWA_POISON"] = poison
    with switched_context(**env) as c:
        run(c)
        if poison is not None:
            assert c.poison_stats()["buffers"] > 0


def test_one_index_many_calls_and_the_pairing_of_calls_and_kinds(ctx, pkg):
    text, _ = repeat_text()
    entries = KO.index(text, K, W)
    rng = random.Random(7)
    L = pkg.lib()
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))

    def fetch(ix, cap):
        t, q = np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32), np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32)
        return L.pwa_mm_seed_fetch(ix._ix, u32p(t), u32p(q), cap), t, q

    with ctx.index(text, minimizers=(K, W), canonical=True) as ix, ctx.index(text[:2000], minimizers=(K, W)) as plain:
        assert fetch(ix, 10)[0] == INVALID                                     # no seeding has run on it
        calls = [([text[a:a + 700] for a in (100, 5000)] + [CO.revcomp(text[20000:20700]), CO.mutate(rng, CO.revcomp(text[9000:9800]), 0.05)], 64),
                 ([CO.revcomp(text[7300:7340]), b""], 5),                       # a smaller call after a larger one
                 ([CO.mutate(rng, text[a:a + 300], 0.02) for a in range(0, 29000, 3000)], 1)]
        for reads, max_occ in calls:
            want = check_seed(ctx, ix, reads, max_occ, entries)
            assert ctx.seed_stats == ix.seed_stats
            flat = [a for lst in want for a in lst]                             # lists 2 r and 2 r + 1 are consecutive in the kept anchors
            rc, t, q = fetch(ix, len(flat))
            assert rc == 0 and list(zip(t.tolist(), q.tolist()))[:len(flat)] == [(a[0], a[1]) for a in flat]
            rc, t, q = fetch(ix, len(flat) + 5)                                 # nothing of an earlier call behind this one's anchors
            assert rc == 0 and set(t[len(flat):].tolist()) == {0xdeadbeef}
            if flat:
                assert fetch(ix, len(flat) - 1)[0] == CAPACITY
            check_entries(ix, entries)                                          # the index itself is untouched by a seeding
        # anc_off_out has 2 n + 1 entries, and not one more
        reads, _ = calls[0]
        off = np.zeros(len(reads) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in reads])
        anc = np.full(2 * len(reads) + 2, 7, dtype=np.uint64)
        assert L.pwa_mm_seed_strands(ix._ix, b"".join(reads), u64p(off), len(reads), 64, u64p(anc)) == 0
        want, _ = KO.seed(text, reads, K, W, entries=entries)
        assert anc.tolist() == [sum(len(lst) for lst in want[:i]) for i in range(2 * len(reads) + 1)] + [7]
        # each wrong pairing of a call and an index kind, at the C boundary and in Python; the kept anchors stay
        before = dict(ix.seed_stats)
        assert L.pwa_mm_seed(ix._ix, b"".join(reads), u64p(off), len(reads), 64, u64p(anc)) == INVALID
        assert b"pwa_mm_seed_strands seeds it" in L.pwa_last_error(ctx._h)     # the message names the other call
        assert L.pwa_mm_seed_strands(plain._ix, b"".join(reads), u64p(off), len(reads), 64, u64p(anc)) == INVALID
        assert b"pwa_mm_seed seeds a plain index" in L.pwa_last_error(ctx._h)
        hsh, pos, std = np.zeros(len(entries), dtype=np.uint64), np.zeros(len(entries), dtype=np.uint32), np.zeros(len(entries), dtype=np.uint8)
        assert L.pwa_mm_fetch_canonical(plain._ix, u64p(hsh), u32p(pos), std.ctypes.data_as(C.POINTER(C.c_uint8)), len(entries)) == INVALID
        assert L.pwa_mm_fetch_canonical(ix._ix, u64p(hsh), u32p(pos), std.ctypes.data_as(C.POINTER(C.c_uint8)), len(entries) - 1) == CAPACITY
        assert L.pwa_mm_fetch_canonical(ix._ix, u64p(hsh), u32p(pos), None, len(entries)) == INVALID
        assert L.pwa_mm_fetch(ix._ix, u64p(hsh), u32p(pos), len(entries)) == 0  # on a canonical index: hash and t as ever
        assert list(zip(hsh.tolist(), pos.tolist())) == [(h, t) for h, t, _ in entries]
        assert L.pwa_mm_seed_strands(ix._ix, b"".join(reads), u64p(off), len(reads), 0, u64p(anc)) == INVALID
        assert L.pwa_mm_seed_strands(ix._ix, b"".join(reads), u64p(off), len(reads), 64, None) == INVALID
        assert L.pwa_mm_seed_strands(ix._ix, None, u64p(off), len(reads), 64, u64p(anc)) == INVALID
        assert fetch(ix, int(anc[2 * len(reads)]))[0] == 0 and ix.seed_stats == before
        for call, index in [(ix.seed, ix), (plain.seed_strands, plain)]:
            with pytest.raises(ValueError):
                call(reads)
        with pytest.raises(ValueError):
            ctx.seed(ix, reads, K)
        with pytest.raises(ValueError):
            ix.seed_strands(reads, 0)
        assert plain.seed(reads[:1]) == MO.seed(text[:2000], reads[:1], K, W)[0] and not plain.canonical
    ix.close()                                                                  # twice is harmless
    with pytest.raises(pkg.PwaError):
        ix.seed_strands([b"ACGT"])
