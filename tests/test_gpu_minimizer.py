"""The minimizer calls on the GPU (Context.sketch, Context.index(minimizers=), MinimizerIndex.entries / seed): every result whole
against minimizer_oracle.py -- at every k and w that changes the number of 8-byte loads or the halo, at the edges of a sequence, of a
256-slot tile and of the blob, on ties, on invalid bytes, at max_occ, in the (t, q) order, over ranges and over the reuse of one index."""
import ctypes as C
import random

import numpy as np
import pytest

import chain_oracle as CO
import minimizer_oracle as MO
from conftest import switched_context
from test_gpu_seed import repeat_text

pytestmark = pytest.mark.gpu

K, W = 13, 10
TILE = 256            # slots per workgroup of the sketch kernel
INVALID, CAPACITY = -1, -5
_cache = {}


def check_sketch(ctx, seqs, k, w):
    """ctx.sketch against the oracle, whole, in both result forms; -> the sketches"""
    want = [MO.sketch(s, k, w) for s in seqs]
    got = ctx.sketch(seqs, k, w)
    assert got == want, (k, w)
    arrays = ctx.sketch(seqs, k, w, as_arrays=True)
    assert all(p.dtype == np.uint32 and h.dtype == np.uint64 for p, h in arrays)
    assert [list(zip(p.tolist(), h.tolist())) for p, h in arrays] == want
    return got


@pytest.mark.parametrize("k", [1, 4, 15, 16, 17, 31])
def test_sketch_at_every_load_count_and_halo(ctx, k):
    rng = random.Random(100 + k)
    text = CO.random_text(rng, 1003)
    # reads that start at every offset mod 8 in the blob: lengths 8 m + 1 move each next read on by one
    reads = [text[100 + 40 * a:100 + 40 * a + 8 * (k + 9) + 1] for a in range(8)]
    for w in (1, 2, 10, 63, 64, 65, 128):
        got = check_sketch(ctx, [text] + reads, k, w)
        assert len(got[0]) >= (len(text) - k + 1) // w and all(got[1:])


@pytest.mark.parametrize("w", [1, 2, 10, 64, 128])
def test_sketch_kmer_counts_at_the_window_and_the_tile(ctx, w):
    rng = random.Random(200 + w)
    k = 5
    counts = [0, 1, w - 1, w, w + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 0, 1]
    seqs = [CO.random_text(rng, n + k - 1) if n else b"ACG" for n in counts]
    got = check_sketch(ctx, seqs, k, w)
    assert got[0] == [] and len(got[1]) == 1 and len(got[-1]) == 1
    for n in (TILE - 1, TILE, TILE + 1, 3 * TILE + 1):           # ... and each alone, from slot 0
        check_sketch(ctx, [CO.random_text(rng, n + k - 1)], k, w)
    assert check_sketch(ctx, [], k, w) == [] and check_sketch(ctx, [b"", b"AC"], k, w) == [[], []]


def test_sketch_tile_edges(ctx):
    rng = random.Random(3)
    k, w = 7, 10
    seq = CO.random_text(rng, 700)
    picked = [p for p, _ in MO.sketch(seq, k, w) if 20 <= p <= 200]
    assert len(picked) > 10
    for p in picked[:6]:
        # the minimizer on the last lane of tile 0, its windows reaching into tile 1; and on the first lane of tile 1
        for first in (TILE - 1 - p, TILE - p):
            got = check_sketch(ctx, [CO.random_text(rng, first + k - 1), seq], k, w)
            assert p in [x for x, _ in got[1]]
    # one tile over many reads of fewer k-mers than w: a neighbouring read's adjacent k-mer is often the smaller one
    ragged = [CO.random_text(rng, rng.randint(k, k + 8)) for _ in range(150)] + [CO.random_text(rng, 40) for _ in range(20)]
    got = check_sketch(ctx, ragged, k, w)
    assert MO.sketch_joined(ragged, k, w) != got and sum(max(len(r) - k + 1, 0) for r in ragged) > 3 * TILE
    # the blob's last byte: a last sequence of one k-mer, of w k-mers, and an empty one behind it
    for tail in ([seq[:k]], [seq[:k + w - 1]], [seq[:k], b""]):
        got = check_sketch(ctx, ragged[:5] + tail, k, w)
        assert got[5] and got[5][-1][0] <= len(tail[0]) - k


def test_sketch_ties(ctx):
    for k, w in [(3, 5), (8, 10), (1, 128), (31, 64)]:
        got = check_sketch(ctx, [b"A" * 300, b"AC" * 150, b"A" * (k + w - 2)], k, w)
        assert [p for p, _ in got[0]] == list(range(0, 300 - k + 1 - w + 1))      # the leftmost of every window
        assert [p for p, _ in got[2]] == [0]                                          # K = w - 1: one window
    # the k-mer of the smallest hash twice, its starts w - 1 and w apart
    k, w = 4, 9
    low = min(range(256), key=lambda v: MO.mix(v, 255))
    m = bytes(b"ACGT"[(low >> 2 * (3 - i)) & 3] for i in range(4))
    rng = random.Random(4)
    for d in (w - 1, w):
        for _ in range(200):
            fill = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
            seq = fill(30) + m + fill(d - 4) + m + fill(30)
            if [p for p in range(len(seq) - 3) if seq[p:p + 4] == m] == [30, 30 + d]:
                break
        else:
            raise AssertionError("no such sequence")
        got = check_sketch(ctx, [seq], k, w)[0]
        assert (30, MO.mix(low, 255)) in got and (30 + d, MO.mix(low, 255)) in got


def test_sketch_invalid_bytes(ctx):
    rng = random.Random(5)
    k, w = 6, 8
    base = CO.random_text(rng, 400)
    put = lambda at, what: base[:at] + what + base[at + len(what):]
    seqs = [put(100, b"N"), put(100, b"a"), put(100, b"\0"), put(100, b"\x80"), put(100, b"\xff"), put(399, b"N"), put(0, b"N"),
            put(150, b"N" * (w + k + 5)),                 # an invalid run longer than w + k: windows with nothing valid
            b"N" * 50, b"acgt" * 20, put(0, b"N" * 394),  # nothing valid at all; ... but the last k-mer
            bytes(rng.choice(b"ACGTN") for _ in range(300))]
    got = check_sketch(ctx, seqs, k, w)
    assert got[8] == [] and got[9] == [] and [p for p, _ in got[10]] == [394]
    assert all(not (100 - k < p <= 100) for s in got[:5] for p, _ in s)
    for w2 in (1, 64, 128):
        check_sketch(ctx, seqs, k, w2)
    check_sketch(ctx, seqs, 31, 10)


def test_sketch_validation_and_capacity(ctx, pkg):
    L = pkg.lib()
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    out, pos, hsh, need = u64(7, 7, 7), (C.c_uint32 * 64)(), (C.c_uint64 * 64)(), C.c_uint64(7)
    seq = b"ACGTTGCAAGGCTTAACCGG"
    sk = lambda off, n, k, w, cap=64: L.pwa_mm_sketch(ctx._h, seq, off, n, k, w, out, pos, hsh, cap, C.byref(need))
    for k, w, code in [(0, 5, INVALID), (1, 5, 0), (31, 5, 0), (32, 5, INVALID), (5, 0, INVALID), (5, 1, 0), (5, 128, 0), (5, 129, INVALID)]:
        assert sk(u64(0, 20), 1, k, w) == code, (k, w)
    assert sk(u64(0, 20, 10), 2, 5, 4) == INVALID and sk(u64(0, 20, 20 + (1 << 31)), 2, 5, 4) == CAPACITY
    assert sk(u64(0, 1 << 31, 5), 2, 5, 4) == CAPACITY and sk(u64(0, 10, 5, 5 + (1 << 31)), 3, 5, 4) == INVALID   # the first offender decides
    assert sk(u64(0, 20), 1, 0, 5) == INVALID and L.pwa_mm_sketch(ctx._h, seq, u64(0, 20), 1, 5, 4, None, pos, hsh, 64, None) == INVALID
    want = [MO.sketch(seq[:12], 3, 4), MO.sketch(seq[12:], 3, 4)]
    total = len(want[0]) + len(want[1])
    assert sk(u64(0, 12, 20), 2, 3, 4) == 0 and need.value == total and list(out) == [0, len(want[0]), total]
    out[1] = out[2] = 7
    assert sk(u64(0, 12, 20), 2, 3, 4, cap=total - 1) == CAPACITY and need.value == total and list(out) == [0, len(want[0]), total]
    ix = C.c_void_p()
    for k, w in [(0, 5), (32, 5), (5, 0), (5, 129)]:
        assert L.pwa_mm_create(ctx._h, seq, 20, k, w, C.byref(ix)) == INVALID and not ix
    assert L.pwa_mm_create(ctx._h, seq, 1 << 31, 5, 5, C.byref(ix)) == CAPACITY and not ix
    assert L.pwa_mm_create(ctx._h, None, 20, 5, 5, C.byref(ix)) == INVALID and L.pwa_mm_create(ctx._h, seq, 20, 5, 5, None) == INVALID


def check_seed(ix, reads, max_occ=64, entries=None, budget=0):
    """ix.seed against the oracle, whole, with the call's stats (budget: the context's PWA_OCC_CHUNK_HITS, where it has one); -> the anchors"""
    want, looked = MO.seed(ix.text, reads, ix.k, ix.w, max_occ, entries=entries)
    got = ix.seed(reads, max_occ)
    assert got == want, (ix.k, ix.w, max_occ)
    assert CO.validate(got) == (0, None)
    st = ix.seed_stats
    assert set(st) == {"sketch_ms", "search_ms", "sort_ms", "slots", "minimizers", "hits", "ranges"}
    assert st["hits"] == sum(len(a) for a in want) and st["minimizers"] == looked
    assert st["slots"] == sum(max(len(r) - ix.k + 1, 0) for r in reads)
    assert st["ranges"] == len(MO.ranges(ix.stats["minimizers"], [len(r) for r in reads], ix.k, max_occ, budget))
    return got


def test_index_entries_and_small_texts(ctx, pkg):
    rng = random.Random(6)
    text = CO.random_text(rng, 5003, repeat=300, copies=4)
    for k, w in [(13, 10), (5, 1), (31, 128), (8, 3)]:
        with ctx.index(text, minimizers=(k, w)) as ix:
            assert isinstance(ix, pkg.MinimizerIndex) and (ix.k, ix.w, ix.text) == (k, w, text)
            want = MO.index(text, k, w)
            h, p = ix.entries()
            assert h.dtype == np.uint64 and p.dtype == np.uint32 and list(zip(h.tolist(), p.tolist())) == want
            assert ix.stats["minimizers"] == len(want) and ix.stats["build_ms"] > 0
            assert len(set(h.tolist())) < len(want) or w > 3                   # the repeat: equal hashes, ordered by t
    assert isinstance(ctx.index(text[:50]), pkg.TextIndex)
    for n in (0, 4, 5):                                                        # n = 0, n < k, n = k
        with ctx.index(b"GATTA"[:n], minimizers=(5, 4)) as ix:
            h, p = ix.entries()
            assert list(zip(h.tolist(), p.tolist())) == MO.index(b"GATTA"[:n], 5, 4) and len(h) == (n == 5)
            assert check_seed(ix, [b"GATTA", b"", b"GATT", b"GATTACA"])[:3] == [[(0, 0, 5)] if n == 5 else [], [], []]
            assert ix.seed_stats["ranges"] == (n == 5)
    with ctx.index(b"NNNNNNNNNN", minimizers=(3, 2)) as ix:                    # k-mers, but none valid
        assert ix.stats["minimizers"] == 0 and check_seed(ix, [b"ACGTACGT"]) == [[]]


def max_occ_inputs():
    """the text, its entries and the reads of test_max_occ_at_and_around_a_minimizers_count"""
    text, _ = repeat_text()
    rng = random.Random(7)
    return text, MO.index(text, K, W), [text[0:400], text[100:900], text[29000:], CO.mutate(rng, text[0:400], 0.03), text[7300:7900]]


def test_max_occ_at_and_around_a_minimizers_count(ctx):
    text, entries, reads = max_occ_inputs()
    count = {}
    for h, _ in entries:
        count[h] = count.get(h, 0) + 1
    unit = sorted(count[h] for _, h in MO.sketch(text[0:400], K, W) if h in count)
    assert unit.count(5) > 20 and unit[-1] >= 5
    with ctx.index(text, minimizers=(K, W)) as ix:
        sizes = {m: len(check_seed(ix, reads, m, entries)[0]) for m in (1, 4, 5, 6, 64, 0xffffffff)}
    assert sizes[4] < sizes[5] <= sizes[6] <= sizes[64] == sizes[0xffffffff] and sizes[5] - sizes[4] == 5 * unit.count(5)


def test_order_is_t_then_q(ctx):
    rng = random.Random(5)
    x = b"GATTACAGATTACCA"                       # 15 symbols; between invalid bytes it is the one valid k-mer of every window it is in (w <= 16)
    fill = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    text = fill(300) + b"N" + x + b"N" + fill(410) + b"N" + x + b"N" + fill(76) + b"N" + x + b"N" + fill(200)
    t1, t2, t3 = 301, 301 + 16 + 411, 301 + 16 + 411 + 16 + 77
    read = x + b"R" + fill(7) + b"R" + x + b"R" + fill(28) + b"R" + x
    q1, q2, q3 = 0, 24, 69
    for w in (1, 8, 16):
        with ctx.index(text, minimizers=(15, w)) as ix:
            got = check_seed(ix, [read, x, fill(40), read])
            assert got[0] == [(t, q, 15) for t in (t1, t2, t3) for q in (q1, q2, q3)] == got[3]
            assert got[1] == [(t1, 0, 15), (t2, 0, 15), (t3, 0, 15)]


def test_w_1_is_the_suffix_array_seeding(ctx):
    rng = random.Random(8)
    text = CO.random_text(rng, 6000, repeat=250, copies=3)
    reads = [CO.mutate(rng, text[a:a + 400], 0.04) for a in range(0, 5600, 700)] + [b"", text[:11], text[-12:]]
    for k, max_occ in [(12, 64), (12, 2), (6, 3)]:
        with ctx.index(text, minimizers=(k, 1)) as ix:
            want = ctx.seed(text, reads, k, max_occ=max_occ)
            assert ix.seed(reads, max_occ) == want == ctx.seed(ix, reads, k, 1, max_occ)
            assert sum(len(a) for a in want) > 100


def ragged():
    if "ragged" not in _cache:
        text, _ = repeat_text()
        rng = random.Random(6)
        reads = []
        for i in range(300):
            ln = rng.choice([0, 5, K - 1, K, 40, 1500]) if i % 10 == 0 else rng.randint(0, 1500)
            at = rng.randrange(0, len(text) - ln + 1)
            reads.append(CO.mutate(rng, text[at:at + ln], rng.choice([0.0, 0.05, 0.1]), alphabet=b"ACGTN" if i % 7 == 0 else b"ACGT"))
        reads[17] = text[0:1500]                         # the longest, and over the repeat unit
        entries = MO.index(text, K, W)
        _cache["ragged"] = reads, entries, MO.seed(text, reads, K, W, entries=entries), [MO.sketch(r, K, W) for r in reads]
    return _cache["ragged"]


@pytest.mark.parametrize("poison", [None, "0xA5"])
@pytest.mark.parametrize("budget", [None, "third", 1])
def test_ranges_give_one_result(ctx, budget, poison):
    text, _ = repeat_text()
    reads, entries, (want, looked), sketches = ragged()
    lens = [len(r) for r in reads]
    worst = [MO.worst_hits(ln, len(entries), K, 64) for ln in lens]
    hits = budget if budget != "third" else sum(worst) // 3
    n_ranges = len(MO.ranges(len(entries), lens, K, 64, hits or 0))
    if budget is None:
        assert n_ranges == 1
    else:
        assert n_ranges >= 3 and (budget != 1 or n_ranges == len([x for x in worst if x]))   # at 1 every read with a k-mer runs alone

    def run(c):
        with c.index(text, minimizers=(K, W)) as ix:
            assert ix.stats["minimizers"] == len(entries)
            got = ix.seed(reads)
            assert got == want and CO.validate(got) == (0, None)
            st = ix.seed_stats
            assert (st["ranges"], st["hits"], st["minimizers"]) == (n_ranges, sum(len(a) for a in want), looked)
            arrays = ix.seed(reads, as_arrays=True)
            assert all(a.dtype == np.uint32 and a.shape == (len(x), 3) for a, x in zip(arrays, want))
            assert [[tuple(x) for x in a.tolist()] for a in arrays] == want
        assert c.sketch(reads, K, W) == sketches           # cut into ranges of sequences by the same budget, over k-mers

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


def test_one_index_many_calls(ctx, pkg):
    text, _ = repeat_text()
    entries = MO.index(text, K, W)
    rng = random.Random(7)
    L = pkg.lib()
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def fetch(ix, cap):
        t, q = np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32), np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32)
        return L.pwa_mm_seed_fetch(ix._ix, u32p(t), u32p(q), cap), t, q

    with ctx.index(text, minimizers=(K, W)) as ix:
        assert fetch(ix, 10)[0] == INVALID                                     # no seeding has run on it
        calls = [([text[a:a + 700] for a in (100, 5000, 20000)] + [CO.mutate(rng, text[9000:9800], 0.05)], 64),
                 ([text[7300:7340], b""], 5),                                   # a smaller call after a larger one
                 ([CO.mutate(rng, text[a:a + 300], 0.02) for a in range(0, 29000, 1500)], 1)]
        for reads, max_occ in calls:
            want = check_seed(ix, reads, max_occ, entries)
            assert ctx.seed_stats == ix.seed_stats
            flat = [a for r in want for a in r]
            rc, t, q = fetch(ix, len(flat))
            assert rc == 0 and list(zip(t.tolist(), q.tolist()))[:len(flat)] == [(a[0], a[1]) for a in flat]
            rc, t, q = fetch(ix, len(flat) + 5)                                 # nothing of an earlier call behind this one's anchors
            assert rc == 0 and set(t[len(flat):].tolist()) == {0xdeadbeef}
            if flat:
                assert fetch(ix, len(flat) - 1)[0] == CAPACITY and fetch(ix, 0)[0] == CAPACITY
            h, p = ix.entries()                                                 # the index itself is untouched by a seeding
            assert list(zip(h.tolist(), p.tolist())) == entries
        # a call that fails validation leaves the stats and the kept anchors; null pointers on a live index
        before = dict(ix.seed_stats)
        off, anc = (C.c_uint64 * 2)(0, 40), (C.c_uint64 * 2)(7, 7)
        assert L.pwa_mm_seed(ix._ix, text[:40], off, 1, 0, anc) == INVALID
        assert L.pwa_mm_seed(ix._ix, text[:40], (C.c_uint64 * 2)(40, 0), 1, 64, anc) == INVALID
        assert L.pwa_mm_seed(ix._ix, text[:40], None, 1, 64, anc) == INVALID
        assert L.pwa_mm_seed(ix._ix, None, off, 1, 64, anc) == INVALID
        assert L.pwa_mm_seed(ix._ix, text[:40], off, 1, 64, None) == INVALID
        assert list(anc) == [7, 7]
        f = [C.c_float(0) for _ in range(3)]
        u = [C.c_uint64(0) for _ in range(4)]
        assert L.pwa_mm_seed_last_stats(ix._ix, *[C.byref(x) for x in f + u]) == 0
        assert dict(zip(("sketch_ms", "search_ms", "sort_ms", "slots", "minimizers", "hits", "ranges"), [x.value for x in f + u])) == before
        assert L.pwa_mm_seed_last_stats(ix._ix, None, None, None, None, None, None, None) == 0
        assert fetch(ix, len(flat))[0] == 0
        hsh, pos = np.zeros(len(entries), dtype=np.uint64), np.zeros(len(entries), dtype=np.uint32)
        assert L.pwa_mm_fetch(ix._ix, hsh.ctypes.data_as(C.POINTER(C.c_uint64)), u32p(pos), len(entries) - 1) == CAPACITY
        with pytest.raises(ValueError):
            ix.seed([b"ACGT"], 0)
        assert ix.seed([]) == [] and fetch(ix, 0)[0] == 0                       # an empty call keeps an empty result
        assert L.pwa_mm_seed_fetch(ix._ix, None, None, 0) == 0
    ix.close()                                                                  # twice is harmless
    with pytest.raises(pkg.PwaError):
        ix.seed([b"ACGT"])
