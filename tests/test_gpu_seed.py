"""pwa_sa_seed on the GPU (Context.index, TextIndex.seed, and Context.seed / map_reads over them): every result whole against
chain_oracle's seeder over a dict of k-mers, and through chain_oracle.validate, at the edges of the 8-byte compare, of the text, of the
read blob, of max_occ, of the sort, of the blocks and tiles, of the ranges, and over the reuse of one index."""
import ctypes as C
import random

import numpy as np
import pytest

import chain_oracle as CO
import seed_oracle as SO
from conftest import switched_context

pytestmark = pytest.mark.gpu

K = 13
INVALID, CAPACITY = -1, -5
_cache = {}


def repeat_text():
    """30 kb with a 400-base unit in five copies (test_gpu_map_reads.planted()'s text), and its 13-mer dictionary"""
    if "repeat" not in _cache:
        text = CO.random_text(random.Random(41), 30000, repeat=400, copies=5)
        _cache["repeat"] = text, CO.kmer_index(text, K)
    return _cache["repeat"]


def check(index, reads, k, step=1, max_occ=64, kmers=None):
    """index.seed against the oracle, whole, with the call's stats; -> the anchors"""
    want = SO.seed(index.text, reads, k, step, max_occ, index=kmers)
    got = index.seed(reads, k, step, max_occ)
    assert got == want, (k, step, max_occ)
    assert CO.validate(got) == (0, None)
    st = index.seed_stats
    assert st["hits"] == sum(len(a) for a in want) and st["slots"] == sum(SO.slots(len(r), k, step) for r in reads)
    assert st["ranges"] == len(SO.ranges(len(index.text), [len(r) for r in reads], k, step, max_occ))
    return got


def test_word_edges_of_the_compare(ctx):
    rng = random.Random(1)
    text = CO.random_text(rng, 1003)                      # not a multiple of 8: the last words of the text are partial
    assert len(text) % 8 == 3
    with ctx.index(text) as ix:
        for k in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65):
            # step 1 and reads cut at every offset mod 8, of lengths that move the next read through every alignment in the blob
            reads = [text[100 + a:100 + a + k + 11 + a] for a in range(8)]
            reads += [CO.mutate(rng, text[300 + 7 * a:300 + 7 * a + 2 * k + 9], 0.05) for a in range(8)]
            # a k-mer that differs from the text's in its last byte only, and in its first byte only
            last, first = bytearray(text[500:500 + k]), bytearray(text[600:600 + k])
            last[-1] ^= 2
            first[0] ^= 2
            reads += [bytes(last), bytes(first), text[-k:], text[:k]]
            got = check(ix, reads, k)
            assert k == 1 or ((len(text) - k, 0, k) in got[-2] and (0, 0, k) in got[-1])   # (at k = 1 every symbol occurs more than 64 times)
            if k >= 15:
                assert got[-4] == [] and got[-3] == [] and all(len(a) >= 10 for a in got[:8])
        assert sum(len(a) for a in check(ix, reads, 1, max_occ=400)) > 1000    # k = 1 with every slot kept: about a quarter of the text each


def test_text_end(ctx):
    rng = random.Random(2)
    text = CO.random_text(rng, 1003)
    n, k = len(text), 12
    with ctx.index(text) as ix:
        tails = [text[-(k - j):] + b"\0" * j for j in (1, 2, 3, 8)]   # the text's tail, then what the padded device text holds past its end
        reads = [text[-k:], text[-k - 1:], text[-k + 1:]] + tails + [text[-(k - 1):] + b"A", text[-30:] + b"\0\0"]
        got = check(ix, reads, k)
        assert got[0] == [(n - k, 0, k)] and got[1] == [(n - k - 1, 0, k), (n - k, 1, k)] and got[2] == []
        assert all(g == [] for g in got[3:8])
        assert got[8] == [(n - 30 + q, q, k) for q in range(30 - k + 1)]     # and nothing at q = 19, 20: those k-mers run past n
    with ctx.index(b"ACGTACGTACG") as ix:                                    # n = 11
        assert check(ix, [b"ACGTACGTACGT", b"ACGTACGTACG", b"CGTACGTACG"], 12) == [[], [], []]    # n < k
        assert ix.seed_stats == dict(search_ms=0.0, sort_ms=0.0, slots=1, hits=0, ranges=0)
        assert check(ix, [b"ACGTACGTACGT", b"ACGTACGTACG", b"CGTACGTACG"], 11) == [[(0, 0, 11)], [(0, 0, 11)], []]   # n = k
    with ctx.index(b"") as ix:
        assert check(ix, [b"A", b""], 1) == [[], []]


def test_blob_end_and_reads_without_slots(ctx):
    text, kmers = repeat_text()
    with ctx.index(text) as ix:
        t = lambda a, ln: text[a:a + ln]
        reads = [b"", t(5000, K - 1), t(6000, K), b"", b"", t(7000, K + 1), t(8000, 3), t(9000, 200), b"", t(10000, K)]
        got = check(ix, reads, K, kmers=kmers)
        assert [len(a) for a in got] == [0, 0, 1, 0, 0, 2, 0, 188, 0, 1]
        assert got[-1] == [(10000, 0, K)]                                     # the last k-mer ends on the blob's last byte
        assert check(ix, reads + [b""], K, kmers=kmers)[-2] == [(10000, 0, K)]
        assert check(ix, [t(11000, 40)], K, kmers=kmers)[0][-1] == (11027, 27, K)   # one read: its last k-mer ends the blob
        assert check(ix, reads, K, step=1000, kmers=kmers)[7] == [(9000, 0, K)]      # a step larger than the read: the slot at q = 0 alone
        assert check(ix, reads, K, step=187, kmers=kmers)[7] == [(9000, 0, K), (9187, 187, K)]
        assert check(ix, [], K) == [] and ix.seed_stats["ranges"] == 0
        assert check(ix, [b"", t(1, 5), b""], K) == [[], [], []] and ix.seed_stats["ranges"] == 0


def test_raw_bytes_and_a_single_symbol_text(ctx):
    rng = random.Random(3)
    text = bytes(rng.choice(b"\x00\x01\x7f\x80\xffA") for _ in range(2001))
    with ctx.index(text) as ix:
        reads = [text[a:a + 60] for a in (0, 333, 1941)] + [CO.mutate(rng, text[700:800], 0.1, alphabet=b"\x00\x80\xff"), b"\x00" * 20, b"\x80\xff" * 9]
        for k, max_occ in [(1, 2001), (1, 64), (3, 64), (4, 9), (8, 64), (9, 64)]:
            got = check(ix, reads, k, max_occ=max_occ)
        assert len(got[0]) >= 52 and len(got[2]) >= 52
    a300 = b"A" * 300
    with ctx.index(a300) as ix:
        reads = [b"A" * 20, a300, b"AB", b"A" * 8]
        assert len(check(ix, reads, 8, max_occ=293)[3]) == 293       # 293 occurrences, at the limit
        assert check(ix, reads, 8, max_occ=292) == [[], [], [], []]   # ... and one above it
        assert len(check(ix, reads, 1, max_occ=300)[2]) == 300
        assert check(ix, reads, 300)[1] == [(0, 0, 300)]
        assert [len(a) for a in check(ix, reads, 200, max_occ=101)] == [0, 101 * 101, 0, 0]


def test_max_occ_at_and_around_a_slots_count(ctx):
    text, kmers = repeat_text()
    unit = sorted(len(kmers[text[q:q + K]]) for q in range(400 - K + 1))
    assert unit[0] == 5 and unit[-1] == 6
    rng = random.Random(4)
    reads = [text[0:400], text[100:900], text[29000:], CO.mutate(rng, text[0:400], 0.03), text[7300:7900]]
    with ctx.index(text) as ix:
        sizes = {}
        for max_occ in (1, 4, 5, 6, 64):
            got = check(ix, reads, K, max_occ=max_occ, kmers=kmers)
            sizes[max_occ] = len(got[0])
        assert sizes[1] == sizes[4] == 0 and sizes[5] == 5 * unit.count(5) and sizes[6] == sizes[64] == sizes[5] + 6 * unit.count(6)
    # the largest k-mer of the text three times, as the last three suffixes: the probe sa[lo + max_occ] inside the array (dropped), on n, past n
    text2 = text[:1002] + b"T" * (K + 2) + text[1002:29000] + b"A"
    kmers2 = CO.kmer_index(text2, K)
    top = b"T" * K
    assert max(kmers2) == top and kmers2[top] == [1002, 1003, 1004]
    with ctx.index(text2) as ix:
        for max_occ, n_hits in [(2, 0), (3, 3), (4, 3), (1, 0), (0xffffffff, 3)]:
            got = check(ix, [top, text2[990:1030]], K, max_occ=max_occ, kmers=kmers2)
            assert len(got[0]) == n_hits
        # ... and the smallest, the first suffixes (lo = 0)
        low = min(kmers2)
        for max_occ in (len(kmers2[low]) - 1, len(kmers2[low]), len(kmers2[low]) + 1):
            if max_occ:
                check(ix, [low], K, max_occ=max_occ, kmers=kmers2)


def test_order_is_t_then_q_and_the_sort_is_stable(ctx):
    rng = random.Random(5)
    x = b"GATTACAGATTACCA"                       # 15 symbols, no proper overlap with itself at k = 15
    fill = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    # x stands between symbols of its own in the text (N) and in the read (R): no k-mer that only overlaps x can hit
    text = fill(300) + b"N" + x + b"N" + fill(410) + b"N" + x + b"N" + fill(76) + b"N" + x + b"N" + fill(200)
    t1, t2, t3 = 301, 301 + 16 + 411, 301 + 16 + 411 + 16 + 77
    read = x + b"R" + fill(7) + b"R" + x + b"R" + fill(28) + b"R" + x
    q1, q2, q3 = 0, 24, 69
    with ctx.index(text) as ix:
        got = check(ix, [read, x], 15)
        assert got[0] == [(t, q, 15) for t in (t1, t2, t3) for q in (q1, q2, q3)] and got[1] == [(t1, 0, 15), (t2, 0, 15), (t3, 0, 15)]
        assert check(ix, [read], 15, step=3)[0] == [(t, q, 15) for t in (t1, t2, t3) for q in (q1, q2, q3)]
    # every hit at one t: no digit of t varies; with one read no digit at all, with several only the read's
    once = fill(500) + b"N" + x + b"N" + fill(500)
    with ctx.index(once) as ix:
        assert check(ix, [read], 15)[0] == [(501, q, 15) for q in (q1, q2, q3)]
        assert check(ix, [read, x, fill(40), read], 15) == [[(501, q, 15) for q in (q1, q2, q3)], [(501, 0, 15)], [], [(501, q, 15) for q in (q1, q2, q3)]]
        assert check(ix, [fill(40), x + b"R"], 15) == [[], [(501, 0, 15)]]     # a single hit in all
        assert ix.seed_stats["hits"] == 1 and ix.seed_stats["ranges"] == 1


@pytest.fixture(scope="module")
def repeat_index(ctx):
    with ctx.index(repeat_text()[0]) as ix:
        yield ix


@pytest.mark.parametrize("target", [255, 256, 257, 4095, 4096, 4097])
def test_block_and_tile_edges(repeat_index, target):
    text, kmers = repeat_text()
    ix = repeat_index
    # total slots: one read, and the same slots over three reads and an empty one
    one = text[3000:3000 + target + K - 1]
    assert ix.seed([one], K) == SO.seed(text, [one], K, index=kmers) and ix.seed_stats["slots"] == target
    a, b = target // 3, target // 2
    reads = [text[3000:3000 + a + K - 1], b"", text[9000:9000 + (b - a) + K - 1], text[15000:15000 + (target - b) + K - 1]]
    check(ix, reads, K, kmers=kmers)
    assert ix.seed_stats["slots"] == target
    # total hits: a read that leaves the second copy of the repeat unit, whose k-mers hit five times each (those that hit six times are
    # dropped by max_occ = 5), into text that hits once, cut where the total is the target
    assert text[7400:7800] == text[0:400]
    start = 7400 + 400 - K - 40
    total, end = 0, None
    for q in range(0, 6000):
        c = len(kmers[text[start + q:start + q + K]])
        total += c if c <= 5 else 0
        if total >= target:
            end = start + q + K
            break
    assert total == target and end is not None
    got = check(ix, [text[start:end]], K, max_occ=5, kmers=kmers)
    assert len(got[0]) == target and ix.seed_stats["hits"] == target


def ragged_reads():
    if "ragged" not in _cache:
        text, kmers = repeat_text()
        rng = random.Random(6)
        reads = []
        for i in range(300):
            ln = rng.choice([0, 5, K - 1, K, 40, 1500]) if i % 10 == 0 else rng.randint(0, 1500)
            at = rng.randrange(0, len(text) - ln + 1)
            reads.append(CO.mutate(rng, text[at:at + ln], rng.choice([0.0, 0.05, 0.1])))
        reads[17] = text[0:1500]                         # the longest, and over the repeat unit
        _cache["ragged"] = reads, SO.seed(text, reads, K, index=kmers)
    return _cache["ragged"]


@pytest.mark.parametrize("poison", [None, "0xA5"])
@pytest.mark.parametrize("budget", [None, "third", 50000, 1])
def test_ranges_give_one_result(ctx, budget, poison):
    text, _ = repeat_text()
    reads, want = ragged_reads()
    lens = [len(r) for r in reads]
    worst = [SO.worst_hits(ln, len(text), K, 1, 64) for ln in lens]
    assert max(worst) > 50000                          # the longest read alone exceeds that budget
    hits = budget if budget != "third" else sum(worst) // 3
    n_ranges = len(SO.ranges(len(text), lens, K, 1, 64, hits or 0))
    if budget is None:
        assert n_ranges == 1
    else:
        assert n_ranges >= 3 and (budget != 1 or n_ranges == len([w for w in worst if w]))   # at 1 every read with a slot runs alone

    def run(c):
        with c.index(text) as ix:
            got = ix.seed(reads, K)
            assert got == want
            assert ix.seed_stats["ranges"] == n_ranges and ix.seed_stats["hits"] == sum(len(a) for a in want)
            arrays = ix.seed(reads, K, as_arrays=True)
            assert all(a.dtype == np.uint32 and a.shape == (len(w), 3) for a, w in zip(arrays, want))
            assert [[tuple(x) for x in a.tolist()] for a in arrays] == want

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
    text, kmers = repeat_text()
    rng = random.Random(7)
    L = pkg.lib()
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def fetch(ix, cap):
        t, q = np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32), np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32)
        return L.pwa_sa_seed_fetch(ix._ix, u32p(t), u32p(q), cap), t, q

    with ctx.index(text) as ix:
        assert ix.stats["rounds"] >= 2 and ix.stats["build_ms"] > 0 and ix.text == text
        assert fetch(ix, 10)[0] == INVALID                                     # no seeding has run on it
        calls = [([text[a:a + 700] for a in (100, 5000, 20000)] + [CO.mutate(rng, text[9000:9800], 0.05)], 13, 1, 64),
                 ([text[7300:7340], b""], 11, 3, 5),                            # a smaller call after a larger one
                 ([CO.mutate(rng, text[a:a + 300], 0.02) for a in range(0, 29000, 1500)], 15, 2, 1)]
        for reads, k, step, max_occ in calls:
            want = SO.seed(text, reads, k, step, max_occ)
            assert ix.seed(reads, k, step, max_occ) == want and ctx.seed_stats == ix.seed_stats
            flat = [a for r in want for a in r]
            rc, t, q = fetch(ix, len(flat))
            assert rc == 0 and list(zip(t.tolist(), q.tolist()))[:len(flat)] == [(a[0], a[1]) for a in flat]
            rc, t, q = fetch(ix, len(flat) + 5)                                 # nothing of an earlier call behind this one's anchors
            assert rc == 0 and set(t[len(flat):].tolist()) == {0xdeadbeef}
            if flat:
                assert fetch(ix, len(flat) - 1)[0] == CAPACITY and fetch(ix, 0)[0] == CAPACITY
            assert ctx.seed(text, reads, k, step, max_occ) == want == ctx.seed(ix, reads, k, step, max_occ)
            arrays = ctx.seed(text, reads, k, step, max_occ, as_arrays=True)
            assert [[tuple(x) for x in a.tolist()] for a in arrays] == want
        # a call that fails validation leaves the stats and the kept anchors; null pointers on a live index
        before = dict(ix.seed_stats)
        off, anc = (C.c_uint64 * 2)(0, 40), (C.c_uint64 * 2)(7, 7)
        assert L.pwa_sa_seed(ix._ix, text[:40], off, 1, 0, 1, 64, anc) == INVALID
        assert L.pwa_sa_seed(ix._ix, text[:40], (C.c_uint64 * 2)(40, 0), 1, 13, 1, 64, anc) == INVALID
        assert L.pwa_sa_seed(ix._ix, text[:40], None, 1, 13, 1, 64, anc) == INVALID
        assert L.pwa_sa_seed(ix._ix, None, off, 1, 13, 1, 64, anc) == INVALID
        assert L.pwa_sa_seed(ix._ix, text[:40], off, 1, 13, 1, 64, None) == INVALID
        assert list(anc) == [7, 7]
        sm, om, a, b, c = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert L.pwa_sa_seed_last_stats(ix._ix, C.byref(sm), C.byref(om), C.byref(a), C.byref(b), C.byref(c)) == 0
        assert dict(search_ms=sm.value, sort_ms=om.value, slots=a.value, hits=b.value, ranges=c.value) == before
        assert L.pwa_sa_seed_last_stats(ix._ix, None, None, None, None, None) == 0
        assert fetch(ix, len(flat))[0] == 0
        with pytest.raises(ValueError):
            ix.seed([b"ACGT"], 0)
        # an empty call keeps an empty result
        assert ix.seed([], 13) == [] and fetch(ix, 0)[0] == 0
        assert L.pwa_sa_seed_fetch(ix._ix, None, None, 0) == 0
    ix.close()                                                                  # twice is harmless
    with pytest.raises(pkg.PwaError):
        ix.seed([b"ACGT"], 2)


def test_chain_and_map_reads_on_an_index(ctx):
    import test_gpu_map_reads as MR
    text, planted = MR.planted()
    reads = [r for r, _, _ in planted[:16]]
    with ctx.index(text) as ix:
        arrays = ix.seed(reads, MR.K, as_arrays=True)
        tuples = ix.seed(reads, MR.K)
        chains = ctx.chain(arrays)                                              # as they come: no re-ordering in between
        assert chains == ctx.chain(tuples) and ctx.chain_stats["anchors"] == sum(len(a) for a in tuples)
        assert [c["score"] for c in chains] == [CO.chain(a, want_dp=False)["score"] for a in tuples]
        on_index = ctx.map_reads(ix, reads, MR.K, *MR.SC, w=MR.W, both_strands=True)
        assert set(ctx.map_stats) == {"seed_s", "chain_s", "align_s"}
        assert on_index == ctx.map_reads(text, reads, MR.K, *MR.SC, w=MR.W, both_strands=True)
        assert all(g is not None for g in on_index)
        assert ctx.map_reads(ix, reads, MR.K, *MR.SC, w=MR.W) == ctx.map_reads(text, reads, MR.K, *MR.SC, w=MR.W)
