"""Context.chain (pwa_chain_anchors) on the GPU against chain_oracle.py: f, pred and every result field, whole."""
import random

import pytest

import chain_oracle as CO
from conftest import switched_context

pytestmark = pytest.mark.gpu

COUNTS = [63, 64, 65, 127, 128, 129, 513]
_cache = {}


def check(ctx, reads, fast=False, **params):
    """the call with the whole DP, and without it, against the oracle -> the call's result"""
    want = (CO.chain_many_fast if fast else CO.chain_many)(reads, **params)
    got = ctx.chain(reads, want_dp=True, **params)
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, (r, params, {k: (g[k], w[k]) for k in w if g[k] != w[k] and k not in ("f", "pred")},
                        [(i, a, b) for i, (a, b) in enumerate(zip(g["f"], w["f"])) if a != b][:3],
                        [(i, a, b) for i, (a, b) in enumerate(zip(g["pred"], w["pred"])) if a != b][:3])
    slim = ctx.chain(reads, want_dp=False, **params)
    assert slim == [{k: v for k, v in w.items() if k not in ("f", "pred")} for w in want]
    return got


def test_the_empty_list_and_reads_with_few_anchors(ctx):
    assert ctx.chain([]) == []
    assert ctx.chain_stats == dict(chain_ms=0.0, anchors=0, ranges=0)
    assert ctx.chain([[], []]) == CO.chain_many([[], []], want_dp=False)
    assert ctx.chain_stats["ranges"] == 0
    reads = [[], [(7, 3, 5)], [], [(7, 3, 5), (20, 16, 4)], [(7, 3, 5), (9000, 16, 4)], [], [(0, 0, 1)], []]
    got = check(ctx, reads)
    assert got[0]["last"] is None and got[1]["last"] == 0 and got[3]["count"] == 2 and got[4]["count"] == 1
    assert ctx.chain_stats["anchors"] == 6 and ctx.chain_stats["ranges"] == 1


def block_and_window_inputs(lookback):
    """-> (reads, parameters) of the test below (test_chain_oracle.py shows what these inputs do not reach)"""
    rng = random.Random(lookback)
    reads = [CO.random_anchors(rng, n, span=rng.choice([60, 400]), max_len=12) for n in COUNTS]
    reads += [[(100 + 3 * i, 3 * i, 2) for i in range(n)] for n in (64, 513)]   # every predecessor admissible, f grows along the window
    return reads, dict(lookback=lookback, max_dist=rng.choice([50, 5000]))


@pytest.mark.parametrize("lookback", [1, 63, 64, 65, 128, 512])
def test_anchor_counts_around_the_block_and_the_window(ctx, lookback):
    """63 .. 513 anchors (a block of the kernel is 64) against windows of 1 .. 512 (a chunk is 64), n < H included; the anchors sit
    densely around one diagonal, so that every window is full of admissible predecessors"""
    reads, params = block_and_window_inputs(lookback)
    got = check(ctx, reads, **params)
    assert max(g["count"] for g in got) > 20


def test_diagonals_gaps_and_overlaps(ctx):
    diag = [(100 + 20 * i, 20 * i, 15) for i in range(150)]
    got = check(ctx, [diag, [(100 + i, i, 15) for i in range(150)], [(5, 5, 3)] * 70 + [(9, 9, 3)] * 3])
    assert got[0]["score"] == 15 * 150 and got[0]["count"] == 150 and (got[0]["diag_lo"], got[0]["diag_hi"]) == (100, 100)
    assert got[1]["score"] == 15 + 149 and got[1]["count"] == 150          # overlapping anchors: dx < len
    assert got[2]["score"] == 6 and got[2]["pred"][70:] == [69, 69, 69]    # duplicates never chain to each other
    bw, md = 7, 90
    two = lambda dd: [(100, 100, 10), (200 + dd, 200, 10)]
    got = check(ctx, [two(bw), two(bw + 1), two(-bw), two(-bw - 1)], bandwidth=bw, gap_scale=0)
    assert [g["count"] for g in got] == [2, 1, 2, 1]
    gap = lambda d: [(0, 0, 5), (d, d, 5)]
    got = check(ctx, [gap(md), gap(md + 1), [(0, 0, 5), (md, 50, 5)], [(0, 0, 5), (md + 1, 50, 5)], [(0, 0, 5), (50, md + 1, 5)]], max_dist=md,
                bandwidth=500, gap_scale=0)
    assert [g["count"] for g in got] == [2, 1, 2, 1, 1]


@pytest.mark.parametrize("gap_scale", [0, 1024])
def test_gap_scale_limits(ctx, gap_scale):
    rng = random.Random(gap_scale + 1)
    check(ctx, [CO.random_anchors(rng, n, span=300, max_len=25) for n in (5, 70, 200)], gap_scale=gap_scale)
    big = [(0, 0, 40), ((1 << 20) + 1000, 1000, 40)]   # dd = 2^20: beta = 10 at gap_scale 0, 4 * 2^20 + 10 at 1024
    got = check(ctx, [big], gap_scale=gap_scale, bandwidth=1 << 20, max_dist=1 << 30)
    assert got[0]["count"] == (2 if gap_scale == 0 else 1)


def test_dd_at_the_powers_of_two(ctx):
    reads = []
    for e in range(21):
        for dd in {(1 << e) - 1, 1 << e, (1 << e) + 1} - {0}:
            if dd <= 1 << 20:
                reads.append([(0, 0, 40), (100 + dd, 100, 40)])
                reads.append([(0, 0, 40), (100, 100 + dd, 40)])
    for gs in (1, 38):
        got = check(ctx, reads, bandwidth=1 << 20, max_dist=1 << 30, gap_scale=gs)
        assert {g["count"] for g in got} == {1, 2}


def test_the_three_ties(ctx):
    got = check(ctx, [[(10, 10, 5), (10, 10, 5), (20, 20, 5)]])
    assert got[0]["pred"] == [-1, -1, 1]                                  # the largest j wins
    got = check(ctx, [[(0, 0, 5), (9, 5, 10)], [(0, 0, 6), (10, 6, 10)]], gap_scale=256)
    assert got[0]["pred"] == [-1, -1] and got[1]["pred"] == [-1, 0]       # cand == len_i keeps pred = -1
    got = check(ctx, [[(10, 10, 7), (5000, 40, 7), (9000, 90, 7)]], max_dist=100)
    assert got[0]["last"] == 0                                            # the smallest e wins
    tie = [(10 + 5 * (i % 64), 10 + 5 * (i % 64), 5) for i in range(64)] * 2   # equal cand in every lane of a later block
    tie.sort(key=lambda a: (a[0] + a[2], a[1] + a[2]))
    check(ctx, [tie], lookback=128)


def ragged():
    """about 300 planted reads of 0 .. 3300 symbols, seeded by the oracle's seeder: 0 .. about 3000 anchors each"""
    if "ragged" not in _cache:
        rng = random.Random(23)
        text = CO.random_text(rng, 40000, repeat=500, copies=3)
        index = CO.kmer_index(text, 12)
        reads = [[] for _ in range(3)]
        for i in range(297):
            ln = [0, 5, 12, 40][i] if i < 4 else rng.randint(100, 3300)
            at = rng.randrange(0, len(text) - ln + 1)
            reads.append(CO.seed(index, CO.mutate(rng, text[at:at + ln], rng.choice([0.0, 0.03, 0.08])), 12))
        rng.shuffle(reads)
        _cache["ragged"] = reads, CO.chain_many_fast(reads)
    return _cache["ragged"]


def test_a_ragged_list_in_ranges_and_over_poisoned_buffers(ctx):
    reads, want = ragged()
    counts = [len(a) for a in reads]
    assert min(counts) == 0 and max(counts) > 2500 and sum(counts) > 100000
    plain = ctx.chain(reads, want_dp=True)
    for r, (g, w) in enumerate(zip(plain, want)):
        assert g == w, (r, counts[r], {k: (g[k], w[k]) for k in w if g[k] != w[k] and k not in ("f", "pred")})
    assert ctx.chain_stats["ranges"] == 1 and ctx.chain_stats["anchors"] == sum(counts) and ctx.chain_stats["chain_ms"] > 0
    assert ctx.chain(reads) == [{k: v for k, v in w.items() if k not in ("f", "pred")} for w in want]
    budget = (CO.ANCHOR_BYTES * sum(counts) + CO.RECORD_BYTES * len(counts)) // 5
    n_ranges = len(CO.ranges(counts, budget))
    assert n_ranges >= 3 and budget >= 4096
    with switched_context(PWA_RANGE_BYTES=budget) as c:
        assert c.chain(reads, want_dp=True) == plain
        assert c.chain_stats["ranges"] == n_ranges and c.chain_stats["anchors"] == sum(counts)
    for byte in ("0xA5", "0"):
        with switched_context(PWA_POISON=byte) as c:
            assert c.chain(reads, want_dp=True) == plain
            assert c.chain(reads) == ctx.chain(reads)
            assert c.poison_stats()["buffers"] > 0
        with switched_context(PWA_POISON=byte, PWA_RANGE_BYTES=budget) as c:
            assert c.chain(reads, want_dp=True) == plain
            assert c.chain_stats["ranges"] == n_ranges


def far_case(name):
    return next(c for c in CO.far_cases() if c["name"] == name)


def hold(label, g, H):
    """what the builder of a far-window read promises (chain_oracle.py), asserted on the call's own result: a mistake that the kernel
    and the oracle share would still show here"""
    kind, n = label[0], len(g["pred"])
    top = (g["score"], g["count"], g["last"])
    if kind == "far":
        d = label[1]
        assert g["pred"] == [-1] * d + [0 if d <= H else -1], label
        assert g["f"] == [10] + [1] * (d - 1) + [20 if d <= H else 10], label
        assert top == ((20, 2, d) if d <= H else (10, 1, 0)), label
    elif kind == "equal":
        d = label[1]
        assert g["pred"] == [-1] * (d + 1) and g["f"][-1] == 20 and top == (20, 1, d), label
    elif kind == "ladder":
        d = label[1]
        assert n == label[2]
        if d <= H:
            assert g["pred"] == [i - d if i >= d else -1 for i in range(n)], label
            assert g["f"] == [5 * (i // d + 1) for i in range(n)], label
            assert top == (5 * ((n - 1) // d + 1), (n - 1) // d + 1, d * ((n - 1) // d)), label
            if n == 2 * d + 70 and d >= 70:
                assert top == (15, 3, 2 * d), label
        else:
            assert g["pred"] == [-1] * n and top == (5, 1, 0), label
        assert g["diag_lo"] == g["diag_hi"] == 4000, label   # one rung is one diagonal, and every chain found ends on rung 0
    elif kind == "tie":
        o1, o2, far_len = label[1:]
        assert n == o2 + 2 and H > o2
        assert g["pred"] == [-1] * (n - 1) + [n - 2 - (o1 if far_len == 10 else o2)], label
        assert g["f"][-1] == 10 + far_len and top == (10 + far_len, 2, n - 1), label
    elif kind == "tail":
        assert top == (500, 100, 1199) and g["pred"][1100] == -1 and g["diag_lo"] == g["diag_hi"] == 30000, label
    else:
        assert kind == "few" and n <= 1


def run_case(ctx, c):
    got = check(ctx, c["reads"], fast=True, **c["params"])
    for label, g in zip(c["labels"], got):
        hold(label, g, c["params"]["lookback"])
    return got


@pytest.mark.parametrize("lookback", CO.EDGE_LOOKBACKS)
def test_the_deciding_predecessor_at_both_edges_of_the_window(ctx, lookback):
    """the one predecessor that counts at offset 0, H - 2, H - 1 (the window's last slot) and H (one beyond it), for H on both sides of
    every threshold between chain_kernel<1>, <2>, <4> and <8>: as a single link (far), along a whole read (ladder, whose walk then
    hops by that distance), and with a cand that only equals len (equal)"""
    c = far_case("edges-%d" % lookback)
    assert {l[1] for l in c["labels"]} == {d for d in (1, lookback - 1, lookback, lookback + 1) if d >= 1}
    run_case(ctx, c)


def test_walks_that_skip_whole_blocks_and_one_that_stays_in_its_tail(ctx):
    """hops of 64, 65, 200 and 512 anchors, five in a row: the walk leaves its block of 64 pred words with every hop and lands in an
    earlier one at lane 0, 63, 62, ... of it; and a read whose best chain is its last 100 anchors, behind a ladder it must not enter"""
    c = far_case("walk")
    got = run_case(ctx, c)
    assert [g["count"] for g in got[:-1]] == [6, 6, 6, 6] and all(g["count"] >= 5 for g in got)
    assert [g["last"] for g in got[:-1]] == [5 * d for d in CO.WALK_HOPS]


def test_ties_between_two_lanes_of_the_key_maximum(ctx):
    """two admissible predecessors and no third, in one quad, in two quads of a row, in two rows, in two chunks: equal cand (the
    nearer, the larger j, wins) and the farther better by one; at lookback 512, and with the farther one in the window's last slot"""
    run_case(ctx, far_case("ties"))
    kernels = []
    for c in CO.far_cases():
        if c["name"].startswith("ties-"):
            assert {o2 + 1 for _, _, o2, _ in c["labels"]} == {c["params"]["lookback"]}
            kernels.append(CO.chunks_of(c["params"]["lookback"]))
            run_case(ctx, c)
    assert kernels == sorted(kernels) and set(kernels) == {1, 2, 4, 8}


def test_the_far_window_reads_in_mixed_order_in_ranges_and_over_poisoned_buffers(ctx):
    """every read of the three tests above in one call, shuffled among empty and one-anchor reads; again with a budget that the
    longest read alone exceeds (the planner's arm "one read that alone exceeds it"), and again over poisoned buffers"""
    c = far_case("mixed")
    reads, params = c["reads"], c["params"]
    counts = [len(a) for a in reads]
    assert counts.count(0) > 10 and counts.count(1) > 10 and len(reads) - c["labels"].count(("few",)) == len(set(c["labels"])) - 1
    plain = run_case(ctx, c)
    weight = lambda r: CO.ANCHOR_BYTES * counts[r] + CO.RECORD_BYTES
    budget = max(weight(r) for r in range(len(reads))) // 2
    cut = CO.ranges(counts, budget)
    assert budget >= 4096 and any(k1 - k0 == 1 and weight(k0) > budget for k0, k1 in cut) and len(cut) > 10
    with switched_context(PWA_RANGE_BYTES=budget) as k:
        assert k.chain(reads, want_dp=True, **params) == plain
        assert k.chain_stats["ranges"] == len(cut) and k.chain_stats["anchors"] == sum(counts)
    with switched_context(PWA_POISON="0xA5") as k:
        assert k.chain(reads, want_dp=True, **params) == plain
        assert k.poison_stats()["buffers"] > 0


@pytest.mark.parametrize("lookback", [200, 512])
def test_seeded_reads_on_a_text_with_eight_copies_of_a_unit(ctx, lookback):
    """a real seeded list whose anchors are dense enough that predecessors beyond offset 127 win (test_chain_oracle.py: ignoring them
    changes this list's result), through chain_kernel<4> and <8>"""
    got = check(ctx, CO.repeat_reads(), fast=True, lookback=lookback)
    assert max(i - p for g in got for i, p in enumerate(g["pred"]) if p >= 0) > 128


def test_validation_matches_the_plan(ctx, pkg):
    top = (1 << 31) - 1
    good = [(5, 5, 3), (9, 9, 3)]
    for reads, params in [([good, [(5, 5, 0)]], {}), ([[(9, 9, 3), (5, 5, 3)]], {}), ([good, [(top, 0, 1)]], {}),
                          ([[(0, 0, 1 << 29), (1 << 29, 1 << 29, 1 << 29)]], {}), ([good], dict(lookback=0)), ([good], dict(lookback=513)),
                          ([good], dict(max_dist=0)), ([good], dict(bandwidth=(1 << 20) + 1)), ([good], dict(gap_scale=1025)),
                          ([[(5, 5, 0)], [(top, 0, 1)]], {}), ([[(top, 0, 1)], [(5, 5, 0)]], {})]:
        plan = pkg.chain_plan(reads, **params)
        assert plan["code"] in (CO.INVALID, CO.CAPACITY)
        with pytest.raises(pkg.PwaError) as e:
            ctx.chain(reads, **params)
        assert pkg.lib().pwa_strerror(plan["code"]).decode() in str(e.value)
        if plan["bad_read"] is not None:
            assert "read %d:" % plan["bad_read"] in str(e.value)
    for reads in ([good, [(top - 1, 0, 1)]], [[(0, 0, 1 << 29), (1 << 29, 1 << 29, (1 << 29) - 1)]]):
        assert pkg.chain_plan(reads)["code"] == 0
        check(ctx, reads, max_dist=1 << 30, bandwidth=1 << 20)
