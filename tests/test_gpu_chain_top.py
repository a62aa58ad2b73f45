"""Context.chain_top (pwa_chain_top) on the GPU against chain_top_oracle.py: every output whole -- the chain records, the number of
chains, mapq, chain_id, f, pred, and the rounds of the stats."""
import random
import time

import pytest

import chain_oracle as CO
import chain_top_oracle as TO
from conftest import switched_context
from test_gpu_chain import COUNTS, ragged

pytestmark = pytest.mark.gpu

_cache = {}
LOW = dict(max_chains=16, min_score=12, min_count=1)   # every seed of the ragged reads is a candidate: up to 14 chains and 1 .. 40 rounds a read


def compare(got, want, stats, what=""):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        w = {k: v for k, v in w.items() if k != "rounds"}
        assert g == w, (what, r, [(k, g[k], w[k]) for k in ("chains", "mapq") if g[k] != w[k]],
                        [(i, a, b) for k in ("f", "pred", "chain_id") for i, (a, b) in enumerate(zip(g[k], w[k])) if a != b][:4])
    assert stats["rounds"] == sum(w["rounds"] for w in want), what
    assert stats["anchors"] == sum(len(w["f"]) for w in want)


def check(ctx, reads, fast=False, **params):
    """the call with every optional output, and without them, against the oracle -> the call's result"""
    want = (TO.chain_top_many_fast if fast else TO.chain_top_many)(reads, **params)
    got = ctx.chain_top(reads, want_dp=True, want_ids=True, **params)
    compare(got, want, ctx.chain_top_stats, params)
    slim = ctx.chain_top(reads, **params)
    assert slim == [dict(chains=w["chains"], mapq=w["mapq"]) for w in want]
    return got


def test_the_empty_list_and_reads_with_few_anchors(ctx):
    assert ctx.chain_top([]) == []
    assert ctx.chain_top_stats == dict(chain_ms=0.0, top_ms=0.0, anchors=0, rounds=0, ranges=0)
    assert ctx.chain_top([[], []]) == [dict(chains=[], mapq=0)] * 2
    assert ctx.chain_top_stats["ranges"] == 0
    reads = [[], [(7, 3, 5)], [], [(7, 3, 5), (20, 16, 4)], [(7, 3, 5), (9000, 16, 4)], [], [(0, 0, 1)], []]
    got = check(ctx, reads, min_score=1, min_count=1)
    assert [len(g["chains"]) for g in got] == [0, 1, 0, 1, 2, 0, 1, 0]
    assert ctx.chain_top_stats["anchors"] == 6 and ctx.chain_top_stats["ranges"] == 1 and ctx.chain_top_stats["rounds"] == 5
    check(ctx, reads, min_score=5, min_count=1, max_chains=1)
    check(ctx, reads)


@pytest.mark.parametrize("lookback", [1, 64, 65, 512])
def test_anchor_counts_around_the_block_and_the_window(ctx, lookback):
    rng = random.Random(lookback)
    reads = [CO.random_anchors(rng, n, span=rng.choice([60, 400]), max_len=12) for n in COUNTS]
    reads += [[(100 + 3 * i, 3 * i, 2) for i in range(n)] for n in (64, 513)]
    for params in (dict(min_score=1, min_count=1, max_chains=16), dict(min_score=8, min_count=2, max_chains=4),
                   dict(min_score=8, min_count=2, max_chains=4, rooted=True), dict(min_score=3, min_count=3, max_chains=1)):
        got = check(ctx, reads, lookback=lookback, **params)
    assert max(len(g["chains"]) for g in got) == 1


def test_the_built_cases(ctx):
    """fork, orphan_branch, equal_f (the tied ends in one block of 64, adjacent blocks, far blocks), isolated, a walk that stops at a
    marked anchor in lane 0 and lane 63 of an earlier block, N = 16 of 20 keepable chains, min_score and min_count met exactly and
    missed by one, ROOTED on and off: each as a read of its own call, then all in one call per parameter set"""
    cases = TO.built_cases()
    by_params = {}
    for name, anchors, params in cases:
        by_params.setdefault(tuple(sorted(params.items())), []).append(anchors)
    assert len(by_params) > 10
    for key, reads in by_params.items():
        check(ctx, reads, **dict(key))
    many = check(ctx, [TO.many_chains(20)], min_score=20, min_count=3, max_chains=16)[0]
    assert len(many["chains"]) == 16 and many["mapq"] == 0
    f = check(ctx, [TO.fork(), TO.fork(70)], min_score=10, min_count=1)
    assert [c["branch"] for c in f[0]["chains"]] == [-1, 1] and [c["branch"] for c in f[1]["chains"]] == [-1, 71]
    f = check(ctx, [TO.fork(), TO.fork(70)], min_score=10, min_count=1, rooted=True)
    assert [len(g["chains"]) for g in f] == [1, 1] and ctx.chain_top_stats["rounds"] == 4


def test_one_chain_equals_the_chain_call(ctx):
    """N = 1 at min_score = min_count = 1 against pwa_chain_anchors on the ragged reads, all fields"""
    reads, want = ragged()
    got = ctx.chain_top(reads, max_chains=1, min_score=1, min_count=1, want_dp=True)
    plain = ctx.chain(reads, want_dp=True)
    for r, (g, p, w) in enumerate(zip(got, plain, want)):
        assert p == w
        if not w["count"]:
            assert g == dict(chains=[], mapq=0, f=[], pred=[])
            continue
        c = dict(g["chains"][0])
        assert c.pop("branch") == -1 and len(g["chains"]) == 1
        assert dict(c, f=g["f"], pred=g["pred"]) == w, r
        assert g["mapq"] == TO.mapq(w["score"], 0, w["count"])
    assert ctx.chain_top_stats["rounds"] == sum(1 for a in reads if len(a))


def ragged_top():
    if "top" not in _cache:
        reads, dp = ragged()   # the DP is the chain tests' own: only the selection is computed here

        def many(max_chains=4, min_score=40, min_count=3, flags=0):
            return [dict(TO.select(a, w.get("f", []), w.get("pred", []), max_chains, min_score, min_count, flags), f=w.get("f", []), pred=w.get("pred", []))
                    for a, w in zip(reads, dp)]
        _cache["top"] = {False: many(), True: many(flags=TO.ROOTED), "low": many(**LOW)}
    return _cache["top"]


def test_a_ragged_list_in_ranges_and_over_poisoned_buffers(ctx):
    reads, _ = ragged()
    counts = [len(a) for a in reads]
    want = ragged_top()
    for rooted in (False, True):
        compare(ctx.chain_top(reads, rooted=rooted, want_dp=True, want_ids=True), want[rooted], ctx.chain_top_stats, rooted)
        assert ctx.chain_top_stats["ranges"] == 1 and ctx.chain_top_stats["chain_ms"] > 0 and ctx.chain_top_stats["top_ms"] > 0
    compare(ctx.chain_top(reads, want_dp=True, want_ids=True, **LOW), want["low"], ctx.chain_top_stats, LOW)
    assert max(len(w["chains"]) for w in want[True]) >= 3 and max(len(w["chains"]) for w in want["low"]) >= 12
    assert sum(w["rounds"] for w in want["low"]) > 2 * sum(len(w["chains"]) for w in want["low"]) - 1500   # and walks that are dropped
    budget = (TO.ANCHOR_BYTES * sum(counts) + TO.read_bytes(4) * len(counts)) // 5
    n_ranges = len(TO.ranges(counts, budget, 4))
    assert n_ranges >= 3
    with switched_context(PWA_RANGE_BYTES=budget) as c:
        compare(c.chain_top(reads, want_dp=True, want_ids=True), want[False], c.chain_top_stats, "ranges")
        assert c.chain_top_stats["ranges"] == n_ranges
    with switched_context(PWA_POISON="0xA5") as c:
        compare(c.chain_top(reads, want_dp=True, want_ids=True), want[False], c.chain_top_stats, "poison")
        assert c.chain_top(reads, rooted=True) == [dict(chains=w["chains"], mapq=w["mapq"]) for w in want[True]]
    with switched_context(PWA_POISON="0xA5", PWA_RANGE_BYTES=budget) as c:
        compare(c.chain_top(reads, rooted=True, want_dp=True, want_ids=True), want[True], c.chain_top_stats, "poison, ranges")
        compare(c.chain_top(reads, want_dp=True, want_ids=True, **LOW), want["low"], c.chain_top_stats, "poison, ranges, low")


def three_copies():
    """a text of 30 kb with a 600-base unit planted at 3000 (as it is), at 12000 (2 % substitutions) and at 24000 (5 %): -> text, unit, loci"""
    if "copies" not in _cache:
        rng = random.Random(77)
        text = bytearray(CO.random_text(rng, 30000))
        unit = bytes(rng.choice(b"ACGT") for _ in range(600))
        loci = (3000, 12000, 24000)
        for at, rate in zip(loci, (0.0, 0.02, 0.05)):
            copy = bytearray(unit)
            for i in rng.sample(range(600), int(600 * rate)):
                copy[i] = rng.choice([b for b in b"ACGT" if b != copy[i]])
            text[at:at + 600] = copy
        _cache["copies"] = bytes(text), unit, loci
    return _cache["copies"]


def test_a_read_from_a_three_copy_repeat_and_a_unique_read(ctx):
    text, unit, loci = three_copies()
    index = CO.kmer_index(text, 12)
    repeat, unique = CO.seed(index, unit, 12), CO.seed(index, text[7000:7600], 12)
    got = check(ctx, [repeat, unique], rooted=True)
    chains = got[0]["chains"]
    assert len(chains) == 3 and all(c["branch"] == -1 for c in chains)
    assert [abs(c["t_begin"] - c["q_begin"] - at) <= 5 for c, at in zip(chains, loci)] == [True] * 3
    assert chains[0]["score"] == 600 > chains[1]["score"] > chains[2]["score"]
    assert got[0]["mapq"] == TO.mapq(chains[0]["score"], chains[1]["score"], chains[0]["count"]) <= 3
    assert got[1]["mapq"] == 60 and got[1]["chains"][0]["score"] == 600


def test_isolated_anchors_cost_one_round_each(ctx):
    """one read of 2^18 isolated anchors under min_count = 2: no chain is kept, every anchor is a round, and the call returns (a
    selection that costs rounds x n would need hours here; tools/chain_top_batch.py and DESIGN.md 3.26 hold the measured time)"""
    n = 1 << 18
    reads = [TO.isolated(n)]
    t0 = time.perf_counter()
    got = ctx.chain_top(reads, min_score=1, min_count=2, want_ids=True)
    print("isolated(2^18): %.3f s, top_ms %.1f" % (time.perf_counter() - t0, ctx.chain_top_stats["top_ms"]))
    assert got[0]["chains"] == [] and got[0]["mapq"] == 0 and got[0]["chain_id"] == [-1] * n
    assert ctx.chain_top_stats["rounds"] == n and ctx.chain_top_stats["anchors"] == n
    got = ctx.chain_top(reads, min_score=1, min_count=1, max_chains=16)
    assert [c["last"] for c in got[0]["chains"]] == list(range(16)) and ctx.chain_top_stats["rounds"] == 16
