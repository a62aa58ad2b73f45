"""chain_top_oracle.py against what its definition promises, without a GPU: chain 0 against chain_oracle.chain, kept chains disjoint,
every score the sum of its links, chain_id and rounds against the walks, mapq at its corners -- and the oracle restated with one
mistake at a time: every mutant changes the result of at least one built case, so the built cases (which test_gpu_chain_top.py runs on
the device) can tell a kernel with that mistake from a right one."""
import random

import pytest

import chain_oracle as CO
import chain_top_oracle as TO


def random_cases(count=300, seed=23):
    rng = random.Random(seed)
    for case in range(count):
        n = rng.randint(1, 200)
        anchors = CO.random_anchors(rng, n, span=rng.choice([30, 120, 400]), max_len=rng.choice([1, 8, 20]))
        dp = dict(lookback=rng.choice([1, 3, 64, 512]), max_dist=rng.choice([5, 40, 5000]), bandwidth=rng.choice([0, 3, 500]), gap_scale=rng.choice([0, 38, 1024]))
        yield case, anchors, dp, rng


def walk_of(c, got):
    """the anchors of kept chain c, from its last anchor back: along pred until the count is used up"""
    walk = [c["last"]]
    while len(walk) < c["count"]:
        walk.append(got["pred"][walk[-1]])
    return walk


def test_chain_0_at_1_1_equals_the_best_chain():
    for case, anchors, dp, rng in random_cases():
        got = TO.chain_top(anchors, max_chains=rng.randint(1, 16), min_score=1, min_count=1, rooted=rng.random() < 0.5, **dp)
        want = CO.chain(anchors, **dp)
        c0 = dict(got["chains"][0])
        assert c0.pop("branch") == -1
        assert c0 == {k: v for k, v in want.items() if k not in ("f", "pred")}, case
        assert (got["f"], got["pred"]) == (want["f"], want["pred"])


def test_kept_chains_are_disjoint_scored_by_their_links_and_listed_in_chain_id():
    branched = dropped = 0
    for case, anchors, dp, rng in random_cases():
        N, ms, mc, rooted = rng.randint(1, 16), rng.choice([1, 5, 20, 40]), rng.choice([1, 2, 3, 6]), rng.random() < 0.5
        got = TO.chain_top(anchors, max_chains=N, min_score=ms, min_count=mc, rooted=rooted, **dp)
        link = dict(max_dist=dp["max_dist"], bandwidth=dp["bandwidth"], gap_scale=dp["gap_scale"])
        ids = [-1] * len(anchors)
        assert len(got["chains"]) <= N and got["rounds"] >= len(got["chains"])
        for ci, c in enumerate(got["chains"]):
            walk = walk_of(c, got)
            b = walk[-1]
            assert all(ids[i] == -1 for i in walk), (case, "kept chains share an anchor")
            for i in walk:
                ids[i] = ci
            assert got["pred"][b] == c["branch"] and (not rooted or c["branch"] == -1)
            s = anchors[b][2] if c["branch"] < 0 else CO.link(anchors[c["branch"]], anchors[b], **link)
            for i, j in zip(walk[1:], walk):   # j follows i
                s += CO.link(anchors[i], anchors[j], **link)
            assert s == c["score"] >= ms and c["count"] >= mc, case
            assert c["score"] <= got["chains"][0]["score"] or ms > 1 or mc > 1
            A = [anchors[i] for i in walk]
            assert (c["q_begin"], c["t_begin"]) == (anchors[b][1], anchors[b][0])
            assert (c["q_end"], c["t_end"]) == (A[0][1] + A[0][2], A[0][0] + A[0][2])
            assert (c["diag_lo"], c["diag_hi"]) == (min(a[0] - a[1] for a in A), max(a[0] - a[1] for a in A))
            branched += c["branch"] >= 0
        assert ids == got["chain_id"], case
        assert all(a["score"] >= b["score"] for a, b in zip(got["chains"], got["chains"][1:]) if a["branch"] < 0 and b["branch"] < 0)
        dropped += got["rounds"] > len(got["chains"])
        rootedscores = [c["score"] for c in got["chains"][1:] if c["branch"] < 0]
        want_mapq = TO.mapq(got["chains"][0]["score"], max(rootedscores, default=0), got["chains"][0]["count"]) if got["chains"] else 0
        assert got["mapq"] == want_mapq
    assert branched > 50 and dropped > 50


def test_no_score_exceeds_chain_0():
    for case, anchors, dp, rng in random_cases(150, seed=5):
        got = TO.chain_top(anchors, max_chains=16, min_score=1, min_count=1, **dp)
        assert all(c["score"] <= got["chains"][0]["score"] for c in got["chains"]), case
        assert sum(c["count"] for c in got["chains"]) == sum(i >= 0 for i in got["chain_id"])


def test_the_numpy_form_equals_the_plain_loop():
    rng = random.Random(2)
    reads = [CO.random_anchors(rng, rng.choice([0, 1, 2, 7, 40, 150])) for _ in range(12)]
    for params in (dict(), dict(max_chains=16, min_score=1, min_count=1, rooted=True), dict(min_score=12, min_count=2, lookback=3)):
        assert TO.chain_top_many_fast(reads, **params) == TO.chain_top_many(reads, **params)


def test_mapq_corners():
    assert TO.mapq(100, 0, 10) == 60 and TO.mapq(100, 0, 11) == 60 and TO.mapq(100, 0, 9) == 54 and TO.mapq(100, 0, 0) == 0
    assert TO.mapq(100, 100, 10) == 0 and TO.mapq(100, 200, 10) == 0 and TO.mapq(100, -5, 10) == 60
    assert TO.mapq(0, 0, 10) == 0 and TO.mapq(-3, 0, 10) == 0
    assert TO.mapq(1 << 30, 1, 10) == 59 and TO.mapq(600, 592, 40) == 0 and TO.mapq(3, 2, 1) == 2


def test_the_builders_keep_their_promises():
    f = TO.chain_top(TO.fork(), min_score=10, min_count=1)
    assert f["pred"] == [-1, 0, 1, 1] and f["f"] == [10, 20, 30, 30]
    assert [(c["score"], c["count"], c["last"], c["branch"]) for c in f["chains"]] == [(30, 3, 2, -1), (10, 1, 3, 1)]
    assert len(TO.chain_top(TO.fork(), min_score=10, min_count=1, rooted=True)["chains"]) == 1
    o = TO.chain_top(TO.orphan_branch(), min_score=5, min_count=1)
    assert o["pred"][:3] == [-1, 0, 0] and o["f"][:3] == [10, 18, 20]          # P, R, Q in (x, y) order
    assert [(c["score"], c["last"], c["branch"]) for c in o["chains"]] == [(40, 6, -1), (20, 2, -1), (8, 1, 0)]
    o = TO.chain_top(TO.orphan_branch(), min_score=5, min_count=3)
    assert len(o["chains"]) == 1 and o["rounds"] == 3 and o["chain_id"][:3] == [-1, -1, -1]
    for gap, lead, mid, high in ((0, 0, 0, 0), (61, 0, 0, 63), (200, 30, 150, 10)):
        a = TO.pad_high(TO.equal_f(gap, lead, mid), high)
        e = TO.chain_top(a, min_score=30, min_count=3, max_chains=4)
        assert [(c["score"], c["last"]) for c in e["chains"]] == [(30, lead + 2), (30, lead + gap + 5)]
        assert e["rounds"] == high + mid + 2
    i = TO.chain_top(TO.isolated(130, 3), min_score=1, min_count=2)
    assert i["f"] == [3] * 130 and i["pred"] == [-1] * 130 and i["chains"] == [] and i["rounds"] == 130
    for lane, block in ((0, 1), (63, 1), (63, 0)):
        s = TO.chain_top(TO.stop_at_lane(lane, block), min_score=10, min_count=1)
        assert s["chains"][1]["branch"] == 64 * block + lane and s["chains"][1]["last"] == 64 * block + lane + 2
    for lane, block in ((1, 0), (0, 1), (63, 1)):
        s = TO.chain_top(TO.stop_at_lane(lane, block, 62), min_score=5, min_count=1, gap_scale=0)
        at = 64 * block + lane
        assert [(c["score"], c["last"], c["branch"]) for c in s["chains"][:2]] == [(30, at + 1, -1), (7, at + 64, at)] and s["pred"][at + 64] == at   # then strays
    for name, anchors, params in TO.built_cases():
        assert CO.validate([anchors]) == (0, None), name


@pytest.mark.parametrize("bug", TO.BUGS)
def test_every_mutant_is_caught_by_a_built_case(bug):
    caught = [name for name, anchors, params in TO.built_cases() if TO.chain_top(anchors, bug=bug, **params) != TO.chain_top(anchors, **params)]
    assert caught, bug


def test_validation_and_ranges_restate_the_call():
    good = [[(5, 5, 3), (9, 9, 3)]]
    assert TO.validate(good) == (0, None)
    for params in (dict(max_chains=0), dict(max_chains=17), dict(min_score=0), dict(min_score=(1 << 30) + 1), dict(min_count=0),
                   dict(min_count=(1 << 24) + 1), dict(flags=2), dict(flags=3), dict(lookback=0)):
        assert TO.validate(good + [[(5, 5, 0)]], **params) == (CO.INVALID, None)
    assert TO.validate(good + [[(5, 5, 0)]]) == (CO.INVALID, 1)
    assert TO.read_bytes(4) == 176 and TO.ANCHOR_BYTES == 48
    # 272 bytes hold read 0, then the empty read 1 alone (a range without anchors is left out), then read 2 alone exceeds them
    assert TO.ranges([2, 0, 3], 48 * 2 + 176) == [(0, 1), (2, 3)] and TO.ranges([2, 0, 3], 0) == [(0, 3)]
    assert TO.ranges([0, 0], 1) == []
