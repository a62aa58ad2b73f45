"""chain_oracle.py against first principles, without a GPU: the DP against an exhaustive search over all anchor subsequences, beta at
its corners, the three tie rules, and planted reads on a text with a repeat."""
import random

import chain_oracle as CO


def test_dp_equals_the_best_subsequence():
    """lists of at most 12 anchors, lookback >= n so that the window does not bite: the maximal f is the best score over every
    subsequence scored by the same alpha - beta terms, and the chain the oracle walks back has that score"""
    rng = random.Random(11)
    seen_chain = 0
    for case in range(60):
        n = rng.randint(1, 12)
        anchors = CO.random_anchors(rng, n, span=rng.choice([30, 120, 400]), max_len=rng.choice([1, 8, 20]))
        params = dict(max_dist=rng.choice([5, 40, 5000]), bandwidth=rng.choice([0, 3, 500]), gap_scale=rng.choice([0, 38, 1024]))
        got = CO.chain(anchors, lookback=rng.choice([n, 12, 64]), **params)
        assert got["score"] == CO.best_subsequence(anchors, **params), (case, anchors, params)
        walk, i = [], got["last"]
        while i >= 0:
            walk.append(i)
            i = got["pred"][i]
        walk.reverse()
        assert len(walk) == got["count"]
        s = anchors[walk[0]][2]
        for a, b in zip(walk, walk[1:]):
            s += CO.link(anchors[a], anchors[b], **params)
        assert s == got["score"]
        seen_chain += got["count"] > 1
    assert seen_chain > 20


def test_the_lockstep_form_equals_the_plain_loop():
    rng = random.Random(17)
    for case in range(12):
        reads = [CO.random_anchors(rng, rng.choice([0, 1, 2, 7, 40, 150]), span=rng.choice([30, 400]), max_len=rng.choice([1, 20])) for _ in range(9)]
        reads.append([(10, 10, 4), ((1 << 20) + 50, 50, 4), ((1 << 20) + 51, 50, 4)])   # dd = 2^20 - 4 and one more
        params = dict(lookback=rng.choice([1, 3, 64, 512]), max_dist=rng.choice([5, 40, 5000, 1 << 30]), bandwidth=rng.choice([0, 3, 500, 1 << 20]),
                      gap_scale=rng.choice([0, 38, 1024]))
        assert CO.chain_many_fast(reads, **params) == CO.chain_many(reads, **params), (case, params)
        assert CO.chain_many_fast(reads, want_dp=False, **params) == CO.chain_many(reads, want_dp=False, **params)
    assert CO.chain_many_fast([]) == [] and CO.chain_many_fast([[]]) == CO.chain_many([[]])


def test_the_window_bites():
    """a predecessor further back than lookback is not seen"""
    anchors = [(10, 10, 5), (15, 300, 1), (16, 300, 1), (17, 300, 1), (15, 15, 5)]   # three strays between the two on the diagonal
    assert CO.validate([anchors]) == (0, None)
    assert CO.chain(anchors, lookback=4, max_dist=50, bandwidth=10)["score"] == 10
    assert CO.chain(anchors, lookback=3, max_dist=50, bandwidth=10)["score"] == 5


def test_beta():
    want = {0: 0, 1: 0, 2: 0, 3: 0, 4: 1, 7: 1, 8: 1, 1 << 20: 10}   # floor(log2 dd) >> 1
    for dd, logpart in want.items():
        assert CO.beta(dd, 0) == logpart, dd
        assert CO.beta(dd, 38) == ((38 * dd) >> 8) + logpart
        assert CO.beta(dd, 1024) == 4 * dd + logpart
    assert CO.beta(1 << 20, 1024) == (1 << 22) + 10 < 1 << 31
    assert CO.beta(7, 38) == 2 and CO.beta(8, 38) == 2 and CO.beta(3, 100) == 1


def test_tie_largest_j_wins():
    anchors = [(10, 10, 5), (10, 10, 5), (20, 20, 5)]   # two equal predecessors
    got = CO.chain(anchors)
    assert got["f"] == [5, 5, 10] and got["pred"] == [-1, -1, 1]


def test_tie_cand_equal_to_len_keeps_no_pred():
    # dd = 4 at gap_scale 256: beta = 4 + 1; cand = 5 + min(10, 14, 10) - 5 = 10 = len_i
    anchors = [(0, 0, 5), (9, 5, 10)]
    assert CO.link(anchors[0], anchors[1], 5000, 500, 256) == 5
    got = CO.chain(anchors, gap_scale=256)
    assert got["f"] == [5, 10] and got["pred"] == [-1, -1] and got["count"] == 1 and got["last"] == 1
    got = CO.chain([(0, 0, 6), (10, 6, 10)], gap_scale=256)   # one better: the link is taken
    assert got["f"] == [6, 11] and got["pred"] == [-1, 0]


def test_tie_smallest_e_wins():
    anchors = [(10, 10, 7), (5000, 40, 7), (9000, 90, 7)]   # three chains of one anchor, equal scores
    got = CO.chain(anchors, max_dist=100)
    assert got["f"] == [7, 7, 7] and got["last"] == 0 and (got["t_begin"], got["t_end"], got["q_begin"], got["q_end"]) == (10, 17, 10, 17)


def test_planted_reads_on_a_text_with_a_repeat():
    """40 reads of 1500 symbols at 8 % on a 20 kb text holding one 600-base repeat, k = 11: the chain's t_begin - q_begin lands within 60
    of the planted start for all 40"""
    rng = random.Random(5)
    text = CO.random_text(rng, 20000, repeat=600, copies=2)
    assert text[:600] == text[-600:]
    index = CO.kmer_index(text, 11)
    reads = CO.planted_reads(rng, text, 38, 1500, 0.08)
    reads += [(CO.mutate(rng, text[at:at + 1500], 0.08), at, "+") for at in (0, 20000 - 1500)]   # two that start or end in the repeat
    for read, at, _ in reads:
        c = CO.chain(CO.seed(index, read, 11), want_dp=False)
        assert c["count"] > 5
        assert abs(c["t_begin"] - c["q_begin"] - at) <= 60, (at, c)
        assert c["diag_lo"] <= c["t_begin"] - c["q_begin"] <= c["diag_hi"]


def test_ranges_and_validation_of_the_oracle():
    assert CO.ranges([], 0) == [] and CO.ranges([0, 0], 0) == []
    assert CO.ranges([3, 0, 2], 0) == [(0, 3)]
    assert CO.ranges([3, 0, 2], 120) == [(0, 1), (1, 3)]      # 100 + 40 > 120 >= 40 + 80
    assert CO.ranges([3, 0, 2], 100) == [(0, 1), (2, 3)]      # the empty read alone launches nothing
    assert CO.ranges([3, 0, 0, 2], 80) == [(0, 1), (3, 4)]    # the two empty reads share a range that launches nothing
    assert CO.ranges([3, 3], 1) == [(0, 1), (1, 2)]
    assert CO.validate([[(5, 5, 1), (4, 4, 1)]]) == (CO.INVALID, 0)
    assert CO.validate([[], [(5, 5, 0)]]) == (CO.INVALID, 1)
    assert CO.validate([[((1 << 31) - 2, 0, 1)]]) == (0, None)
    assert CO.validate([[((1 << 31) - 1, 0, 1)]]) == (CO.CAPACITY, 0)
    assert CO.validate([[]], lookback=513) == (CO.INVALID, None)
