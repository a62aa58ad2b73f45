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


MUTANTS = ["win+1", "win-1", "dead64", "dead128", "dead192", "dead256", "dead448", "stale64", "stale128", "stale256", "tie_small_j", "nonstrict"]


def dp_mutant(reads, mut=None, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38):
    """chain_oracle.dp of every read with one named mistake (None: none), the way a kernel that keeps its window in chunks of 64 lanes
    could be wrong -> [(f, pred)].  Written per anchor over numpy arrays of the window, j descending (offset 0 first):
        win+1 / win-1   the window is one longer / one shorter
        deadK           a predecessor at offset >= K (offset: i - 1 - j) is never admissible
        staleK          a predecessor at offset >= K is read one lane stale: x, y and f are those of j + 1
        tie_small_j     the smallest j among equal cand
        nonstrict       cand >= len_i takes the link"""
    import numpy as np
    H = lookback + (mut == "win+1") - (mut == "win-1")
    dead = int(mut[4:]) if mut and mut.startswith("dead") else 1 << 30
    stale = int(mut[5:]) if mut and mut.startswith("stale") else 1 << 30
    out = []
    for anchors in reads:
        n = len(anchors)
        A = np.asarray(anchors, dtype=np.int64).reshape(-1, 3)
        X, Y, L = A[:, 0] + A[:, 2], A[:, 1] + A[:, 2], A[:, 2]
        F, P = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        for i in range(n):
            off = np.arange(min(i, H))
            j = i - 1 - off
            src = np.where(off >= stale, j + 1, j)
            dx, dy = X[i] - X[src], Y[i] - Y[src]
            dd = np.abs(dx - dy)
            adm = (dx > 0) & (dx <= max_dist) & (dy > 0) & (dy <= max_dist) & (dd <= bandwidth) & (off < dead)
            F[i] = L[i]
            if not adm.any():
                continue
            dx, dy, dd, ja = dx[adm], dy[adm], dd[adm], j[adm]
            bt = np.where(dd > 0, ((gap_scale * dd) >> 8) + ((np.frexp(np.maximum(dd, 1).astype(np.float64))[1] - 1) >> 1), 0)   # CO.beta
            cand = F[src[adm]] + np.minimum(L[i], np.minimum(dx, dy)) - bt
            best = cand.max()
            if best >= L[i] if mut == "nonstrict" else best > L[i]:
                F[i] = best
                P[i] = ja[cand == best].min() if mut == "tie_small_j" else ja[cand == best].max()
        out.append((F.tolist(), P.tolist()))
    return out


def noticed(case, mut):
    """the reads of a case whose (f, pred) change under a mistake"""
    if mut.startswith(("dead", "stale")) and int(mut.lstrip("adelst")) >= case["params"]["lookback"]:
        return []   # no offset of this window is that large
    return [r for r, (a, b) in enumerate(zip(case["dp"], dp_mutant(case["reads"], mut, **case["params"]))) if a != b]


def test_the_far_window_cases_tell_a_wrong_recurrence_from_the_right_one():
    """every call of the GPU suite's far-window tests is valid input; dp_mutant without a mistake is the oracle's dp; and each
    mistake changes (f, pred) of at least one read -- of the edge, walk and tie cases for the window, the chunks and the ties, and
    of the seeded list for dead128, which is what that list is there for.  This is the proof that those GPU tests would notice a
    kernel with a dead or shifted chunk; no broken kernel is ever run"""
    cases = CO.far_cases()
    assert {c["params"]["lookback"] for c in cases} >= set(CO.EDGE_LOOKBACKS)
    assert {CO.chunks_of(c["params"]["lookback"]) for c in cases} == {1, 2, 4, 8}
    for c in cases:
        assert len(c["reads"]) == len(c["labels"]) > 0
        assert CO.validate(c["reads"], **c["params"]) == (0, None), c["name"]
        c["dp"] = [(w["f"], w["pred"]) for w in CO.chain_many_fast(c["reads"], **c["params"])]
        if not c["name"].startswith("seeded") and c["name"] != "mixed":   # those two: the lockstep form, held to dp() above
            assert c["dp"] == [CO.dp(a, **c["params"]) for a in c["reads"]], c["name"]
        assert dp_mutant(c["reads"], None, **c["params"]) == c["dp"], c["name"]
    built = [c for c in cases if not c["name"].startswith("seeded") and c["name"] != "mixed"]   # mixed repeats their reads
    for mut in MUTANTS:
        hits = sum(len(noticed(c, mut)) for c in built)
        print(mut, hits)
        assert hits >= 1, mut
    for c in cases:
        if c["name"].startswith("seeded"):
            assert noticed(c, "dead128"), c["name"]
            assert max(len(a) for a in c["reads"]) > 2000


def test_the_earlier_inputs_do_not_reach_beyond_offset_127():
    """why the far-window cases exist: on the inputs of test_anchor_counts_around_the_block_and_the_window a window that is dead, or one
    lane stale, from offset 128 on changes nothing"""
    from test_gpu_chain import block_and_window_inputs
    for lookback in (1, 63, 64, 65, 128, 512):
        reads, params = block_and_window_inputs(lookback)
        want = [CO.dp(a, **params) for a in reads]
        assert dp_mutant(reads, None, **params) == want
        for mut in ("dead128", "stale128"):
            assert dp_mutant(reads, mut, **params) == want, (lookback, mut)


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
