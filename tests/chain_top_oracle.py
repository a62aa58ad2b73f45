"""Top-N chains of a read and mapping quality (pwa_chain_top, pwa_mapq; include/pwalign.h, "Top-N chains of a read") restated in plain
Python: the test-side oracle of the feature.  Anchors, their order, the parameters of the DP, f and pred are chain_oracle's.

Per read every anchor carries a mark, initially free.  Candidates are the anchors in order of descending f, the smaller index first
among equal f.  For each candidate e, in that order:
  1. stop the read when N chains are kept, or when f(e) < min_score;
  2. skip e if it is marked;
  3. otherwise this is a round: walk cur = e, pred(cur), ...  The walk ends at the anchor b whose pred is -1 (base 0, branch -1) or
     at the anchor b whose pred p is already marked (base f(p), branch p);
  4. score = f(e) - base, count = the anchors of the walk;
  5. kept iff score >= min_score and count >= min_count and (not ROOTED or branch == -1);
  6. the walk's anchors are marked either way: with the kept chain's index, or as dropped (-2).
mapq(s1, s2, c1) = min(60, (60 (s1 - s2) min(c1, 10)) div (10 s1)), 0 when s1 <= 0, s2 clamped to [0, s1]; a read's mapq takes s1 and
c1 from chain 0 and s2 from the best chain 1 .. with branch -1 (0 if none), and is 0 without a kept chain.

`bug` restates the selection with one mistake (test_chain_top_oracle.py shows that the built cases catch each of them)."""
import chain_oracle as CO

ROOTED = 1
FREE, DROPPED = -1, -2
ANCHOR_BYTES = 48   # device bytes per anchor: t, q, len, f, pred, the mark, two sort keys of 8 and two sort values of 4


def read_bytes(max_chains):
    """device bytes per read: its chain slots of ten words and a head of four"""
    return 40 * max_chains + 16


BUGS = ("larger_index", "dropped_unmarked", "base_at_b", "stop_at_dropped", "dropped_count", "score_gt", "count_gt", "rooted_ignored", "s2_branched")


def mapq(s1, s2, c1):
    if s1 <= 0:
        return 0
    s2 = min(max(s2, 0), s1)
    return min(60, (60 * (s1 - s2) * min(c1, 10)) // (10 * s1))


def select(anchors, f, pred, max_chains=4, min_score=40, min_count=3, flags=0, bug=None):
    """the selection over a DP computed elsewhere -> dict(chains, mapq, chain_id, rounds)"""
    assert bug is None or bug in BUGS
    n = len(anchors)
    mark = [FREE] * n
    order = sorted(range(n), key=lambda i: (-f[i], -i if bug == "larger_index" else i))
    chains, rounds, slots = [], 0, 0   # slots: what counts toward N
    for e in order:
        if slots >= max_chains or f[e] < min_score:
            break
        if mark[e] != FREE:
            continue
        rounds += 1
        walk, cur = [e], e
        while pred[cur] >= 0 and mark[pred[cur]] == FREE:
            assert pred[cur] < cur
            cur = pred[cur]
            walk.append(cur)
        b, branch = cur, pred[cur]
        base = 0 if branch < 0 else f[b] if bug == "base_at_b" else f[branch]
        score, count = f[e] - base, len(walk)
        keep = (score > min_score if bug == "score_gt" else score >= min_score) and (count > min_count if bug == "count_gt" else count >= min_count)
        if flags & ROOTED and bug != "rooted_ignored":
            keep = keep and branch < 0
        if keep:
            A = [anchors[i] for i in walk]
            chains.append(dict(score=score, count=count, last=e, q_begin=anchors[b][1], q_end=anchors[e][1] + anchors[e][2], t_begin=anchors[b][0],
                               t_end=anchors[e][0] + anchors[e][2], diag_lo=min(a[0] - a[1] for a in A), diag_hi=max(a[0] - a[1] for a in A),
                               branch=branch))
            slots += 1
        else:
            if bug == "stop_at_dropped":
                break
            if bug == "dropped_count":
                slots += 1
        if keep or bug != "dropped_unmarked":
            for i in walk:
                mark[i] = len(chains) - 1 if keep else DROPPED
    s2 = max([c["score"] for c in chains[1:] if c["branch"] < 0 or bug == "s2_branched"], default=0)
    return dict(chains=chains, mapq=mapq(chains[0]["score"], s2, chains[0]["count"]) if chains else 0, chain_id=[m if m >= 0 else -1 for m in mark],
                rounds=rounds)


def chain_top(anchors, max_chains=4, min_score=40, min_count=3, rooted=False, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38, bug=None):
    """one read's result as Context.chain_top returns it with want_dp and want_ids, plus rounds"""
    anchors = [tuple(int(v) for v in a) for a in anchors]
    f, pred = CO.dp(anchors, lookback, max_dist, bandwidth, gap_scale)
    out = select(anchors, f, pred, max_chains, min_score, min_count, ROOTED if rooted else 0, bug)
    out.update(f=f, pred=pred)
    return out


def chain_top_many(reads, **params):
    return [chain_top(a, **params) for a in reads]


def chain_top_many_fast(reads, max_chains=4, min_score=40, min_count=3, rooted=False, **dp_params):
    """chain_top_many with the DP of chain_oracle.dp_many (numpy, for lists too large for the plain loop)"""
    out = []
    for a, (f, pred) in zip(reads, CO.dp_many(reads, **dp_params)):
        a = [tuple(int(v) for v in x) for x in a]
        o = select(a, f, pred, max_chains, min_score, min_count, ROOTED if rooted else 0)
        o.update(f=f, pred=pred)
        out.append(o)
    return out


def validate(reads, max_chains=4, min_score=40, min_count=3, flags=0, **params):
    """(code, first offending read or None) as pwa_chain_top_plan answers: the new parameters in the parameter step, then chain_oracle's"""
    if not (1 <= max_chains <= 16 and 1 <= min_score <= 1 << 30 and 1 <= min_count <= 1 << 24 and flags in (0, ROOTED)):
        return CO.INVALID, None
    return CO.validate(reads, **params)


def ranges(counts, budget, max_chains=4):
    """chain_oracle.ranges with this call's bytes per anchor and per read"""
    out, k0, n = [], 0, len(counts)
    weight = lambda r: ANCHOR_BYTES * counts[r] + read_bytes(max_chains)
    while k0 < n:
        k1, tot = k0 + 1, weight(k0)
        while k1 < n and (not budget or tot + weight(k1) <= budget):
            tot += weight(k1)
            k1 += 1
        if any(counts[k0:k1]):
            out.append((k0, k1))
        k0 = k1
    return out


# ---- builders that put the deciding anchor where a test wants it.  All under the default DP parameters; anchors of len 10 on a
# ---- diagonal, text ends 10 apart, link with gain 10 and no gap cost

def _run(t0, q0, k, ln=10):
    """k anchors in a row on one diagonal, each adding ln"""
    return [(t0 + ln * i, q0 + ln * i, ln) for i in range(k)]


def fork(pad=0):
    """X -> Y, then Z1 and Z2 both with pred = Y (after `pad` isolated anchors that shift every index).  Z1 = (t, q) continues the
    diagonal; Z2 starts one text base further (after Y dd = 1: beta = 0 under gap_scale 38; after Z1 dy = 0: not admissible), equal f.  The first walk is Z1, Y, X: score 30, count 3,
    rooted.  The second is Z2 alone: a one-anchor stub with branch = Y, score 10.  Under ROOTED it is dropped"""
    stray = [(10 + 7000 * i, 5000, 5) for i in range(pad)]   # far apart in t, far off in q: no links
    base = 7000 * pad + 20000
    return sorted(stray + _run(base, 100, 3) + [(base + 21, 120, 10)], key=lambda a: (a[0] + a[2], a[1] + a[2]))


def orphan_branch():
    """P -> Q is dropped by min_count = 3; R has pred = P and f(R) < f(Q); R's walk stops at the dropped P: branch = P, score
    f(R) - f(P).  A third, longer chain elsewhere is kept first.  P = len 10, Q = len 10 on the diagonal (f 20), R = len 8 two off
    the diagonal (f 18 - 0)"""
    main = _run(50000, 300, 4)                       # f 10 .. 40: kept, chain 0
    P, Q = (1000, 100, 10), (1010, 110, 10)          # f 10, 20
    R = (1012, 110, 8)                               # after P: dx 10, dy 8, dd 2: gain min(8, 10, 8) - beta(2) = 8 - 0 -> f 18; after Q: dx 0, no
    return sorted([P, Q, R] + main, key=lambda a: (a[0] + a[2], a[1] + a[2]))


def equal_f(gap, lead=0, mid=0):
    """two rooted chains of equal f = 30 (three anchors each); `lead` isolated anchors before the first, `gap` isolated anchors between
    them in the anchor array (the first `mid` of them of len 30, the others of len 5), so that the two ends sit `gap` + 3 apart in the
    anchor array and `mid` + 1 apart in the sorted order; pad_high() moves both down the sorted order"""
    stray = lambda k, t0, ln: [(t0 + 6000 * i, 9000, ln) for i in range(k)]
    a = _run(6000 * lead + 100000, 100, 3)
    t1 = a[-1][0] + 6000
    b0 = t1 + 6000 * gap + 6000
    return stray(lead, 10, 5) + a + stray(mid, t1, 30) + stray(gap - mid, t1 + 6000 * mid, 5) + _run(b0, 100, 3)


def pad_high(anchors, k, ln=60):
    """anchors, then k isolated anchors of len `ln` (f = ln above every f of the builders): they come first in the sorted order and
    shift every candidate of `anchors` by k places"""
    t0 = max(a[0] + a[2] for a in anchors) + 6000
    return list(anchors) + [(t0 + 6000 * i, 9500, ln) for i in range(k)]


def isolated(n, ln=1):
    """n anchors more than max_dist = 5000 apart: every f = len, every pred = -1"""
    return [(5001 * i, 0, ln) for i in range(n)]


def stop_at_lane(lane, block=1, far=0):
    """a kept chain whose second anchor sits at index 64 * block + lane, and a later-ranked anchor S with that second anchor as its
    pred: its walk stops at once, at a marked anchor in lane `lane` of block `block`.  Index layout: isolated strays up to the index,
    then chain A = (a0, a1 at the index, a2), then `far` strays (at most 62), then S at index + 2 + far with pred = a1 and no link to
    a2 (dy = 0).  far = 0: S is one text base off the diagonal, f(S) = 30 = f(a2).  far > 0 (use gap_scale 0): S ends far + 8 text
    bases later, dd = far + 8, f(S) = 30 - (floor(log2 dd) >> 1); far = 62 puts S in the next block at a1's lane"""
    at = 64 * block + lane
    assert 0 <= far <= 62 and at >= 1   # a0 sits before a1
    stray = [(10 + 6000 * i, 9000, 5) for i in range(at - 1)]
    t0 = 6000 * at + 100000
    A = _run(t0, 100, 3)                      # indices at - 1, at, at + 1
    if not far:
        return stray + A + [(t0 + 21, 120, 10)]           # after a1: dx 11, dy 10, dd 1
    between = [(t0 + 26 + i, 9000, 5) for i in range(far)]   # text ends t0 + 31 ..: after a2, before S; no links (dy 0 or beyond max_dist)
    return stray + A + between + [(t0 + 28 + far, 120, 10)]   # after a1: dx far + 18, dy 10, dd far + 8


def many_chains(k, length=3):
    """k rooted chains of `length` anchors, more than max_dist apart, scores descending by one (the first anchor's len)"""
    out = []
    for c in range(k):
        t0 = 20000 * c + 1000
        out += [(t0, 100, 10 + k - c)] + [(t0 + k - c + 10 * i, 100 + k - c + 10 * i, 10) for i in range(1, length)]
    return out


def built_cases():
    """[(name, anchors, params)]: the cases test_chain_top_oracle.py holds the mutants to and test_gpu_chain_top.py runs on the device"""
    cases = []
    for rooted in (False, True):
        for pad in (0, 70):
            cases.append(("fork-%d-%d" % (pad, rooted), fork(pad), dict(min_score=10, min_count=1, rooted=rooted)))
    cases.append(("fork-low", fork(), dict(min_score=1, min_count=1)))
    cases.append(("orphan", orphan_branch(), dict(min_score=5, min_count=3)))
    cases.append(("orphan-1", orphan_branch(), dict(min_score=5, min_count=1)))
    cases.append(("orphan-n2", orphan_branch(), dict(min_score=5, min_count=3, max_chains=2)))
    # the tied ends in one block of 64, in adjacent blocks and in far blocks, of the anchor array and of the sorted order
    for gap, lead, mid, high in ((0, 0, 0, 0), (0, 0, 0, 63), (61, 0, 0, 0), (61, 0, 0, 63), (200, 30, 150, 10), (200, 0, 0, 127), (3, 0, 3, 61)):
        a = pad_high(equal_f(gap, lead, mid), high)
        cases.append(("equal-%d-%d-%d-%d" % (gap, lead, mid, high), a, dict(min_score=30, min_count=3, max_chains=1)))
        cases.append(("equal-all-%d-%d-%d-%d" % (gap, lead, mid, high), a, dict(min_score=30, min_count=3, max_chains=4)))
    for n in (1, 63, 64, 65, 130):
        cases.append(("isolated-%d" % n, isolated(n, 3), dict(min_score=3, min_count=1, max_chains=16)))
        cases.append(("isolated-c2-%d" % n, isolated(n, 3), dict(min_score=1, min_count=2)))
    for lane, block in ((0, 1), (63, 1), (0, 2), (63, 0), (17, 3)):
        cases.append(("stop-%d-%d" % (lane, block), stop_at_lane(lane, block), dict(min_score=10, min_count=1)))
        cases.append(("stop-rooted-%d-%d" % (lane, block), stop_at_lane(lane, block), dict(min_score=10, min_count=1, rooted=True)))
    for lane, block in ((1, 0), (0, 1), (63, 1), (5, 2)):   # ... and at a1's own lane of the block before S's
        cases.append(("stop-far-%d-%d" % (lane, block), stop_at_lane(lane, block, 62), dict(min_score=5, min_count=1, gap_scale=0)))
    cases.append(("stop-far-30", stop_at_lane(40, 1, 30), dict(min_score=5, min_count=1, gap_scale=0, rooted=True)))
    cases.append(("many-16", many_chains(20), dict(min_score=20, min_count=3, max_chains=16)))
    cases.append(("many-4", many_chains(20), dict(min_score=20, min_count=3, max_chains=4)))
    s = many_chains(3)[0][2] + 20                     # the best chain's score
    for ms in (s - 1, s, s + 1):                      # a chain scoring exactly min_score and one scoring min_score - 1
        cases.append(("score-%d" % ms, many_chains(3), dict(min_score=ms - 1, min_count=1)))
    for mc in (2, 3, 4):                              # exactly min_count anchors, and min_count - 1
        cases.append(("count-%d" % mc, many_chains(3) + _run(90000, 100, 2), dict(min_score=10, min_count=mc)))
    cases.append(("branched-second", fork() + _run(60000, 100, 2), dict(min_score=10, min_count=1)))   # chain 1 the rooted run, chain 2 the stub
    short_first = [(500, 100, 50)] + many_chains(3)   # an isolated anchor of f = 50 comes first and is dropped by min_count; the chains follow
    cases.append(("short-first", short_first, dict(min_score=20, min_count=3, max_chains=3)))
    cases.append(("short-first-2", short_first, dict(min_score=20, min_count=3, max_chains=2)))
    return cases
