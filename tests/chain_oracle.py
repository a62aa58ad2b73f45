"""Collinear chaining of anchors (pwa_chain_anchors, include/pwalign.h) restated in plain Python: the test-side oracle of the feature.

An anchor of a read is (t, q, len), len >= 1: read[q .. q + len) == text[t .. t + len).  x = t + len, y = q + len.  Within a read the
anchors are in non-decreasing lexicographic order of (x, y).  For anchor i, over the predecessors j in [max(0, i - H), i), all of them:
    dx = x_i - x_j, dy = y_i - y_j, dd = |dx - dy|
    j is admissible iff 0 < dx <= max_dist, 0 < dy <= max_dist and dd <= bandwidth
    cand(j) = f(j) + min(len_i, dx, dy) - beta(dd)
    beta(0) = 0; for dd >= 1, beta(dd) = ((gap_scale * dd) >> 8) + (floor(log2 dd) >> 1)
    f(i) = max(len_i, max_j cand(j))
    pred(i) = -1 unless some admissible cand(j) > len_i strictly; otherwise the largest j among the admissible j of maximal cand.
The chain ends at e, the smallest index with maximal f, and runs e, pred(e), ... down to b with pred(b) = -1.  Its result: score
f(e), count, last e, the span (q_b, y_e, t_b, x_e), and (min, max) of t - q over its anchors.  A read without anchors: score 0,
count 0, last None, zeros elsewhere.

Also here: the validation rules of the call, the greedy cut of a read list into ranges, a seeder over a dict of k-mers, and what
Context.map_reads makes of a chain (the text window and the band)."""
INVALID, CAPACITY = -1, -5
ANCHOR_BYTES, RECORD_BYTES = 20, 40   # device bytes per anchor (t, q, len, f, pred) and per read (its result record)


def beta(dd, gap_scale):
    return 0 if dd == 0 else ((gap_scale * dd) >> 8) + ((dd.bit_length() - 1) >> 1)


def link(a, b, max_dist, bandwidth, gap_scale):
    """what anchor b adds to a chain that ends in anchor a: alpha - beta, or None when a is not admissible before b"""
    dx, dy = b[0] + b[2] - a[0] - a[2], b[1] + b[2] - a[1] - a[2]
    dd = abs(dx - dy)
    if not (0 < dx <= max_dist and 0 < dy <= max_dist and dd <= bandwidth):
        return None
    return min(b[2], dx, dy) - beta(dd, gap_scale)


def dp(anchors, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38):
    """f and pred of one read's anchors"""
    f, pred = [], []
    for i, a in enumerate(anchors):
        best, bj = None, -1
        for j in range(max(0, i - lookback), i):
            g = link(anchors[j], a, max_dist, bandwidth, gap_scale)
            if g is not None and (best is None or f[j] + g >= best):   # >=: the largest j among equals
                best, bj = f[j] + g, j
        if best is not None and best > a[2]:
            f.append(best)
            pred.append(bj)
        else:
            f.append(a[2])
            pred.append(-1)
    return f, pred


def chain(anchors, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38, want_dp=True):
    """one read's result as Context.chain returns it"""
    anchors = [tuple(int(v) for v in a) for a in anchors]
    if not anchors:
        out = dict(score=0, count=0, last=None, q_begin=0, q_end=0, t_begin=0, t_end=0, diag_lo=0, diag_hi=0)
        if want_dp:
            out.update(f=[], pred=[])
        return out
    f, pred = dp(anchors, lookback, max_dist, bandwidth, gap_scale)
    e = f.index(max(f))
    walk = [e]
    while pred[walk[-1]] >= 0:
        assert pred[walk[-1]] < walk[-1]
        walk.append(pred[walk[-1]])
    b = walk[-1]
    diags = [anchors[i][0] - anchors[i][1] for i in walk]
    out = dict(score=f[e], count=len(walk), last=e, q_begin=anchors[b][1], q_end=anchors[e][1] + anchors[e][2], t_begin=anchors[b][0],
               t_end=anchors[e][0] + anchors[e][2], diag_lo=min(diags), diag_hi=max(diags))
    if want_dp:
        out.update(f=f, pred=pred)
    return out


def chain_many(reads, want_dp=True, **params):
    return [chain(a, want_dp=want_dp, **params) for a in reads]


def dp_many(reads, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38):
    """dp() of many reads in numpy, all reads in lockstep over the anchor index (for lists too large for the plain loop;
    test_chain_oracle.py holds it to dp()) -> [(f, pred)]"""
    import numpy as np
    R, counts = len(reads), np.array([len(a) for a in reads], dtype=np.int64)
    N = int(counts.max()) if R else 0
    X, Y, L = (np.zeros((R, N), dtype=np.int64) for _ in range(3))
    for r, a in enumerate(reads):
        if len(a):
            a = np.asarray(a, dtype=np.int64).reshape(-1, 3)
            X[r, :len(a)], Y[r, :len(a)], L[r, :len(a)] = a[:, 0] + a[:, 2], a[:, 1] + a[:, 2], a[:, 2]
    F, P = np.zeros((R, N), dtype=np.int64), np.full((R, N), -1, dtype=np.int64)
    NEG = -(1 << 60)
    for i in range(N):
        act = np.flatnonzero(counts > i)
        li = L[act, i]
        F[act, i] = li
        j0 = max(0, i - lookback)
        if j0 == i:
            continue
        dx, dy = X[act, i, None] - X[act, j0:i], Y[act, i, None] - Y[act, j0:i]
        dd = np.abs(dx - dy)
        adm = (dx > 0) & (dx <= max_dist) & (dy > 0) & (dy <= max_dist) & (dd <= bandwidth)
        bt = np.where(dd > 0, ((gap_scale * dd) >> 8) + ((np.frexp(np.maximum(dd, 1).astype(np.float64))[1] - 1) >> 1), 0)
        cand = np.where(adm, F[act, j0:i] + np.minimum(li[:, None], np.minimum(dx, dy)) - bt, NEG)[:, ::-1]
        a = np.argmax(cand, axis=1)   # the first maximum of the reversed window: the largest j
        best = cand[np.arange(len(act)), a]
        take = best > li
        F[act[take], i] = best[take]
        P[act[take], i] = i - 1 - a[take]
    return [(F[r, :counts[r]].tolist(), P[r, :counts[r]].tolist()) for r in range(R)]


def chain_from_dp(anchors, f, pred, want_dp=True):
    """chain()'s result from a DP computed elsewhere"""
    if not len(anchors):
        return chain([], want_dp=want_dp)
    e = f.index(max(f))
    walk = [e]
    while pred[walk[-1]] >= 0:
        walk.append(pred[walk[-1]])
    b = walk[-1]
    A = [tuple(int(v) for v in anchors[i]) for i in walk]
    out = dict(score=f[e], count=len(walk), last=e, q_begin=A[-1][1], q_end=A[0][1] + A[0][2], t_begin=A[-1][0], t_end=A[0][0] + A[0][2],
               diag_lo=min(a[0] - a[1] for a in A), diag_hi=max(a[0] - a[1] for a in A))
    if want_dp:
        out.update(f=f, pred=pred)
    return out


def chain_many_fast(reads, want_dp=True, **params):
    return [chain_from_dp(a, f, p, want_dp) for a, (f, p) in zip(reads, dp_many(reads, **params))]


def best_subsequence(anchors, max_dist, bandwidth, gap_scale):
    """the best score over ALL subsequences of the anchors (at most ~12 of them), a chain scored by the same alpha - beta terms"""
    n, best = len(anchors), 0
    for mask in range(1, 1 << n):
        idx = [i for i in range(n) if mask >> i & 1]
        s = anchors[idx[0]][2]
        for a, b in zip(idx, idx[1:]):
            g = link(anchors[a], anchors[b], max_dist, bandwidth, gap_scale)
            if g is None:
                s = None
                break
            s += g
        if s is not None:
            best = max(best, s)
    return best


def validate(reads, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38):
    """(code, first offending read or None) as pwa_chain_plan answers: parameters first, then the reads in order, and inside a read
    the count, then anchor by anchor a len of 0, an end at or beyond 2^31, the order, then the sum of len"""
    if not (1 <= lookback <= 512 and 1 <= max_dist <= 1 << 30 and 0 <= bandwidth <= 1 << 20 and 0 <= gap_scale <= 1024):
        return INVALID, None
    for r, anchors in enumerate(reads):
        if len(anchors) > 1 << 24:
            return CAPACITY, r
        prev = None
        for t, q, ln in anchors:
            if ln == 0:
                return INVALID, r
            if t + ln >= 1 << 31 or q + ln >= 1 << 31:
                return CAPACITY, r
            if prev is not None and (t + ln, q + ln) < prev:
                return INVALID, r
            prev = (t + ln, q + ln)
        if sum(a[2] for a in anchors) >= 1 << 30:
            return CAPACITY, r
    return 0, None


def ranges(counts, budget):
    """the greedy cut: consecutive reads as long as their bytes fit the budget, or one read that alone exceeds it (budget 0: no
    limit) -> [(first read, end read)] of the ranges that hold an anchor; a range of empty reads launches nothing and is left out"""
    out, k0, n = [], 0, len(counts)
    weight = lambda r: ANCHOR_BYTES * counts[r] + RECORD_BYTES
    while k0 < n:
        k1, tot = k0 + 1, weight(k0)
        while k1 < n and (not budget or tot + weight(k1) <= budget):
            tot += weight(k1)
            k1 += 1
        if any(counts[k0:k1]):
            out.append((k0, k1))
        k0 = k1
    return out


# ---- seeding and mapping

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def kmer_index(text, k):
    ix = {}
    for t in range(len(text) - k + 1):
        ix.setdefault(text[t:t + k], []).append(t)
    return ix


def seed(index, read, k, step=1, max_occ=64):
    """the anchors (t, q, k) of one read's k-mers at q = 0, step, ..., those of more than max_occ occurrences dropped, in (t, q) order"""
    out = []
    for q in range(0, len(read) - k + 1, step):
        hits = index.get(read[q:q + k], ())
        if len(hits) <= max_occ:
            out += [(t, q, k) for t in hits]
    return sorted(out)


def window_and_band(c, n, text_len, w):
    """what map_reads aligns a read of n symbols with chain c in: (window start, window end, band lo, band hi), or None where the band
    is wider than 4096 or fails the banded call's semi-global rule (band_hi >= 0 and n + band_lo <= m)"""
    if not c["count"]:
        return None
    ws = max(0, c["t_begin"] - c["q_begin"] - w)
    we = min(text_len, c["t_end"] + (n - c["q_end"]) + w)
    lo, hi = c["diag_lo"] - ws - w, c["diag_hi"] - ws + w
    if hi - lo + 1 > 4096 or hi < 0 or n + lo > we - ws:
        return None
    return ws, we, lo, hi


def mutate(rng, s, rate, alphabet=b"ACGT"):
    """s with about `rate` of its symbols edited: substitutions, insertions and deletions in equal parts"""
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < rate / 3:
            out.append(rng.choice([a for a in alphabet if a != c]))
        elif u < 2 * rate / 3:
            out.append(c)
            out.append(rng.choice(alphabet))
        elif u < rate:
            continue
        else:
            out.append(c)
    return bytes(out)


def random_text(rng, n, repeat=0, copies=2):
    """n random bases; with `repeat`, that many bases of it occur `copies` times, spread over the text"""
    t = bytearray(rng.choice(b"ACGT") for _ in range(n))
    if repeat:
        unit = bytes(t[:repeat])
        for c in range(1, copies):
            at = c * (n - repeat) // max(copies - 1, 1)
            t[at:at + repeat] = unit
    return bytes(t)


def planted_reads(rng, text, count, length, rate, both_strands=False):
    """[(read, planted start, strand)]: text[start:start + length] mutated at `rate`, and with both_strands every other one reversed"""
    out = []
    for i in range(count):
        ln = length if isinstance(length, int) else rng.randint(*length)
        at = rng.randrange(0, len(text) - ln + 1)
        r = mutate(rng, text[at:at + ln], rate)
        minus = both_strands and i % 2 == 1
        out.append((revcomp(r) if minus else r, at, "-" if minus else "+"))
    return out


def random_anchors(rng, n, span=400, max_len=20):
    """n anchors of one read, sorted as the call requires: a noisy diagonal with strays, overlaps and duplicates"""
    out = []
    for _ in range(n):
        q = rng.randrange(span)
        t = q + rng.choice([0, 0, 0, 1, -1, 3, rng.randrange(-span, span)]) + span
        out.append((t, q, rng.randint(1, max_len)))
    if n > 2 and rng.random() < 0.5:
        out[rng.randrange(n)] = out[rng.randrange(n)]
    return sorted(out, key=lambda a: (a[0] + a[2], a[1] + a[2]))


# ---- inputs where one far predecessor decides: every chunk of the kernel's window, every tie of its key maximum, every walk hop

def far_predecessor(d):
    """d + 1 anchors whose last one has exactly one admissible predecessor, anchor 0, d back: the d - 1 anchors between them end at
    the last anchor's text position (dx = 0), far off its diagonal, and have no predecessor themselves.  Under the default
    parameters (any bandwidth, any gap_scale) pred[-1] == 0 and f[-1] == 20 when d <= lookback, pred[-1] == -1 and f[-1] == 10
    otherwise, and every other pred is -1"""
    return [(100, 100, 10)] + [(129, 0, 1)] * (d - 1) + [(120, 120, 10)]


def equal_predecessor(d):
    """far_predecessor(d) with a last anchor that starts where anchor 0 starts and is twice as long: dx == dy == 10, so cand is
    10 + 10 == len of the last anchor, which is not enough: every pred is -1, f[-1] == 20 and the chain is the last anchor alone,
    whatever the lookback.  (A kernel that takes cand >= len would answer pred[-1] == 0 when d <= lookback)"""
    return [(100, 100, 10)] + [(119, 0, 1)] * (d - 1) + [(100, 100, 20)]


def ladder(d, n, bw=3, step=7, ln=5):
    """n anchors on d diagonals bw + 1 apart, taken in turn: anchor i is on diagonal 4000 - (i % d) * (bw + 1), text ends `step` apart.
    With bandwidth <= bw and gap_scale 0 the admissible predecessors of i are i - d, i - 2 d, ..., and i - d has the largest cand, so
    pred[i] == i - d and f[i] == ln * (i // d + 1) for every i >= d when d <= lookback, and every pred is -1 when d > lookback.  The
    chain of d <= lookback hops by exactly d on one diagonal: last == d * ((n - 1) // d), the smallest index of maximal f, and
    count == (n - 1) // d + 1; with n == 2 * d + 70 and d >= 70 that is last == 2 * d, the first of 70 equal f, and count == 3"""
    assert d >= 1 and (d - 1) * (bw + 1) < 4000 and step >= ln
    return [(step * i + 4000, step * i + (i % d) * (bw + 1), ln) for i in range(n)]


def two_way_tie(o1, o2, far_len=10):
    """o2 + 2 anchors whose last one, i, has exactly two admissible predecessors, i - 1 - o1 and i - 1 - o2 (o1 < o2), under
    bandwidth 1, gap_scale 0, max_dist 10000 and any lookback > o2.  The last anchor is on diagonal D, the two on D + 1 and D - 1,
    every other anchor alone on a diagonal 10 * (offset + 2) above D; text ends are 12 apart and len is 10, so alpha is len.  The
    nearer one has len 10, the farther one far_len: with 10 the two cand are equal and pred[-1] is the nearer one, n - 2 - o1, with
    f[-1] == 20; with 11 the farther one wins, pred[-1] == n - 2 - o2 == 0 and f[-1] == 21.  Every other pred is -1"""
    assert 0 <= o1 < o2 <= 511 and far_len >= 1
    n, D, out = o2 + 2, 100, []
    for k in range(n):
        o = n - 2 - k   # the offset in the last anchor's window; -1: the last anchor itself
        diag, ln = (D, 10) if o < 0 else (D + 1, 10) if o == o1 else (D - 1, far_len) if o == o2 else (D + 10 * (o + 2), 10)
        x = 6000 + 12 * k
        out.append((x - ln, x - diag - ln, ln))
    return out


EDGE_LOOKBACKS = [1, 63, 64, 65, 127, 128, 129, 192, 255, 256, 257, 448, 511, 512]   # both sides of every kernel_for threshold
EDGE_PARAMS = dict(bandwidth=3, gap_scale=0)
WALK_HOPS = [64, 65, 200, 512]
TIE_OFFSETS = [(0, 1), (1, 2), (2, 3), (3, 4), (7, 8), (15, 16), (31, 32), (47, 48), (63, 64), (64, 127), (127, 128), (5, 300), (255, 256),
               (510, 511), (0, 511)]   # the two lanes in one quad, two quads, two halves of a row, two rows, two chunks
TIE_PARAMS = dict(bandwidth=1, gap_scale=0, max_dist=10000)   # every builder above keeps its promise under these, too
_far = {}


def chunks_of(lookback):
    """the C of the chain_kernel<C> that kernel_for(lookback) picks"""
    return 1 if lookback <= 64 else 2 if lookback <= 128 else 4 if lookback <= 256 else 8


def ladder_with_tail():
    """ladder(512, 1100) and then 100 anchors in a row on a far diagonal: the best chain is the tail, whole, and never enters the ladder"""
    return ladder(512, 1100) + [(30000 + 5 * k, 5 * k, 5) for k in range(100)]


def repeat_reads():
    """60 planted reads of 300 .. 2000 symbols at 5 % on a 40 kb text that holds a 500-base unit 8 times, seeded with k = 12, step 1,
    max_occ 64: where a read meets the unit its anchors come in eights, and predecessors far back in the window compete"""
    if "repeat" not in _far:
        import random
        rng = random.Random(41)
        text = random_text(rng, 40000, repeat=500, copies=8)
        index = kmer_index(text, 12)
        _far["repeat"] = [seed(index, read, 12, 1, 64) for read, _, _ in planted_reads(rng, text, 60, (300, 2000), 0.05)]
    return _far["repeat"]


def far_cases():
    """the calls of test_gpu_chain.py's far-window tests, built without a GPU: [dict(name, params, reads, labels)], labels[r] naming
    the builder and the arguments of reads[r] -- ("far", d), ("ladder", d, n), ("equal", d), ("tie", o1, o2, far_len), ("tail",),
    ("seeded",), ("few",) -- so that a test can hold the call's result to what the builder promises (test_chain_oracle.py holds the list itself
    to the oracle and shows which mistakes in the recurrence it catches)"""
    if "cases" in _far:
        return _far["cases"]
    cases = []
    for H in EDGE_LOOKBACKS:
        ds = [d for d in sorted({1, H - 1, H, H + 1}) if d >= 1]
        cases.append(dict(name="edges-%d" % H, params=dict(EDGE_PARAMS, lookback=H),
                          reads=[r for d in ds for r in (far_predecessor(d), ladder(d, 2 * d + 70), equal_predecessor(d))],
                          labels=[l for d in ds for l in (("far", d), ("ladder", d, 2 * d + 70), ("equal", d))]))
    cases.append(dict(name="walk", params=dict(EDGE_PARAMS, lookback=512), reads=[ladder(d, 5 * d + 3) for d in WALK_HOPS] + [ladder_with_tail()],
                      labels=[("ladder", d, 5 * d + 3) for d in WALK_HOPS] + [("tail",)]))
    ties = [(o1, o2, fl) for o1, o2 in TIE_OFFSETS for fl in (10, 11)]
    cases.append(dict(name="ties", params=dict(TIE_PARAMS, lookback=512), reads=[two_way_tie(*t) for t in ties], labels=[("tie",) + t for t in ties]))
    for C in (1, 2, 4, 8):   # the farther candidate in the window's last slot: one call per lookback, in the order of the kernels
        for H in sorted({o2 + 1 for _, o2 in TIE_OFFSETS if chunks_of(o2 + 1) == C}):
            own = [t for t in ties if t[1] + 1 == H]
            cases.append(dict(name="ties-%d" % H, params=dict(TIE_PARAMS, lookback=H), reads=[two_way_tie(*t) for t in own], labels=[("tie",) + t for t in own]))
    import random
    seen, mixed = set(), []
    for c in cases:   # every read above, once
        for a, l in zip(c["reads"], c["labels"]):
            if l not in seen:
                seen.add(l)
                mixed.append((a, l))
    random.Random(7).shuffle(mixed)
    few = [[], [(7, 3, 5)], [], [(0, 0, 1)]]
    mixed = [p for i, m in enumerate(mixed) for p in ([m, (few[i // 3 % 4], ("few",))] if i % 3 == 0 else [m])]
    cases.append(dict(name="mixed", params=dict(TIE_PARAMS, lookback=512), reads=[a for a, _ in mixed], labels=[l for _, l in mixed]))
    for H in (200, 512):
        cases.append(dict(name="seeded-%d" % H, params=dict(lookback=H), reads=repeat_reads(), labels=[("seeded",)] * len(repeat_reads())))
    _far["cases"] = cases
    return cases
