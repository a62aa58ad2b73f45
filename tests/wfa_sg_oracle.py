"""Semi-global wavefront alignments (pwa_scores_wfa_sg, pwa_align_wfa_sg_batch; include/pwalign.h, "Semi-global wavefront alignments")
restated in numpy: the test-side oracle of the feature.  The whole pattern against any substring of the text, both text ends free.

Penalties are counted per PATTERN symbol (every one is consumed, so n = matches + mismatches + 'D'), not on the global calls' 2x scale:
    x0 = match - mismatch   o0 = -gap_open   eI0 = -gap_extend   eD0 = match - gap_extend      score = match n - g P
A run of L 'I' costs o + L eI, a run of L 'D' costs o + L eD, a skipped text prefix or suffix nothing.  The wavefronts of wfa_oracle.py
with two extend penalties:
    I[s][k] = max(M[s-o-eI][k-1], I[s-eI][k-1]) + 1
    D[s][k] = max(M[s-o-eD][k+1], D[s-eD][k+1])
    M[s][k] = extend(max(M[s-x][k] + 1, I[s][k], D[s][k]))          M[0][k] = extend(k) for k = 0 .. m
Wavefront s spans [max(-n, -khD(s)), m].  The sweep ends at the first s at which a diagonal holds an offset with j - k = n, on the
LOWEST such diagonal (the first maximum of row n: gotoh_oracle's end rule for "sg"); the backtrace stops at s = 0 on a diagonal
0 .. m, the start cell (0, k)."""
from math import gcd

import numpy as np

import wfa_oracle as WO

NEG = WO.NEG
in_range = WO.in_range


def penalties(match, mismatch, go, ge):
    """(x, o, eI, eD, g), or ValueError where the header says PWA_E_INVALID"""
    if go > 0 or ge >= 0 or match <= mismatch or match - ge <= 0:
        raise ValueError("scoring without a semi-global penalty form")
    x0, o0, i0, d0 = match - mismatch, -go, -ge, match - ge
    g = gcd(gcd(x0, o0), gcd(i0, d0))
    return x0 // g, o0 // g, i0 // g, d0 // g, g


def khd(s, o, ed):
    return 0 if s < o + ed else (s - o) // ed


def span(s, n, m, o, ed):
    return max(-n, -khd(s, o, ed)), m


def width(s, n, m, o, ed):
    return m + 1 + min(n, khd(s, o, ed))


def cells_to(p, n, m, o, ed):
    """sum of width(s) over s = 0 .. p, term by term"""
    s = np.arange(p + 1, dtype=np.int64)
    h = np.where(s < o + ed, 0, (s - o) // ed)
    return int((np.minimum(h, n) + m + 1).sum())


def p_worst(n, m, x, o, ed):
    if n == 0:
        return 0
    return min(o + n * ed, n * x) if m >= n else o + n * ed


def plan(n, m, match, mismatch, go, ge, min_score=None):
    """-> (p_max, cells); (None, 0) for a pair the host already knows is not found"""
    x, o, ei, ed, g = penalties(match, mismatch, go, ge)
    p_max = p_worst(n, m, x, o, ed)
    if min_score is not None:
        p_max = min(p_max, (match * n - min_score) // g)
    if p_max < 0 or (n > m and p_max < o + (n - m) * ed):
        return None, 0
    return p_max, cells_to(p_max, n, m, o, ed)


def score_of(pen, n, match, g):
    return match * n - g * pen


def sweep(p, t, pen, p_max):
    """-> (P or None, k_end, wavefronts): wavefronts[s] = (M, I, D) for every non-empty score s <= P over the diagonals -n - 1 .. m + 1
    (diagonal k at index k + n + 1), as wfa_oracle.sweep keeps them"""
    p, t = WO._arr(p), WO._arr(t)
    n, m = len(p), len(t)
    x, o, ei, ed = pen
    K = np.arange(-n - 1, m + 2, dtype=np.int64)
    none = np.full(len(K), NEG, dtype=np.int64)
    pad = none[:1]
    R = WO._runs(p, t)
    W = {}

    def pick(a, b, which):   # max(M of a, I or D of b), either wavefront may be missing
        if a is None and b is None:
            return none
        if b is None:
            return a[0]
        if a is None:
            return b[which]
        return np.maximum(a[0], b[which])

    for s in range(p_max + 1):
        wx, woi, wi, wod, wd = W.get(s - x), W.get(s - o - ei), W.get(s - ei), W.get(s - o - ed), W.get(s - ed)
        if s and wx is None and woi is None and wi is None and wod is None and wd is None:
            continue
        if s == 0:
            I = D = none
            pre = np.where((K >= 0) & (K <= m), K, NEG)
        else:
            gi, gd = pick(woi, wi, 1), pick(wod, wd, 2)
            J = np.stack([none if wx is None else wx[0] + 1, np.concatenate([pad, gi[:-1] + 1]), np.concatenate([gd[1:], pad])])
            i = J - K
            J = np.where((J >= 0) & (J <= m) & (i >= 0) & (i <= n), J, NEG)   # the trim, on every term
            I, D = J[1], J[2]
            pre = J.max(axis=0)
        ok = pre >= 0
        j = np.where(ok, pre, 0)
        M = np.where(ok, pre + R[np.where(ok, pre - K, 0), j], NEG)
        W[s] = (M, I, D)
        hit = np.nonzero((M >= 0) & (M - K == n))[0]
        if len(hit):
            return s, int(K[hit[0]]), W
    return None, None, W


def offsets_inside_the_span(W, pen, n, m):
    """no wavefront holds an offset left of its planned span"""
    x, o, ei, ed = pen
    for s, planes in W.items():
        lo, hi = span(s, n, m, o, ed)
        for a in planes:
            live = np.nonzero(a >= 0)[0] - (n + 1)
            if len(live) and (live.min() < lo or live.max() > hi):
                return False
    return True


def backtrace(W, pen, P, k_end, n, m):
    """-> (ops in traceback order, start diagonal)"""
    x, o, ei, ed = pen

    def get(s, which, k):
        w = W.get(s)
        return NEG if w is None or not -n - 1 <= k <= m + 1 else int(w[which][k + n + 1])

    ops = bytearray()
    s, k, j, st = P, k_end, n + k_end, 0
    while True:
        if st == 0:
            if s == 0:
                assert 0 <= k <= m and j >= k
                ops += b"M" * (j - k)
                return bytes(ops), k
            X = get(s - x, 0, k)
            X = X + 1 if X >= 0 and X + 1 <= m and X + 1 - k <= n else NEG
            I, D = get(s, 1, k), get(s, 2, k)
            v = max(X, I, D)
            assert 0 <= v <= j
            ops += b"M" * (j - v)
            if X == v:      # ties: mismatch >= I >= D
                ops += b"M"
                s, j = s - x, v - 1
            elif I == v:
                st, j = 1, v
            else:
                st, j = 2, v
        elif st == 1:
            ops += b"I"
            if get(s - o - ei, 0, k - 1) >= get(s - ei, 1, k - 1):   # a tie opens
                s, st = s - o - ei, 0
            else:
                s = s - ei
            k, j = k - 1, j - 1
        else:
            ops += b"D"
            if get(s - o - ed, 0, k + 1) >= get(s - ed, 2, k + 1):
                s, st = s - o - ed, 0
            else:
                s = s - ed
            k = k + 1


NOT_FOUND = dict(score=None, penalty=None, end=(0, 0), start=(0, 0), ops=b"")


def align(p, t, match, mismatch, go, ge, min_score=None, want_ops=True):
    """-> dict(score, penalty, end, start, ops, cells): score / penalty None, ops b"" and both cells (0, 0) for a pair not found; cells
    as pwa_wfa_last_stats counts them"""
    x, o, ei, ed, g = penalties(match, mismatch, go, ge)
    n, m = len(p), len(t)
    p_max, _ = plan(n, m, match, mismatch, go, ge, min_score)
    if p_max is None:
        return dict(NOT_FOUND, cells=0)
    P, k_end, W = sweep(p, t, (x, o, ei, ed), p_max)
    if P is None:
        return dict(NOT_FOUND, cells=cells_to(p_max, n, m, o, ed))
    out = dict(score=score_of(P, n, match, g), penalty=P, end=(n, n + k_end), cells=cells_to(P, n, m, o, ed))
    if want_ops:
        out["ops"], k0 = backtrace(W, (x, o, ei, ed), P, k_end, n, m)
        out["start"] = (0, k0)
    return out
