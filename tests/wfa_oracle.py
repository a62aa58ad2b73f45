"""Wavefront (WFA) affine-gap global alignment (pwa_scores_wfa, pwa_align_wfa_batch; include/pwalign.h) restated in numpy: the test-side
oracle of the feature.

The sweep is by penalty s, not by cell.  With x, o, e the reduced penalties of a mismatch, a gap open and a gap extend (`penalties`),
a wavefront holds per diagonal k = j - i the furthest text offset j reachable with penalty s, in three states:
    I[s][k] = max(M[s-o-e][k-1], I[s-e][k-1]) + 1
    D[s][k] = max(M[s-o-e][k+1], D[s-e][k+1])
    M[s][k] = extend(max(M[s-x][k] + 1, I[s][k], D[s][k]))
every term trimmed to 0 <= j <= m and 0 <= j - k <= n (NULL otherwise) before the max is taken.  Wavefront s spans the diagonals
[max(-n, -khi(s)), min(m, khi(s))]; a score whose three source wavefronts are all empty is empty itself and is skipped.  The sweep ends
at the first s with M[s][m - n] == m, and the backtrace walks the stored wavefronts with the tie rules mismatch >= I >= D in state M
and "a tie opens" in states I and D."""
from math import gcd

import numpy as np

NEG = -(1 << 40)   # NULL: below every offset, never wraps in int64


def _arr(x):
    return np.frombuffer(bytes(x), dtype=np.uint8)


def penalties(match, mismatch, go, ge):
    """(x, o, e, g), or ValueError where the header says PWA_E_INVALID"""
    if go > 0 or ge > 0 or match <= mismatch or match - 2 * ge <= 0:
        raise ValueError("scoring without a penalty form")
    x0, o0, e0 = 2 * (match - mismatch), -2 * go, match - 2 * ge
    g = gcd(gcd(x0, o0), e0)
    return x0 // g, o0 // g, e0 // g, g


def in_range(n, m, match, mismatch, go, ge):
    return (n + m + 2) * max(abs(match), abs(mismatch), abs(go) + abs(ge)) < 1 << 28


def khi(s, o, e):
    return 0 if s < o + e else (s - o) // e


def span(s, n, m, o, e):
    h = khi(s, o, e)
    return max(-n, -h), min(m, h)


def width(s, n, m, o, e):
    lo, hi = span(s, n, m, o, e)
    return hi - lo + 1


def cells_to(p, n, m, o, e):
    """sum of width(s) over s = 0 .. p"""
    s = np.arange(p + 1, dtype=np.int64)
    h = np.where(s < o + e, 0, (s - o) // e)
    return int((np.minimum(h, n) + np.minimum(h, m) + 1).sum())


def plan(n, m, match, mismatch, go, ge, min_score=None):
    """-> (p_max, cells); (None, 0) for a pair the host already knows is not found"""
    x, o, e, g = penalties(match, mismatch, go, ge)
    p_max = (o + n * e if n else 0) + (o + m * e if m else 0)
    if min_score is not None:
        p_max = min(p_max, (match * (n + m) - 2 * min_score) // g)
    if p_max < 0 or (n != m and p_max < o + abs(n - m) * e):
        return None, 0
    return p_max, cells_to(p_max, n, m, o, e)


def score_of(pen, n, m, match, g):
    v = match * (n + m) - g * pen
    assert v % 2 == 0
    return v // 2


def _runs(p, t):
    """R[i][j] = the number of equal symbols p[i + r] == t[j + r], r = 0, 1, ..: what an extend from (i, j) adds; zero on the rim"""
    n, m = len(p), len(t)
    R = np.zeros((n + 2, m + 2), dtype=np.int64)
    if n and m:
        eq = p[:, None] == t[None, :]
        for i in range(n - 1, -1, -1):
            R[i, :m] = np.where(eq[i], R[i + 1, 1:m + 1] + 1, 0)
    return R


def sweep(p, t, pen, p_max):
    """-> (P or None, wavefronts): wavefronts[s] = (M, I, D) for every non-empty score s <= P, each an array over the diagonals
    -n - 1 .. m + 1 (diagonal k at index k + n + 1; the two outermost never hold an offset)"""
    p, t = _arr(p), _arr(t)
    n, m = len(p), len(t)
    x, o, e = pen
    K = np.arange(-n - 1, m + 2, dtype=np.int64)
    none = np.full(len(K), NEG, dtype=np.int64)
    pad = np.full(1, NEG, dtype=np.int64)
    R = _runs(p, t)
    W = {}
    for s in range(p_max + 1):
        wx, wo, we = W.get(s - x), W.get(s - o - e), W.get(s - e)
        if s and wx is None and wo is None and we is None:
            continue
        if s == 0:
            I = D = none
            pre = none.copy()
            pre[n + 1] = 0
        else:
            gi = none if wo is None and we is None else wo[0] if we is None else we[1] if wo is None else np.maximum(wo[0], we[1])
            gd = none if wo is None and we is None else wo[0] if we is None else we[2] if wo is None else np.maximum(wo[0], we[2])
            J = np.stack([none if wx is None else wx[0] + 1, np.concatenate([pad, gi[:-1] + 1]), np.concatenate([gd[1:], pad])])
            i = J - K
            J = np.where((J >= 0) & (J <= m) & (i >= 0) & (i <= n), J, NEG)   # the trim, on every term
            I, D = J[1], J[2]
            pre = J.max(axis=0)
        ok = pre >= 0
        j = np.where(ok, pre, 0)
        M = np.where(ok, pre + R[np.where(ok, pre - K, 0), j], NEG)
        W[s] = (M, I, D)
        if M[m - n + n + 1] == m:
            return s, W
    return None, W


def backtrace(W, pen, P, n, m):
    """ops in traceback order"""
    x, o, e = pen

    def get(s, which, k):
        w = W.get(s)
        return NEG if w is None else int(w[which][k + n + 1])

    ops = bytearray()
    s, k, j, st = P, m - n, m, 0
    while True:
        if st == 0:
            if s == 0:
                assert k == 0
                ops += b"M" * j
                return bytes(ops)
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
            if get(s - o - e, 0, k - 1) >= get(s - e, 1, k - 1):   # a tie opens
                s, st = s - o - e, 0
            else:
                s = s - e
            k, j = k - 1, j - 1
        else:
            ops += b"D"
            if get(s - o - e, 0, k + 1) >= get(s - e, 2, k + 1):
                s, st = s - o - e, 0
            else:
                s = s - e
            k = k + 1


def align(p, t, match, mismatch, go, ge, min_score=None, want_ops=True):
    """-> dict(score, penalty, ops, cells): score / penalty None and ops b"" for a pair not found; cells as pwa_wfa_last_stats counts them"""
    x, o, e, g = penalties(match, mismatch, go, ge)
    n, m = len(p), len(t)
    p_max, _ = plan(n, m, match, mismatch, go, ge, min_score)
    if p_max is None:
        return dict(score=None, penalty=None, ops=b"", cells=0)
    P, W = sweep(p, t, (x, o, e), p_max)
    if P is None:
        return dict(score=None, penalty=None, ops=b"", cells=cells_to(p_max, n, m, o, e))
    out = dict(score=score_of(P, n, m, match, g), penalty=P, cells=cells_to(P, n, m, o, e))
    if want_ops:
        out["ops"] = backtrace(W, (x, o, e), P, n, m)
    return out
