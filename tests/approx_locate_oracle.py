"""Start positions and locally minimal ends of k-edit hits (include/pwalign.h, pwa_approx_starts / pwa_approx_minima) restated in
numpy: the test-side oracle, on top of approx_oracle.py.

The start of a hit (e, d) of pattern p is the largest s <= e with ed(p, text[s:e]) <= d.  Reversing both strings turns "largest start"
into "first end": with D'[0][j] = j (the anchored form), D'[m][j] of p reversed against text[:e] reversed is ed(p, text[e - j:e])."""
import numpy as np

import approx_oracle as AO


def anchored_row(p, t):
    """D'[m][0 .. n] of pattern p against text t with D'[0][j] = j, D'[i][0] = i: last_row with the first row 0 .. n (int64)"""
    p, t = AO._arr(p), AO._arr(t)
    n = len(t)
    idx = np.arange(n + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, len(p) + 1):
        x = np.empty(n + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(prev[:-1] + (t != p[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(x - idx) + idx
    return prev


def start_of(p, text, e, d):
    """the start of hit (e, d), or None where no substring that ends at e lies within d of p"""
    m = len(p)
    lo = max(0, e - m - d)
    row = anchored_row(bytes(p)[::-1], bytes(text[lo:e])[::-1])
    at = np.nonzero(row == d)[0]   # row m moves by +-1 per column from m >= d down: the first index of d is the first value <= d
    return e - int(at[0]) if len(at) else None


def minima_from_row(row, k):
    """[(end, dist)] of the locally minimal ends within k, from the FULL last row D[m][0 .. n] (row[0] = m): the leftmost end of
    every plateau that is entered by a descent and left by a rise, the text end counting as a rise."""
    row = [int(x) for x in row]
    n = len(row) - 1
    out = []
    e = 1
    while e <= n:
        f = e
        while f < n and row[f + 1] == row[e]:
            f += 1
        if row[e] <= k and row[e - 1] > row[e] and (f == n or row[f + 1] > row[e]):
            out.append((e, row[e]))
        e = f + 1
    return out


def minima_from_hits(hit_list, m, k, n):
    """the definition of pwa_approx_minima on the hit list alone: c(e) = dist of the hit at e, min(k, m) + 1 for an end without one,
    c(0) = m"""
    above = min(k, m) + 1
    c = {e: d for e, d in hit_list}
    c[0] = m
    out = []
    for e, d in hit_list:
        if c.get(e - 1, above) <= d:
            continue
        f = e
        while f < n and c.get(f + 1, above) == d:
            f += 1
        if f == n or c.get(f + 1, above) > d:
            out.append((e, d))
    return out
