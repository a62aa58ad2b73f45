"""Banded X-drop extension (pwa_extend_banded_batch and pwa_extend_banded_subst_batch, include/pwalign.h: "EXT") restated in numpy:
the test-side oracle of the feature.

The matrix is banded_oracle's NW matrix, and `fill` is that module's; what is new is what is read from it: per row the maximum over
the in-band cells with j >= 1 and its first column (rmax / rcol of the fill), the best-cell record over the rows in order (replaced
on a strictly larger value only, started as score 0 at (0, 0)), the X-drop stop rule, NW's walk from the end cell, and the
pattern-end result: (rmax(n), its first column) when rows == n >= 1, (0, 0) for an empty pattern, None otherwise.  None of these
depends on the kind of scoring; `sc` is gotoh_oracle's scoring value.  scalar_dp is the same contract once more as a plain
three-matrix DP, cell by cell."""
import numpy as np

import banded_oracle as BO
import gotoh_oracle as go_

NEG = BO.NEG
_LOW = NEG // 2
MAX_XDROP = 1 << 27
NO_PEND = None


def band_valid(n, m, lo, hi):
    """the validity rule of include/pwalign.h: the anchor (0, 0) is in the band"""
    return lo <= 0 <= hi


def fill(pairs, bands, sc, go, ge):
    return BO.fill(pairs, bands, "nw", sc, go, ge)


def record(rmax, rcol, n, xdrop):
    """the best-cell record and the stop rule over one pair's rows -> (score, (i, j), rows)"""
    rm = rmax[1:n + 1]
    has = rm > _LOW
    before = np.maximum.accumulate(np.concatenate([[0], np.where(has, rm, 0)]))[:n]   # best(i - 1), were no row to stop
    if xdrop >= 0:
        stops = ~has | (rm < before - xdrop)
        rows = int(np.argmax(stops)) if stops.any() else n
    else:
        rows = int(np.nonzero(has)[0][-1]) + 1 if has.any() else 0
    if rows == 0:
        return 0, (0, 0), 0
    seen = np.where(has[:rows], rm[:rows], NEG)
    x = int(np.argmax(seen))   # the first maximum
    if seen[x] <= 0:
        return 0, (0, 0), rows
    return int(seen[x]), (x + 1, int(rcol[x + 1])), rows


def pattern_end(rmax, rcol, n, m, rows):
    """the pattern-end result of one pair from its row records and its rows_out -> (score, j) or None"""
    if n == 0:
        return (0, 0)
    if m == 0 or rows != n:
        return NO_PEND
    assert rmax[n] > _LOW and rcol[n] >= 1   # rows == n: row n has an in-band cell with j >= 1
    return (int(rmax[n]), int(rcol[n]))


def result(tab, g, n, m, xdrop):
    if n == 0 or m == 0:
        return dict(score=0, end=(0, 0), start=(0, 0), ops=b"", rows=0, pend=pattern_end(None, None, n, m, 0))
    score, end, rows = record(tab["rmax"][g], tab["rcol"][g], n, xdrop)
    ops, start = BO.walk(tab, g, "nw", end[0], end[1])
    return dict(score=score, end=end, start=start, ops=ops, rows=rows, pend=pattern_end(tab["rmax"][g], tab["rcol"][g], n, m, rows))


def extend_multi(pairs, bands, sc, go, ge, xdrops, group=64):
    """[(p, t)], [(lo, hi)] (valid bands), several drops over one fill -> {xdrop: [dict(score, end, start, ops, rows, pend)]}"""
    out = {xd: [None] * len(pairs) for xd in xdrops}
    live = []
    for k, (p, t) in enumerate(pairs):
        if len(p) and len(t):
            live.append(k)
        else:
            for xd in xdrops:
                out[xd][k] = result(None, 0, len(p), len(t), xd)
    live.sort(key=lambda k: (len(pairs[k][0]), bands[k][1] - bands[k][0]))
    for a in range(0, len(live), group):
        kk = live[a:a + group]
        tab = fill([pairs[k] for k in kk], [bands[k] for k in kk], sc, go, ge)
        for g, k in enumerate(kk):
            for xd in xdrops:
                out[xd][k] = result(tab, g, len(pairs[k][0]), len(pairs[k][1]), xd)
    return out


def extend_many(pairs, bands, sc, go, ge, xdrop, group=64):
    return extend_multi(pairs, bands, sc, go, ge, [xdrop], group)[xdrop]


def extend(p, t, band, sc, go, ge, xdrop):
    return extend_many([(p, t)], [band], sc, go, ge, xdrop)[0]


def scalar_dp(p, t, band, sc, go, ge, xdrop, matrix=False):
    """Plain three-matrix DP of the same contract, float -inf, cell by cell, rows in order with the stop test after each (small
    pairs) -> dict(score, end, start, ops, rows, pend); matrix=True: also H of every row (no stop applied), under "H" """
    cell = go_.scorer(sc)[1]
    n, m = len(p), len(t)
    if n == 0 or m == 0:
        return dict(score=0, end=(0, 0), start=(0, 0), ops=b"", rows=0, pend=(0, 0) if n == 0 else NO_PEND)
    lo, hi = band
    oe = go + ge
    inf = float("-inf")
    inb = lambda i, j: lo <= j - i <= hi
    H = [[inf] * (m + 1) for _ in range(n + 1)]
    E = [[inf] * (m + 1) for _ in range(n + 1)]
    F = [[inf] * (m + 1) for _ in range(n + 1)]
    src = [[0] * (m + 1) for _ in range(n + 1)]
    eop = [[False] * (m + 1) for _ in range(n + 1)]
    fop = [[False] * (m + 1) for _ in range(n + 1)]
    for j in range(0, m + 1):
        if lo <= 0 and j <= hi:
            H[0][j] = go + j * ge if j else 0
    best, end, rows, stopped, pend = 0, (0, 0), 0, False, NO_PEND
    for i in range(1, n + 1):
        if hi >= 0 and -i >= lo:
            H[i][0] = go + i * ge
        rmax, rj = inf, 0
        for j in range(1, m + 1):
            if not inb(i, j):
                continue
            eo, ee = H[i][j - 1] + oe, E[i][j - 1] + ge
            E[i][j], eop[i][j] = (eo, True) if eo >= ee else (ee, False)
            fo, fe = H[i - 1][j] + oe, F[i - 1][j] + ge
            F[i][j], fop[i][j] = (fo, True) if fo >= fe else (fe, False)
            d = H[i - 1][j - 1] + cell(p[i - 1], t[j - 1])
            h = max(d, E[i][j], F[i][j])
            src[i][j] = BO.SRC_D if d == h else BO.SRC_E if E[i][j] == h else BO.SRC_F
            H[i][j] = h
            if h > rmax:
                rmax, rj = h, j
        if stopped:
            continue
        if xdrop >= 0 and rmax < best - xdrop:   # (-inf < anything: a row without a cell stops)
            stopped = True
            if not matrix:
                break
            continue
        if rmax > inf:
            rows = i
            if i == n:   # row n was kept and has a cell: the pattern-end result
                pend = (int(rmax), rj)
        if rmax > best:
            best, end = rmax, (i, rj)
    if xdrop >= 0 and not stopped:
        rows = n
    tab = dict(src=np.array(src), eop=np.array(eop), fop=np.array(fop))
    ops, start = go_.walk(tab, "nw", end[0], end[1])
    out = dict(score=int(best), end=end, start=start, ops=ops, rows=rows, pend=pend)
    if matrix:
        out["H"] = H
    return out
