"""Banded X-drop extension (pwa_extend_banded_batch, include/pwalign.h: "EXT") restated in numpy: the test-side oracle of the feature.

The matrix is banded_oracle's NW matrix, filled the same way in band coordinates (slot x of row i = cell (i, i + lo + x)); what is new
is what is read from it: per row the maximum over the in-band cells with j >= 1 and its first column, the best-cell record over the
rows in order (replaced on a strictly larger value only, started as score 0 at (0, 0)), the X-drop stop rule, and NW's walk from the
end cell.  scalar_dp is the same contract once more as a plain three-matrix DP, cell by cell."""
import numpy as np

import banded_oracle as BO
import gotoh_oracle as go_

NEG = BO.NEG
_LOW = NEG // 2
MAX_XDROP = 1 << 27


def band_valid(n, m, lo, hi):
    """the validity rule of include/pwalign.h: the anchor (0, 0) is in the band"""
    return lo <= 0 <= hi


def fill(pairs, bands, match, mismatch, go, ge):
    """banded_oracle.fill's NW tables (src, eop, fop, lo, W), and per pair and row i: rmax (the maximum of H over the in-band cells
    with j >= 1, NEG when there is none) and rcol (its first column)"""
    G = len(pairs)
    ns = np.array([len(p) for p, _ in pairs], dtype=np.int64)
    ms = np.array([len(t) for _, t in pairs], dtype=np.int64)
    lo = np.array([b[0] for b in bands], dtype=np.int64)
    hi = np.array([b[1] for b in bands], dtype=np.int64)
    lo = np.minimum(np.maximum(lo, -ns), ms)
    hi = np.maximum(np.minimum(hi, ms), -ns)
    W = hi - lo + 1
    B = int(W.max())
    nmax, mmax = int(ns.max()), int(ms.max())
    P = np.zeros((G, max(nmax, 1)), dtype=np.int16)
    T = np.full((G, max(mmax, 1)), -1, dtype=np.int16)
    for g, (p, t) in enumerate(pairs):
        P[g, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        T[g, :len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
    oe = go + ge
    xs = np.arange(B, dtype=np.int64)[None, :]
    src = np.zeros((G, nmax + 1, B), dtype=np.uint8)
    eop = np.zeros((G, nmax + 1, B), dtype=bool)
    fop = np.zeros((G, nmax + 1, B), dtype=bool)
    rmax = np.full((G, nmax + 1), NEG, dtype=np.int64)
    rcol = np.zeros((G, nmax + 1), dtype=np.int64)
    rows = np.arange(G)
    Hp = Fp = None
    neg1 = np.full((G, 1), NEG, dtype=np.int64)
    for i in range(0, nmax + 1):
        j = i + lo[:, None] + xs
        inb = (xs < W[:, None]) & (j >= 0) & (j <= ms[:, None]) & (i <= ns[:, None])
        if i == 0:
            H = np.where(inb & (lo[:, None] <= 0), (go + j * ge) * (j > 0), NEG).astype(np.int64)
            F = np.full((G, B), NEG, dtype=np.int64)
        else:
            up_h = np.concatenate([Hp[:, 1:], neg1], axis=1)
            up_f = np.concatenate([Fp[:, 1:], neg1], axis=1)
            tsym = T[rows[:, None], np.clip(j - 1, 0, max(mmax, 1) - 1)]
            s = np.where(P[:, i - 1:i] == tsym, match, mismatch).astype(np.int64)
            diag = Hp + s
            fo, fe = up_h + oe, up_f + ge
            F = np.maximum(fo, fe)
            fopen = fo >= fe
            A = np.maximum(diag, F)
            col0 = j == 0
            A = np.where(col0, np.where(inb & (hi[:, None] >= 0), go + i * ge, NEG), A)
            A = np.where(inb, A, NEG)
            A = np.where(A < _LOW, NEG, A)
            cm = np.maximum.accumulate(A - j * ge, axis=1)
            cm = np.concatenate([neg1, cm[:, :-1]], axis=1)
            E = (j - 1) * ge + oe + cm
            E = np.where(inb & ~col0 & (E > _LOW), E, NEG)
            H = np.where(col0, A, np.maximum(A, E))
            F = np.where(inb & ~col0 & (F > _LOW), F, NEG)
            hl = np.concatenate([neg1, H[:, :-1]], axis=1)
            el = np.concatenate([neg1, E[:, :-1]], axis=1)
            eop[:, i, :] = hl + oe >= el + ge
            fop[:, i, :] = fopen
            src[:, i, :] = np.where(diag == H, BO.SRC_D, np.where(E == H, BO.SRC_E, BO.SRC_F))
            Hc = np.where(inb & (j >= 1) & (H > _LOW), H, NEG)
            rmax[:, i] = Hc.max(axis=1)
            rcol[:, i] = i + lo + np.argmax(Hc == rmax[:, i:i + 1], axis=1)
        Hp, Fp = H, F
    return dict(src=src, eop=eop, fop=fop, lo=lo, W=W, rmax=rmax, rcol=rcol)


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


def result(tab, g, n, m, xdrop):
    if n == 0 or m == 0:
        return dict(score=0, end=(0, 0), start=(0, 0), ops=b"", rows=0)
    score, end, rows = record(tab["rmax"][g], tab["rcol"][g], n, xdrop)
    ops, start = BO.walk(tab, g, "nw", end[0], end[1])
    return dict(score=score, end=end, start=start, ops=ops, rows=rows)


def extend_multi(pairs, bands, match, mismatch, go, ge, xdrops, group=64):
    """[(p, t)], [(lo, hi)] (valid bands), several drops over one fill -> {xdrop: [dict(score, end, start, ops, rows)]}"""
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
        tab = fill([pairs[k] for k in kk], [bands[k] for k in kk], match, mismatch, go, ge)
        for g, k in enumerate(kk):
            for xd in xdrops:
                out[xd][k] = result(tab, g, len(pairs[k][0]), len(pairs[k][1]), xd)
    return out


def extend_many(pairs, bands, match, mismatch, go, ge, xdrop, group=64):
    return extend_multi(pairs, bands, match, mismatch, go, ge, [xdrop], group)[xdrop]


def extend(p, t, band, match, mismatch, go, ge, xdrop):
    return extend_many([(p, t)], [band], match, mismatch, go, ge, xdrop)[0]


def scalar_dp(p, t, band, match, mismatch, go, ge, xdrop, matrix=False):
    """Plain three-matrix DP of the same contract, float -inf, cell by cell, rows in order with the stop test after each (small
    pairs) -> dict(score, end, start, ops, rows); matrix=True: also H of every row (no stop applied), under "H" """
    n, m = len(p), len(t)
    if n == 0 or m == 0:
        return dict(score=0, end=(0, 0), start=(0, 0), ops=b"", rows=0)
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
    best, end, rows, stopped = 0, (0, 0), 0, False
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
            d = H[i - 1][j - 1] + (match if p[i - 1] == t[j - 1] else mismatch)
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
        if rmax > best:
            best, end = rmax, (i, rj)
    if xdrop >= 0 and not stopped:
        rows = n
    tab = dict(src=np.array(src), eop=np.array(eop), fop=np.array(fop))
    ops, start = go_.walk(tab, "nw", end[0], end[1])
    out = dict(score=int(best), end=end, start=start, ops=ops, rows=rows)
    if matrix:
        out["H"] = H
    return out
