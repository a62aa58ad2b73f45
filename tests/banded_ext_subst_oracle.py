"""Banded X-drop extension under a substitution matrix with the pattern-end result (pwa_extend_banded_subst_batch, include/pwalign.h)
restated in numpy: the test-side oracle of the feature.

The matrix is banded_subst_oracle.fill's NW matrix -- the same recurrences in band coordinates, s(i, j) = M[code[p[i-1]],
code[t[j-1]]]; its traceback tables ARE that function's (`fill` below asserts it), so the walk is banded_oracle's -- and what is read
from it is banded_ext_oracle's: per row the maximum over the in-band cells with j >= 1 and its first column (computed here, because
banded_subst_oracle.fill keeps H of row n only), that module's `record` (best cell, stop rule, rows) and its NW walk.  New is the
pattern-end result: (rmax(n), its first column) when rows == n >= 1, (0, 0) for an empty pattern, None otherwise.  scalar_dp is the
same contract once more as a plain three-matrix DP, cell by cell.  `table` is (code[256], n_sym, submat) as subst_table returns it."""
import numpy as np

import banded_ext_oracle as XO
import banded_oracle as BO
import banded_subst_oracle as BSO
import gotoh_oracle as go_
from subst_oracle import _table

NEG = BO.NEG
_LOW = NEG // 2
NO_PEND = None
band_valid = XO.band_valid


def fill(pairs, bands, table, go, ge):
    """banded_subst_oracle.fill's NW tables (src, eop, fop, lo, W) and, per pair and row i, rmax / rcol as banded_ext_oracle.fill
    defines them.  The rows' H are recomputed here with the same recurrence; the traceback tables must come out the same."""
    code, M = _table(table)
    tab = BSO.fill(pairs, bands, "nw", table, go, ge)
    G = len(pairs)
    ns = np.array([len(p) for p, _ in pairs], dtype=np.int64)
    ms = np.array([len(t) for _, t in pairs], dtype=np.int64)
    lo, W = tab["lo"], tab["W"]
    hi = lo + W - 1
    B = int(W.max())
    nmax, mmax = int(ns.max()), int(ms.max())
    P = np.zeros((G, max(nmax, 1)), dtype=np.int16)
    T = np.zeros((G, max(mmax, 1)), dtype=np.int16)
    for g, (p, t) in enumerate(pairs):
        P[g, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        T[g, :len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
    oe = go + ge
    top = M.shape[0] - 1
    xs = np.arange(B, dtype=np.int64)[None, :]
    rmax = np.full((G, nmax + 1), NEG, dtype=np.int64)
    rcol = np.zeros((G, nmax + 1), dtype=np.int64)
    src = np.zeros((G, nmax + 1, B), dtype=np.uint8)
    rows = np.arange(G)
    neg1 = np.full((G, 1), NEG, dtype=np.int64)
    Hp = Fp = None
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
            s = M[np.minimum(code[P[:, i - 1:i]], top), np.minimum(code[tsym], top)]
            diag = Hp + s
            F = np.maximum(up_h + oe, up_f + ge)
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
            src[:, i, :] = np.where(diag == H, BO.SRC_D, np.where(E == H, BO.SRC_E, BO.SRC_F))
            Hc = np.where(inb & (j >= 1) & (H > _LOW), H, NEG)
            rmax[:, i] = Hc.max(axis=1)
            rcol[:, i] = i + lo + np.argmax(Hc == rmax[:, i:i + 1], axis=1)
        Hp, Fp = H, F
    assert (src == tab["src"]).all()   # the same matrix as banded_subst_oracle's
    return dict(src=tab["src"], eop=tab["eop"], fop=tab["fop"], lo=lo, W=W, rmax=rmax, rcol=rcol)


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
        return dict(XO.result(None, 0, n, m, xdrop), pend=pattern_end(None, None, n, m, 0))
    r = XO.result(tab, g, n, m, xdrop)
    r["pend"] = pattern_end(tab["rmax"][g], tab["rcol"][g], n, m, r["rows"])
    return r


def extend_multi(pairs, bands, table, go, ge, xdrops, group=64):
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
        tab = fill([pairs[k] for k in kk], [bands[k] for k in kk], table, go, ge)
        for g, k in enumerate(kk):
            for xd in xdrops:
                out[xd][k] = result(tab, g, len(pairs[k][0]), len(pairs[k][1]), xd)
    return out


def extend_many(pairs, bands, table, go, ge, xdrop, group=64):
    return extend_multi(pairs, bands, table, go, ge, [xdrop], group)[xdrop]


def extend(p, t, band, table, go, ge, xdrop):
    return extend_many([(p, t)], [band], table, go, ge, xdrop)[0]


def scalar_dp(p, t, band, table, go, ge, xdrop, matrix=False):
    """Plain three-matrix DP of the same contract, float -inf, cell by cell, rows in order with the stop test after each (small
    pairs) -> dict(score, end, start, ops, rows, pend); matrix=True: also H of every row (no stop applied), under "H" """
    code, M = _table(table)
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
            d = H[i - 1][j - 1] + int(M[code[p[i - 1]], code[t[j - 1]]])
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
