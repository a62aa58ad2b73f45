"""Affine-gap alignment under a substitution matrix (pwa_align_subst_batch, include/pwalign.h) restated in numpy: gotoh_oracle's fill
with s(i, j) = M[code[p[i-1]], code[t[j-1]]] in place of match / mismatch.  Everything after the fill -- the three-state walk, end
cells, pairs with an empty side -- is gotoh_oracle's own, imported.  `code` is a 256-entry map from byte value to symbol code, M an
(n_sym, n_sym) integer matrix, row = pattern code, column = text code; it may be asymmetric and hold any signs."""
import numpy as np

import gotoh_oracle as GO
from gotoh_oracle import NEG, SRC_D, SRC_E, SRC_F, SRC_Z, _arr, _one, result, walk   # noqa: F401 (walk, result: re-exported)


def _table(table):
    code, n_sym, submat = table
    return np.asarray(code, dtype=np.int64), np.asarray(submat, dtype=np.int64).reshape(n_sym, n_sym)


def fill(P, T, mode, table, go, ge):
    """gotoh_oracle.fill with the matrix: P (B, n) uint8, T (B, m) uint8 (RAW bytes) -> dict(H, src, eop, fop)"""
    code, M = _table(table)
    P, T = np.atleast_2d(P), np.atleast_2d(T)
    cP, cT = code[P], code[T]
    nb, n = P.shape
    m = T.shape[1]
    oe = go + ge
    jj = np.arange(m + 1, dtype=np.int64)
    H = np.zeros((nb, n + 1, m + 1), dtype=np.int64)
    src = np.zeros((nb, n + 1, m + 1), dtype=np.uint8)
    eop = np.zeros((nb, n + 1, m + 1), dtype=bool)
    fop = np.zeros((nb, n + 1, m + 1), dtype=bool)
    if mode == "nw":
        H[:, 0, 1:] = go + jj[1:] * ge
    if mode in ("nw", "sg"):
        H[:, 1:, 0] = go + np.arange(1, n + 1, dtype=np.int64) * ge
    Fp = np.full((nb, m + 1), NEG, dtype=np.int64)   # F of row 0: -inf
    for i in range(1, n + 1):
        hp = H[:, i - 1, :]
        s = M[cP[:, i - 1:i], cT]
        diag = hp[:, :-1] + s
        fo, fe = hp + oe, Fp + ge
        F = np.maximum(fo, fe)
        fopen = fo >= fe
        A = np.empty((nb, m + 1), dtype=np.int64)
        A[:, 0] = H[:, i, 0]
        A[:, 1:] = np.maximum(diag, F[:, 1:])
        if mode == "sw":
            A[:, 1:] = np.maximum(A[:, 1:], 0)
        E = np.full((nb, m + 1), NEG, dtype=np.int64)
        if m:
            cm = np.maximum.accumulate(A - jj * ge, axis=1)[:, :-1]   # max_{k < j}, j = 1..m
            E[:, 1:] = (jj[1:] - 1) * ge + oe + cm
        h = np.maximum(A, E)
        h[:, 0] = H[:, i, 0]
        H[:, i, :] = h
        eopen = np.zeros((nb, m + 1), dtype=bool)
        if m:
            eopen[:, 1:] = h[:, :-1] + oe >= np.concatenate([np.full((nb, 1), NEG), E[:, 1:-1]], axis=1) + ge
        d, e, f = diag, E[:, 1:], F[:, 1:]
        hv = h[:, 1:]
        if mode == "sw":
            c = np.where(hv == 0, SRC_Z, np.where(d == hv, SRC_D, np.where(f == hv, SRC_F, SRC_E)))
        else:
            c = np.where(d == hv, SRC_D, np.where(e == hv, SRC_E, SRC_F))
        src[:, i, 1:] = c
        eop[:, i, :] = eopen
        fop[:, i, :] = fopen
        Fp = F
    return dict(H=H, src=src, eop=eop, fop=fop)


def align(p, t, mode, table, go, ge, want_ops=True):
    p, t = _arr(p), _arr(t)
    tab = fill(p[None, :], t[None, :], mode, table, go, ge)
    return result(_one(tab, 0), mode, len(p), len(t), go, ge, want_ops)


def prefixes(p, t, ms, mode, table, go, ge, want_ops=True):
    """(p, t[:m]) for every m in ms, from one fill of (p, t)"""
    p, t = _arr(p), _arr(t)
    tab = _one(fill(p[None, :], t[None, :], mode, table, go, ge), 0)
    return [result(tab, mode, len(p), m, go, ge, want_ops) for m in ms]


def align_many(pairs, mode, table, go, ge, want_ops=True, group=32):
    """[(p, t)] -> [dict]; pairs of the same shape are filled together, `group` at a time"""
    out = [None] * len(pairs)
    by_shape = {}
    for k, (p, t) in enumerate(pairs):
        by_shape.setdefault((len(p), len(t)), []).append(k)
    for (n, m), ks in by_shape.items():
        for g in range(0, len(ks), group):
            kk = ks[g:g + group]
            P = np.stack([_arr(pairs[k][0]) for k in kk]) if n else np.zeros((len(kk), 0), np.uint8)
            T = np.stack([_arr(pairs[k][1]) for k in kk]) if m else np.zeros((len(kk), 0), np.uint8)
            tab = fill(P, T, mode, table, go, ge)
            for x, k in enumerate(kk):
                out[k] = result(_one(tab, x), mode, n, m, go, ge, want_ops)
    return out


def op_score(p, t, ops, start, table, go, ge):
    """The score of an op list (traceback order) from its start cell under the matrix: every maximal run of 'I' or of 'D' is one gap."""
    code, M = _table(table)
    i, j = start
    s, run, prev = 0, 0, None
    for o in reversed(bytes(ops)):
        if o != prev and run:
            s += go + run * ge
            run = 0
        if o == 77:
            s += int(M[code[p[i]], code[t[j]]])
            i += 1
            j += 1
        else:
            run += 1
            if o == 68:
                i += 1
            else:
                j += 1
        prev = o
    if run:
        s += go + run * ge
    return s


def scalar_dp(p, t, mode, table, go, ge):
    """Plain three-matrix DP with -inf, cell by cell (small pairs): -> (H, src, eop, fop) as lists of lists"""
    code, M = _table(table)
    n, m = len(p), len(t)
    oe = go + ge
    inf = float("-inf")
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[inf] * (m + 1) for _ in range(n + 1)]
    F = [[inf] * (m + 1) for _ in range(n + 1)]
    src = [[0] * (m + 1) for _ in range(n + 1)]
    eop = [[False] * (m + 1) for _ in range(n + 1)]
    fop = [[False] * (m + 1) for _ in range(n + 1)]
    for j in range(1, m + 1):
        H[0][j] = go + j * ge if mode == "nw" else 0
    for i in range(1, n + 1):
        H[i][0] = 0 if mode == "sw" else go + i * ge
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            eo, ee = H[i][j - 1] + oe, E[i][j - 1] + ge
            E[i][j], eop[i][j] = (eo, True) if eo >= ee else (ee, False)
            fo, fe = H[i - 1][j] + oe, F[i - 1][j] + ge
            F[i][j], fop[i][j] = (fo, True) if fo >= fe else (fe, False)
            d = H[i - 1][j - 1] + int(M[code[p[i - 1]], code[t[j - 1]]])
            if mode == "sw":
                h = max(0, d, E[i][j], F[i][j])
                src[i][j] = SRC_Z if h == 0 else SRC_D if d == h else SRC_F if F[i][j] == h else SRC_E
            else:
                h = max(d, E[i][j], F[i][j])
                src[i][j] = SRC_D if d == h else SRC_E if E[i][j] == h else SRC_F
            H[i][j] = h
    return H, src, eop, fop
