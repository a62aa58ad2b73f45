"""Affine-gap ("gotoh") alignment (pwa_align_gotoh_batch, include/pwalign.h) restated in numpy: the test-side oracle of the feature.

A gap of length L scores gap_open + L * gap_extend; E = 'I' (left), F = 'D' (up), ties OPEN; H tie-break NW / SG: diag >= E >= F,
SW: zero > diag > F > E.  Rows are computed one at a time for a group of same-shape pairs.  F comes from the row above; the left
chain is closed form: with gap_open <= 0, reopening a gap from an E-derived H is never better than extending it, so
    E[i][j] = (j - 1) * ge + oe + max_{k < j}(A[k] - k * ge),   A[k] = max(diag, F) at column k (SW: and 0), A[0] = H[i][0]
and H = max(A, E).  The open / extend bits and the H source then follow from the values with the tie rules.  DP column j depends
only on columns <= j: the tables of (p, t[:m']) are the first m' + 1 columns of those of (p, t) (`prefixes`).

The scoring of a diagonal step is one value `sc`, here and in the banded oracles built on this module: a pair (match, mismatch)
(pwa_align_gotoh_batch) or a substitution table (code[256], n_sym, submat) as subst_table returns it (pwa_align_subst_batch): row =
pattern code, column = text code; the matrix may be asymmetric and hold any signs.  `scorer` is the only place that tells the two
apart."""
import numpy as np

MODES = {"nw": 0, "sw": 1, "sg": 2}
SRC_D, SRC_E, SRC_F, SRC_Z = 0, 1, 2, 3   # H source codes of this module
NEG = -(1 << 40)                         # -inf: far below any value, never wraps in int64


def _arr(x):
    return np.frombuffer(bytes(x), dtype=np.uint8)


def scorer(sc):
    """sc -> (row, cell): row(pattern symbols (B, 1), text symbols (B, m)) -> (B, m) int64 diagonal scores, cell(a, b) -> int.  A
    banded fill pads its texts with -1 and its patterns with 0; those slots lie outside the matrix and the fill masks them: -1
    equals no byte, and the table reads it as byte 0 and a byte without a code as the last symbol (`row` only: `cell` sees real
    bytes, and one without a code is an error there)."""
    if len(sc) == 2:
        match, mismatch = sc
        return (lambda pc, ts: np.where(pc == ts, match, mismatch).astype(np.int64)), (lambda a, b: match if a == b else mismatch)
    code, n_sym, submat = sc
    code, M = np.asarray(code, dtype=np.int64), np.asarray(submat, dtype=np.int64).reshape(n_sym, n_sym)
    sym = lambda x: np.minimum(code[np.maximum(x, 0)], n_sym - 1)
    return (lambda pc, ts: M[sym(pc), sym(ts)]), (lambda a, b: int(M[code[a], code[b]]))


def random_table(seed, alphabet, lo=-9, hi=11, unknown=None, fold_case=False):
    """an asymmetric matrix with entries in lo..hi, a positive diagonal and some positive off-diagonal entries, as a scoring value"""
    from conftest import load_pkg
    rng = np.random.RandomState(seed)
    k = len(alphabet)
    m = rng.randint(lo, hi + 1, size=(k, k))
    m[np.arange(k), np.arange(k)] = rng.randint(1, hi + 1, size=k)
    return load_pkg().subst_table(alphabet, m, unknown=unknown, fold_case=fold_case)


def fill(P, T, mode, sc, go, ge):
    """P: (B, n) uint8, T: (B, m) uint8 (raw bytes) -> dict(H, src, eop, fop): H (B, n + 1, m + 1) int64; src the H source (uint8), eop / fop
    whether E / F opened at the cell (bool); row 0 and column 0 hold the boundary values (src there is unused)."""
    row = scorer(sc)[0]
    P, T = np.atleast_2d(P), np.atleast_2d(T)
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
        diag = hp[:, :-1] + row(P[:, i - 1:i], T)
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


def walk(tab, mode, i, j):
    """The three-state walk from (i, j) in state H -> (ops in traceback order, start cell)."""
    src, eop, fop = tab["src"], tab["eop"], tab["fop"]
    ops = bytearray()
    st = 0
    while i > 0 and j > 0:
        if st == 0:
            h = src[i, j]
            if h == SRC_Z:
                break
            if h == SRC_D:
                ops.append(77)
                i -= 1
                j -= 1
                continue
            st = 1 if h == SRC_E else 2
        if st == 1:
            ops.append(73)
            st = 0 if eop[i, j] else 1
            j -= 1
        else:
            ops.append(68)
            st = 0 if fop[i, j] else 2
            i -= 1
    if mode != "sw":
        ops += b"D" * i
        i = 0
        if mode == "nw":
            ops += b"I" * j
            j = 0
    return bytes(ops), (i, j)


def gap_cost(L, go, ge):
    return go + L * ge if L else 0


def result(tab, mode, n, m, go, ge, want_ops=True):
    """score, end, start, ops of (p, t[:m]) from the tables of one pair (p, t) with len(t) >= m"""
    if n == 0 or m == 0:
        if mode == "sw" or (mode == "sg" and n == 0):
            return dict(score=0, end=(0, 0), start=(0, 0), ops=b"")
        L = n if mode == "sg" else n + m
        return dict(score=gap_cost(L, go, ge), end=(n, 0 if mode == "sg" else m), start=(0, 0), ops=b"D" * n + b"I" * (0 if mode == "sg" else m))
    H = tab["H"]
    if mode == "nw":
        end = (n, m)
    elif mode == "sg":
        end = (n, int(np.argmax(H[n, :m + 1])))
    else:
        sub = H[:n + 1, :m + 1]
        best = int(sub.max())
        if best <= 0:
            end = (0, 0)
        else:
            i = int(np.argmax(sub.max(axis=1) == best))
            end = (i, int(np.argmax(sub[i] == best)))
    out = dict(score=int(H[end[0], end[1]]), end=end)
    if want_ops:
        out["ops"], out["start"] = walk(tab, mode, end[0], end[1])
    return out


def _one(tab, x):
    return {k: v[x] for k, v in tab.items()}


def align(p, t, mode, sc, go, ge, want_ops=True):
    p, t = _arr(p), _arr(t)
    tab = fill(p[None, :], t[None, :], mode, sc, go, ge)
    return result(_one(tab, 0), mode, len(p), len(t), go, ge, want_ops)


def prefixes(p, t, ms, mode, sc, go, ge, want_ops=True):
    """(p, t[:m]) for every m in ms, from one fill of (p, t)"""
    p, t = _arr(p), _arr(t)
    tab = _one(fill(p[None, :], t[None, :], mode, sc, go, ge), 0)
    return [result(tab, mode, len(p), m, go, ge, want_ops) for m in ms]


def align_many(pairs, mode, sc, go, ge, want_ops=True, group=32):
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
            tab = fill(P, T, mode, sc, go, ge)
            for x, k in enumerate(kk):
                out[k] = result(_one(tab, x), mode, n, m, go, ge, want_ops)
    return out


def op_score(p, t, ops, start, sc, go, ge):
    """The affine score of an op list (traceback order) from its start cell: every maximal run of 'I' or of 'D' is one gap."""
    cell = scorer(sc)[1]
    i, j = start
    s, run, prev = 0, 0, None
    for o in reversed(bytes(ops)):
        if o != prev and run:
            s += go + run * ge
            run = 0
        if o == 77:
            s += cell(p[i], t[j])
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


def scalar_dp(p, t, mode, sc, go, ge):
    """Plain three-matrix DP with -inf, cell by cell (small pairs): -> (H, src, eop, fop) as lists of lists"""
    cell = scorer(sc)[1]
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
            d = H[i - 1][j - 1] + cell(p[i - 1], t[j - 1])
            if mode == "sw":
                h = max(0, d, E[i][j], F[i][j])
                src[i][j] = SRC_Z if h == 0 else SRC_D if d == h else SRC_F if F[i][j] == h else SRC_E
            else:
                h = max(d, E[i][j], F[i][j])
                src[i][j] = SRC_D if d == h else SRC_E if E[i][j] == h else SRC_F
            H[i][j] = h
    return H, src, eop, fop
