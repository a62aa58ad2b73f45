"""Semi-global alignment (PWA_MODE_SG, include/pwalign.h) restated in numpy: the test-side oracle of the mode.

The pinned C oracle (oracle/) is hw2.cpp's NW and SW only; this module restates the semi-global semantics from the header:
NW's recurrence and tie-break (diag first, then left if strictly greater, then up if strictly greater), row 0 = 0, column 0 =
i * gap, end cell (n, j*) with j* the smallest j of a maximum of row n, NW's walk from there while i > 0.

Rows are computed one at a time for a whole group of same-shape pairs.  With a linear gap the left chain of a row is closed
form: H[j] = gap * j + cummax_k<=j(A[k] - gap * k), A = max(diag, up) (A[0] = the row's column-0 value), so a 10k x 10k pair
takes seconds.  DP column j depends only on columns <= j: the matrices of (p, t[:m']) are the first m' + 1 columns of those
of (p, t), which the tests use to get many text lengths out of one fill."""
import numpy as np

D, L, U, S = ord("d"), ord("l"), ord("u"), ord(" ")


def _arr(x):
    return np.frombuffer(bytes(x), dtype=np.uint8)


def fill(P, T, match, mismatch, gap, codes=True, dp=False):
    """P: (B, n) uint8 patterns, T: (B, m) uint8 texts.  Returns (last, tb, mat): last = row n (B, m + 1) int64; tb = the
    traceback codes (B, n + 1, m + 1) uint8 as pwa_align_matrices writes them (or None); mat = the whole dp (or None)."""
    P, T = np.atleast_2d(P), np.atleast_2d(T)
    nb, n = P.shape
    m = T.shape[1]
    jg = gap * np.arange(m + 1, dtype=np.int64)
    prev = np.zeros((nb, m + 1), dtype=np.int64)   # row 0: free
    tb = np.full((nb, n + 1, m + 1), S, dtype=np.uint8) if codes else None
    mat = np.zeros((nb, n + 1, m + 1), dtype=np.int64) if dp else None
    if dp:
        mat[:, :, 0] = gap * np.arange(n + 1, dtype=np.int64)
        mat[:, 0, :] = 0
    for i in range(1, n + 1):
        s = np.where(P[:, i - 1:i] == T, match, mismatch).astype(np.int64)
        diag = prev[:, :-1] + s
        up = prev[:, 1:] + gap
        a = np.empty((nb, m + 1), dtype=np.int64)
        a[:, 0] = i * gap
        a[:, 1:] = np.maximum(diag, up)
        h = jg + np.maximum.accumulate(a - jg, axis=1)
        if codes:
            left = h[:, :-1] + gap
            c = np.where(left > diag, L, D).astype(np.uint8)
            c = np.where(up > np.maximum(diag, left), U, c)
            tb[:, i, 1:] = c
            tb[:, i, 0] = U
        if dp:
            mat[:, i, :] = h
        prev = h
    return prev, tb, mat


def walk(tb, n, j):
    """NW's walk (hw2.cpp:163-181) from (n, j) on one pair's codes, stopping at row 0 -> (ops in traceback order, start)."""
    i, ops = n, bytearray()
    while i > 0 and j > 0:
        c = tb[i, j]
        if c == D:
            ops.append(77)
            i -= 1
            j -= 1
        elif c == U:
            ops.append(68)
            i -= 1
        else:
            ops.append(73)
            j -= 1
    ops += b"D" * i   # column 0 is all 'u'
    return bytes(ops), (0, j)


def result(last, tb, n, m, gap, want_ops=True):
    """score, end, start, ops of (p, t[:m]) from a fill of (p, t) with len(t) >= m"""
    if n == 0:
        return dict(score=0, end=(0, 0), start=(0, 0), ops=b"")
    row = last[: m + 1]
    js = int(np.argmax(row))   # the first maximum: the smallest j
    out = dict(score=int(row[js]), end=(n, js))
    if want_ops:
        out["ops"], out["start"] = walk(tb, n, js)
    return out


def align(p, t, match, mismatch, gap, want_ops=True, mats=False):
    """One pair -> dict(score, end, start, ops[, dp, tb])"""
    p, t = _arr(p), _arr(t)
    n, m = len(p), len(t)
    last, tb, mat = fill(p[None, :], t[None, :], match, mismatch, gap, codes=want_ops or mats, dp=mats)
    out = result(last[0], tb[0] if tb is not None else None, n, m, gap, want_ops)
    if mats:
        out["dp"], out["tb"] = mat[0].astype(np.int32), tb[0]
    return out


def prefixes(p, t, ms, match, mismatch, gap, want_ops=True):
    """(p, t[:m]) for every m in ms, from one fill of (p, t)"""
    p, t = _arr(p), _arr(t)
    last, tb, _ = fill(p[None, :], t[None, :], match, mismatch, gap, codes=want_ops)
    return [result(last[0], tb[0] if want_ops else None, len(p), m, gap, want_ops) for m in ms]


def align_many(pairs, match, mismatch, gap, want_ops=True, group=64):
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
            last, tb, _ = fill(P, T, match, mismatch, gap, codes=want_ops)
            for x, k in enumerate(kk):
                out[k] = result(last[x], tb[x] if want_ops else None, n, m, gap, want_ops)
    return out


def op_score(p, t, ops, start, match, mismatch, gap):
    """the sum of the walk's op scores (match / mismatch per 'M', gap per 'D' / 'I')"""
    i, j = start
    s = 0
    for o in reversed(ops):
        if o == 77:
            s += match if p[i] == t[j] else mismatch
            i += 1
            j += 1
        elif o == 68:
            s += gap
            i += 1
        else:
            s += gap
            j += 1
    return s
