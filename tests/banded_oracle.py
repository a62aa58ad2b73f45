"""Banded affine-gap alignment (pwa_align_banded_batch, include/pwalign.h) restated in numpy: the test-side oracle of the feature.

gotoh_oracle's recurrences, tie rules and walk over the cells with lo <= j - i <= hi; everything else is -inf.  A row is computed over
its in-band columns only: the tables are kept in band coordinates, slot x of row i = cell (i, i + lo + x), so the row above sits one
slot to the right and the diagonal neighbour in the same slot.  The closed-form left chain of gotoh_oracle.fill stays valid because a
row's in-band columns are contiguous.  A group of pairs (any lengths, any bands) is filled together, padded to the longest pattern and
the widest band.  int64 with a far -inf.  The diagonal score is gotoh_oracle's scoring value `sc` (match / mismatch, or a substitution
table: pwa_align_banded_subst_batch).  Per row the fill also keeps the maximum of H over the in-band cells with j >= 1 and its first
column: what the X-drop extension (banded_ext_oracle) reads from the NW band."""
import numpy as np

import gotoh_oracle as go_

SRC_D, SRC_E, SRC_F, SRC_Z = go_.SRC_D, go_.SRC_E, go_.SRC_F, go_.SRC_Z
NEG = go_.NEG
_LOW = NEG // 2


def band_valid(mode, n, m, lo, hi):
    """the validity rule of include/pwalign.h"""
    if lo > hi:
        return False
    if mode == "nw":
        return lo <= 0 <= hi and lo <= m - n <= hi
    if mode == "sg":
        return hi >= 0 and n + lo <= m
    return True


def random_band(rng, mode, n, m):
    """a random valid band: the narrowest one the mode admits a quarter of the time (width 1 where that is valid), else wider"""
    d = m - n
    k1, k2 = [(0, 0), (rng.randint(0, 3), rng.randint(0, 3)), (rng.randint(0, n + m), rng.randint(0, n + m))][min(rng.randint(0, 3), 2)]
    if mode == "nw":
        b = (min(0, d) - k1, max(0, d) + k2)
    elif mode == "sg":
        lo = rng.randint(-n - 1, d)
        b = (lo, max(lo, 0) + (0 if k1 == 0 else k2))
    else:
        lo = rng.randint(-n - 2, m + 2)
        b = (lo, lo + (0 if k1 == 0 else k2))
    assert band_valid(mode, n, m, *b)
    return b


def fill(pairs, bands, mode, sc, go, ge):
    """pairs: [(p, t)] (raw bytes), bands: [(lo, hi)] -> dict(src, eop, fop: (G, nmax + 1, B) in band coordinates; hlast: H of each
    pair's row n; best: SW's first row-major maximum (score, i, j) per pair; lo, W: the clamped bands' lo and width; rmax, rcol: (G,
    nmax + 1), per row i >= 1 the maximum of H over the in-band cells with j >= 1 (NEG when there is none) and its first column)"""
    score = go_.scorer(sc)[0]
    G = len(pairs)
    ns = np.array([len(p) for p, _ in pairs], dtype=np.int64)
    ms = np.array([len(t) for _, t in pairs], dtype=np.int64)
    lo = np.array([b[0] for b in bands], dtype=np.int64)
    hi = np.array([b[1] for b in bands], dtype=np.int64)
    # (the band clamped to the matrix holds the same cells and keeps the tables small)
    lo = np.minimum(np.maximum(lo, -ns), ms)
    hi = np.maximum(np.minimum(hi, ms), -ns)
    W = hi - lo + 1
    B = int(W.max())
    nmax, mmax = int(ns.max()), int(ms.max())
    P = np.zeros((G, max(nmax, 1)), dtype=np.int16)
    T = np.full((G, max(mmax, 1)), -1, dtype=np.int16)   # (columns past a text are outside its matrix: masked by `inb`)
    for g, (p, t) in enumerate(pairs):
        P[g, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        T[g, :len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
    oe = go + ge
    xs = np.arange(B, dtype=np.int64)[None, :]
    src = np.zeros((G, nmax + 1, B), dtype=np.uint8)
    eop = np.zeros((G, nmax + 1, B), dtype=bool)
    fop = np.zeros((G, nmax + 1, B), dtype=bool)
    hlast = np.full((G, B), NEG, dtype=np.int64)
    best = np.zeros((G, 3), dtype=np.int64)
    rmax = np.full((G, nmax + 1), NEG, dtype=np.int64)
    rcol = np.zeros((G, nmax + 1), dtype=np.int64)
    rows = np.arange(G)
    Hp = Fp = None
    for i in range(0, nmax + 1):
        j = i + lo[:, None] + xs                                         # column of every slot
        inb = (xs < W[:, None]) & (j >= 0) & (j <= ms[:, None]) & (i <= ns[:, None])
        if i == 0:
            H = np.where(inb, (go + j * ge) * (j > 0) if mode == "nw" else 0, NEG).astype(np.int64)
            if mode == "nw":
                H = np.where(inb & (lo[:, None] <= 0), H, NEG)
            F = np.full((G, B), NEG, dtype=np.int64)
        else:
            up_h = np.concatenate([Hp[:, 1:], np.full((G, 1), NEG, dtype=np.int64)], axis=1)   # (i - 1, j)
            up_f = np.concatenate([Fp[:, 1:], np.full((G, 1), NEG, dtype=np.int64)], axis=1)
            tsym = T[rows[:, None], np.clip(j - 1, 0, max(mmax, 1) - 1)]
            diag = Hp + score(P[:, i - 1:i], tsym)                       # (i - 1, j - 1): the same slot
            fo, fe = up_h + oe, up_f + ge
            F = np.maximum(fo, fe)
            fopen = fo >= fe
            A = np.maximum(diag, F)
            if mode == "sw":
                A = np.maximum(A, 0)
            col0 = j == 0                                                # the boundary value, where its path lies in the band
            b0 = 0 if mode == "sw" else go + i * ge
            ok0 = inb & col0 if mode == "sw" else inb & col0 & (hi[:, None] >= 0)
            A = np.where(col0, np.where(ok0, b0, NEG), A)
            A = np.where(inb, A, NEG)
            A = np.where(A < _LOW, NEG, A)
            cm = np.maximum.accumulate(A - j * ge, axis=1)
            cm = np.concatenate([np.full((G, 1), NEG, dtype=np.int64), cm[:, :-1]], axis=1)    # max over the columns to the left
            E = (j - 1) * ge + oe + cm
            E = np.where(inb & ~col0 & (E > _LOW), E, NEG)
            H = np.where(col0, A, np.maximum(A, E))
            F = np.where(inb & ~col0 & (F > _LOW), F, NEG)
            hl = np.concatenate([np.full((G, 1), NEG, dtype=np.int64), H[:, :-1]], axis=1)
            el = np.concatenate([np.full((G, 1), NEG, dtype=np.int64), E[:, :-1]], axis=1)
            eop[:, i, :] = hl + oe >= el + ge
            fop[:, i, :] = fopen
            if mode == "sw":
                c = np.where(H == 0, SRC_Z, np.where(diag == H, SRC_D, np.where(F == H, SRC_F, SRC_E)))
            else:
                c = np.where(diag == H, SRC_D, np.where(E == H, SRC_E, SRC_F))
            src[:, i, :] = c
            Hc = np.where(inb & (j >= 1) & (H > _LOW), H, NEG)
            rmax[:, i] = Hc.max(axis=1)
            rcol[:, i] = i + lo + np.argmax(Hc == rmax[:, i:i + 1], axis=1)
        if mode == "sw":
            rb = H.max(axis=1)
            better = rb > best[:, 0]
            xb = np.argmax(H == rb[:, None], axis=1)
            best[better, 0] = rb[better]
            best[better, 1] = i
            best[better, 2] = (i + lo + xb)[better]
        last = ns == i
        hlast[last] = H[last]
        Hp, Fp = H, F
    return dict(src=src, eop=eop, fop=fop, hlast=hlast, best=best, lo=lo, W=W, rmax=rmax, rcol=rcol)


def walk(tab, g, mode, i, j):
    """gotoh_oracle.walk over pair g's banded tables"""
    src, eop, fop, lo = tab["src"][g], tab["eop"][g], tab["fop"][g], int(tab["lo"][g])
    ops = bytearray()
    st = 0
    while i > 0 and j > 0:
        x = j - i - lo
        if st == 0:
            h = src[i, x]
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
            st = 0 if eop[i, x] else 1
            j -= 1
        else:
            ops.append(68)
            st = 0 if fop[i, x] else 2
            i -= 1
    if mode != "sw":
        ops += b"D" * i
        i = 0
        if mode == "nw":
            ops += b"I" * j
            j = 0
    return bytes(ops), (i, j)


def result(tab, g, mode, n, m, go, ge):
    if n == 0 or m == 0:
        return go_.result(None, mode, n, m, go, ge)
    lo, W = int(tab["lo"][g]), int(tab["W"][g])
    if mode == "nw":
        end, score = (n, m), int(tab["hlast"][g, m - n - lo])
    elif mode == "sg":
        row = tab["hlast"][g, :W]
        x = int(np.argmax(row))
        end, score = (n, n + lo + x), int(row[x])
    else:
        b = tab["best"][g]
        end, score = ((int(b[1]), int(b[2])), int(b[0])) if b[0] > 0 else ((0, 0), 0)
    ops, start = walk(tab, g, mode, end[0], end[1])
    return dict(score=score, end=end, start=start, ops=ops)


def align_many(pairs, bands, mode, sc, go, ge, group=64):
    """[(p, t)], [(lo, hi)] (valid bands) -> [dict(score, end, start, ops)]; pairs of similar pattern length are filled together"""
    out = [None] * len(pairs)
    live = [k for k, (p, t) in enumerate(pairs) if len(p) and len(t)]
    for k, (p, t) in enumerate(pairs):
        if not (len(p) and len(t)):
            out[k] = go_.result(None, mode, len(p), len(t), go, ge)
    live.sort(key=lambda k: (len(pairs[k][0]), bands[k][1] - bands[k][0]))
    for a in range(0, len(live), group):
        kk = live[a:a + group]
        tab = fill([pairs[k] for k in kk], [bands[k] for k in kk], mode, sc, go, ge)
        for g, k in enumerate(kk):
            out[k] = result(tab, g, mode, len(pairs[k][0]), len(pairs[k][1]), go, ge)
    return out


def align(p, t, band, mode, sc, go, ge):
    return align_many([(p, t)], [band], mode, sc, go, ge)[0]


def ops_in_band(ops, start, band):
    """every cell of the op list's path (traceback order, from its start cell) lies in the band"""
    i, j = start
    lo, hi = band
    ok = lo <= j - i <= hi
    for o in reversed(bytes(ops)):
        if o == 77:
            i, j = i + 1, j + 1
        elif o == 68:
            i += 1
        else:
            j += 1
        ok = ok and lo <= j - i <= hi
    return ok


def walk_diagonals(ops, start):
    """(min, max) of j - i over the path of an op list"""
    i, j = start
    d = j - i
    dmin = dmax = d
    for o in reversed(bytes(ops)):
        if o == 68:
            d -= 1
        elif o == 73:
            d += 1
        dmin, dmax = min(dmin, d), max(dmax, d)
    return dmin, dmax


def scalar_dp(p, t, band, mode, sc, go, ge):
    """Plain three-matrix DP with a band mask and float -inf, cell by cell (small pairs) -> dict(score, end, start, ops)"""
    cell = go_.scorer(sc)[1]
    n, m = len(p), len(t)
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
        if mode == "nw":
            if lo <= 0 and j <= hi and inb(0, j):
                H[0][j] = go + j * ge if j else 0
        elif inb(0, j):
            H[0][j] = 0
    for i in range(1, n + 1):
        if mode == "sw":
            if inb(i, 0):
                H[i][0] = 0
        elif hi >= 0 and -i >= lo:
            H[i][0] = go + i * ge
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if not inb(i, j):
                continue
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
    if n == 0 or m == 0:
        return go_.result(None, mode, n, m, go, ge)
    bv = 0
    if mode == "nw":
        end = (n, m)
    elif mode == "sg":
        bj = max(range(m + 1), key=lambda j: (H[n][j], -j))
        end = (n, bj)
    else:
        end = (0, 0)
        for i in range(n + 1):
            for j in range(m + 1):
                if H[i][j] > bv:
                    bv, end = H[i][j], (i, j)
    tab = dict(src=np.array(src), eop=np.array(eop), fop=np.array(fop))
    ops, start = go_.walk(tab, mode, end[0], end[1])
    return dict(score=bv if mode == "sw" else int(H[end[0]][end[1]]), end=end, start=start, ops=ops)
