"""The codes form of the wavefront alignments (pwa_align_wfa_codes_batch; include/pwalign.h, "The codes form") restated in plain Python
on the wavefronts of wfa_oracle.py: the code plane, pass A over the codes alone, pass B over the records and the sequences.  It keeps
the device's layout -- wavefront s at byte cum(s) of the plane, a skipped wavefront left as junk, the records at the front of an op
region of n + m bytes that pass B fills from the end downwards -- so that the claims the kernels rest on are checked here: the codes
and a greedy extend are enough to rebuild wfa_oracle.backtrace's op list, and no write lands on an unread record."""
import numpy as np

import wfa_oracle as WO

SRC_X, SRC_I, SRC_D, SRC_NONE = 0, 1, 2, 3
OPEN_I, OPEN_D = 4, 8
TO_M = 0x80
JUNK = 0xA7   # what a skipped wavefront's bytes hold: bits that would send a walk astray if it ever read them


def cum(s, n, m, o, e):
    """cells of the wavefronts 0 .. s - 1"""
    return WO.cells_to(s - 1, n, m, o, e) if s else 0


def code_plane(W, pen, P, n, m):
    """one byte per cell of the wavefronts 0 .. P, from the values the offset walk compares"""
    x, o, e = pen
    plane = np.full(WO.cells_to(P, n, m, o, e), JUNK, dtype=np.uint8)
    K = np.arange(-n - 1, m + 2, dtype=np.int64)
    none = np.full(len(K), WO.NEG, dtype=np.int64)
    pad = none[:1]

    def left(a):    # a[k - 1] at k
        return np.concatenate([pad, a[:-1]])

    def right(a):   # a[k + 1] at k
        return np.concatenate([a[1:], pad])

    for s in sorted(W):
        wx, wo, we = W.get(s - x), W.get(s - o - e), W.get(s - e)
        vx = none if wx is None else wx[0] + 1
        vx = np.where((vx >= 0) & (vx <= m) & (vx - K >= 0) & (vx - K <= n), vx, WO.NEG)
        vi, vd = W[s][1], W[s][2]
        v = np.maximum(np.maximum(vx, vi), vd)
        src = np.where(v < 0, SRC_NONE, np.where(vx == v, SRC_X, np.where(vi == v, SRC_I, SRC_D)))   # ties: mismatch, then I, then D
        if s == 0:
            src[:] = SRC_NONE
        mo = none if wo is None else wo[0]
        code = src | np.where(left(mo) >= left(none if we is None else we[1]), OPEN_I, 0) | np.where(right(mo) >= right(none if we is None else we[2]), OPEN_D, 0)
        lo, hi = WO.span(s, n, m, o, e)
        at = cum(s, n, m, o, e)
        plane[at:at + hi - lo + 1] = code[lo + n + 1:hi + n + 2]
    return plane


class Fault(Exception):
    pass


def pass_a(plane, pen, P, n, m, region):
    """the records into region[0 .. E) -> (E, op count)"""
    x, o, e = pen
    cap = n + m
    s, k, st, E, ui, uj = P, m - n, 0, 0, 0, 0
    for _ in range(2 * cap + 3):
        if st == 0 and s == 0:
            if k != 0:
                raise Fault("score 0 off the main diagonal")
            break
        if s < 0 or E >= cap:
            raise Fault("left the sweep")
        lo, hi = WO.span(s, n, m, o, e)
        if not lo <= k <= hi:
            raise Fault("left the span")
        code = plane[cum(s, n, m, o, e) + k - lo]
        if st == 0:
            src = code & 3
            if src == SRC_NONE:
                raise Fault("a NULL cell")
            if src == SRC_X:
                region[E] = ord("M") | TO_M
                E, ui, uj, s = E + 1, ui + 1, uj + 1, s - x
            else:
                st = src
        else:
            ins = st == 1
            opened = bool(code & (OPEN_I if ins else OPEN_D))
            region[E] = ord("I" if ins else "D") | (TO_M if opened else 0)
            E += 1
            if ins:
                uj, k = uj + 1, k - 1
            else:
                ui, k = ui + 1, k + 1
            s -= o + e if opened else e
            if opened:
                st = 0
    else:
        raise Fault("no end")
    if ui > n or uj > m or n - ui != m - uj:
        raise Fault("the edits do not fit the pair")
    return E, E + n - ui


def pass_b(p, t, region, E, cnt):
    """the op list into region[0 .. cnt), over the records, in traceback order"""
    n, m = len(p), len(t)
    i = j = 0
    wr = cnt
    unread = E   # records region[0 .. unread) not read yet

    def extend(room):
        nonlocal i, j, wr
        run = 0
        while i + run < n and j + run < m and p[i + run] == t[j + run]:
            run += 1
        if run > room:
            raise Fault("more matches than op slots")
        assert wr - run >= unread   # no write on an unread record
        region[wr - run:wr] = b"M" * run
        wr, i, j = wr - run, i + run, j + run

    for r in range(E - 1, -1, -1):
        rec = region[r]
        unread = r
        if rec & TO_M:
            extend(wr - (r + 1))
        op = rec & 0x7F
        i += op != ord("I")
        j += op != ord("D")
        assert wr - 1 >= unread
        region[wr - 1] = op
        wr -= 1
    extend(wr)
    if wr or (i, j) != (n, m):
        raise Fault("the replay does not end on (n, m)")


def backtrace(p, t, W, pen, P):
    """wfa_oracle.backtrace's op list, from the codes and the sequences alone"""
    n, m = len(p), len(t)
    plane = code_plane(W, pen, P, n, m)
    region = bytearray([JUNK]) * (n + m)
    E, cnt = pass_a(plane, pen, P, n, m, region)
    pass_b(p, t, region, E, cnt)
    return bytes(region[:cnt])


def align(p, t, match, mismatch, go, ge, min_score=None):
    """wfa_oracle.align with the op list of the codes form -> (result of the codes form, result of the offset walk)"""
    x, o, e, g = WO.penalties(match, mismatch, go, ge)
    want = WO.align(p, t, match, mismatch, go, ge, min_score)
    if want["score"] is None:
        return dict(want), want
    P, W = WO.sweep(p, t, (x, o, e), want["penalty"])
    assert P == want["penalty"]
    return dict(want, ops=backtrace(bytes(p), bytes(t), W, (x, o, e), P)), want
