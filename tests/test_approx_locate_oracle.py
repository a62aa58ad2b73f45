"""The oracle of the start positions and minima (approx_locate_oracle.py) against the definitions, the anchored column step of
approx_start_kernel (approx.hip.h) restated on Python integers, the bounds of a start, and minima taken from the hit list alone
against minima of the full row.  No GPU."""
import numpy as np

import approx_locate_oracle as LO
import approx_oracle as AO


def small_cases(seed, count, max_m, max_n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        alphabet = b"ACGT"[:int(rng.integers(1, 5))]
        m, n = int(rng.integers(1, max_m + 1)), int(rng.integers(0, max_n + 1))
        p = AO.random_seq(rng, m, alphabet)
        t = AO.random_seq(rng, n, alphabet)
        if n > m and rng.integers(2):   # a mutated copy in the text, so that small distances occur
            copy = AO.mutate(rng, p, int(rng.integers(0, 3)), alphabet)[:n]
            at = int(rng.integers(0, n - len(copy) + 1))
            t = t[:at] + copy + t[at + len(copy):]
        out.append((p, t))
    return out


def plain_anchored(p, t):
    """D'[m][0 .. n] by the triple loop, D'[0][j] = j"""
    m, n = len(p), len(t)
    d = [list(range(n + 1))] + [[i] + [0] * n for i in range(1, m + 1)]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            d[i][j] = min(d[i - 1][j - 1] + (p[i - 1] != t[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1)
    return d[m]


def test_anchored_row_equals_the_triple_loop():
    for p, t in small_cases(1, 200, 9, 20):
        assert LO.anchored_row(p, t).tolist() == plain_anchored(p, t), (p, t)


def anchored_column(p, t, words):
    """D'[m][0 .. n] by the start kernel's step: a column of 64 * words bits with the pattern at its top, pad rows below it that
    match NO symbol and hold Pv = Mv = 0, one add over the whole column, shifts by one with a 1 coming into Ph at bit 0."""
    m, bits = len(p), 64 * words
    pad, full = bits - m, (1 << bits) - 1
    peq = {c: sum(1 << (pad + i) for i in range(m) if p[i] == c) for c in set(t) | set(p)}   # pad bits clear
    pv, mv, score, out = full & ~((1 << pad) - 1), 0, m, [m]
    for c in t:
        eq = peq[c]
        xh = ((((eq & pv) + pv) & full) ^ pv) | eq
        ph = mv | (full & ~(xh | pv))
        mh = pv & xh
        score += (ph >> (bits - 1)) - (mh >> (bits - 1))
        xv = eq | mv
        ph1, mh1 = ((ph << 1) | 1) & full, (mh << 1) & full
        pv = mh1 | (full & ~(xv | ph1))
        mv = ph1 & xv
        if pad:   # the pad rows stay as they began
            assert pv & ((1 << pad) - 1) == 0 and mv & ((1 << pad) - 1) == 0
        out.append(score)
    return out


def test_anchored_column_step_on_integers():
    cases = small_cases(2, 2500, 70, 90)
    rng = np.random.default_rng(3)
    for m in (31, 32, 33, 63, 64, 65, 127, 128, 129, 200):
        p = AO.random_seq(rng, m, b"ACGT")
        cases.append((p, AO.mutate(rng, p, m // 10, b"ACGT") + AO.random_seq(rng, 40, b"ACGTN")))
        cases.append((b"A" * m, b"A" * (m // 2) + b"C" + b"A" * m))
    assert len(cases) > 2500
    for p, t in cases:
        want = LO.anchored_row(p, t).tolist()
        words = (len(p) + 63) // 64
        for w in (words, words + 1):
            assert anchored_column(p, t, w) == want, (len(p), w)


def test_start_bounds_and_the_definition_at_every_end():
    """For every end e of 300 small cases: the reversed anchored row's minimum is D[m][e], its first index j lies in
    [max(0, m - d), min(e, m + d)], and start_of (which looks at the last m + d symbols only) names e - j."""
    ends = 0
    for p, t in small_cases(4, 300, 12, 120):
        m = len(p)
        row = AO.last_row(p, t)
        for e in range(1, len(t) + 1):
            d = int(row[e])
            back = LO.anchored_row(p[::-1], t[:e][::-1])
            assert int(back.min()) == d, (p, t, e)
            j = int(np.nonzero(back == d)[0][0])
            assert max(0, m - d) <= j <= min(e, m + d), (p, t, e, j)
            assert not (back[:j] <= d).any()
            assert LO.start_of(p, t, e, d) == e - j
            if d:
                assert LO.start_of(p, t, e, d - 1) is None   # an understated distance has no start
            ends += 1
    assert ends > 10000


def test_minima_from_the_hit_list_equal_minima_of_the_row():
    kept = total = 0
    cases = small_cases(5, 400, 24, 160)
    cases += [(b"AB", b"A" * 50), (b"AAAA", b"A" * 40), (b"ACGT", b"")]   # a plateau without an end, all zeros, an empty text
    for p, t in cases:
        m, n = len(p), len(t)
        row = AO.last_row(p, t)
        for k in (0, 1, m // 4, m - 1, m, m + 3):
            hits = AO.hits(p, t, k)
            got = LO.minima_from_hits(hits, m, k, n)
            assert got == LO.minima_from_row(row, k), (p, t, k)
            total += len(hits)
            kept += len(got)
    assert total > 50000 and 0 < kept < total


def test_minima_definition_on_hand_made_rows():
    # m = 3: a plateau from column 0 (value m) is not kept; a descent into a plateau that ends with the text is
    assert LO.minima_from_row([3, 3, 3, 2, 2, 3, 1, 1], 3) == [(3, 2), (6, 1)]
    assert LO.minima_from_row([3, 3, 3, 3], 3) == []
    assert LO.minima_from_row([3, 2, 1, 0, 1, 0, 0, 1, 2, 1], 1) == [(3, 0), (5, 0), (9, 1)]
    assert LO.minima_from_row([3, 2, 1, 1, 0], 5) == [(4, 0)]   # a plateau left by a descent is not kept
