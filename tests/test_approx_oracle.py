"""The approximate-search oracle (approx_oracle.py) against the definition, the warm-up property the task plan rests on, and the
kernel's column step (approx.hip.h) restated on Python integers.  No GPU."""
import numpy as np

import approx_oracle as AO


def tiny_cases(seed=20240611, count=300):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        sigma = int(rng.integers(1, 5))
        alphabet = b"ACGT"[:sigma]
        m, n = int(rng.integers(1, 9)), int(rng.integers(0, 25))
        out.append((AO.random_seq(rng, m, alphabet), AO.random_seq(rng, n, alphabet)))
    return out


CASES = tiny_cases()


def test_numpy_rows_equal_the_triple_loop():
    for p, t in CASES:
        want = AO.plain(p, t)[len(p)]
        assert AO.last_row(p, t).tolist() == want, (p, t)
        for k in (0, 1, len(p) - 1, len(p), len(p) + 3):
            h = AO.hits(p, t, k)
            assert h == [(e, want[e]) for e in range(1, len(t) + 1) if want[e] <= k]
            assert AO.best(h) == (min((want[e], e) for e in range(1, len(t) + 1) if want[e] <= k) if h else None)


def test_fresh_start_w_columns_back_keeps_hits_and_makes_none():
    """A scan that starts from D[i] = i at any column s <= max(0, e - w), w = m + min(k, m), gives D[m][e] exactly where it is a hit,
    and never less than the true value anywhere."""
    checked = 0
    for p, t in CASES:
        m, n = len(p), len(t)
        full = AO.last_row(p, t)
        for s in range(0, n + 1):
            fresh = AO.last_row(p, t, start=s)
            assert (fresh >= full[s:]).all(), (p, t, s)
            for k in (0, 1, m - 1, m, m + 3):
                w = m + min(k, m)
                for e in range(s + 1, n + 1):
                    if s <= max(0, e - 1 - w):   # the task's rule with lo = e - 1: its first reported end
                        assert (fresh[e - s] <= k) == (full[e] <= k), (p, t, s, k, e)
                        if full[e] <= k:
                            assert fresh[e - s] == full[e]
                        checked += 1
    assert checked > 10000


def kernel_column(p, t, words):
    """D[m][1 .. n] by the kernel's step: a column of 64 * words bits with the pattern at its top, pad rows below it that every
    symbol matches and that start at 0, one add over the whole column, shifts by one with 0 coming in at bit 0."""
    m, bits = len(p), 64 * words
    pad, full = bits - m, (1 << bits) - 1
    peq = {}
    for c in set(t) | set(p):
        peq[c] = ((1 << pad) - 1) | sum(1 << (pad + i) for i in range(m) if p[i] == c)
    pv, mv, score, out = full & ~((1 << pad) - 1), 0, m, []
    for c in t:
        eq = peq[c]
        xh = ((((eq & pv) + pv) & full) ^ pv) | eq
        ph = mv | (full & ~(xh | pv))
        mh = pv & xh
        score += (ph >> (bits - 1)) - (mh >> (bits - 1))
        xv = eq | mv
        ph1, mh1 = (ph << 1) & full, (mh << 1) & full
        pv = mh1 | (full & ~(xv | ph1))
        mv = ph1 & xv
        out.append(score)
    return out


def test_kernel_column_step_on_integers():
    rng = np.random.default_rng(7)
    cases = list(CASES[:100])
    for m in (31, 32, 33, 63, 64, 65, 127, 128, 129, 200):
        p = AO.random_seq(rng, m, b"ACGT")
        t = AO.random_seq(rng, 150, b"ACGTN") + AO.mutate(rng, p, m // 10, b"ACGT") + AO.random_seq(rng, 40, b"ACGTN")
        cases.append((p, t))
        cases.append((b"A" * m, b"A" * 150 + b"C" + b"A" * 150))
    for p, t in cases:
        words = (len(p) + 63) // 64
        for w in (words, words + 1):
            assert kernel_column(p, t, w) == AO.last_row(p, t)[1:].tolist(), (len(p), w)


def test_plan_restatement_tiles_and_bounds():
    tasks = AO.plan(1000, [5, 70], [1, 100], 64)
    for q, m, k in ((0, 5, 1), (1, 70, 100)):
        mine = [t for t in tasks if t[0] == q]
        assert [t[2] for t in mine] == list(range(0, 1000, 64)) and mine[-1][3] == 1000
        assert all(s <= max(0, lo - (m + min(k, m))) and s % 16 == 0 for _, s, lo, _ in mine)
