"""The row order of the packed profile form's integer row (batch_scores.hip.h, PROF16 with INT = true), restated in numpy and checked
against the oracle without a GPU: the last column's subtract of a row deferred into the next row's step and written into col[] in
place, the pad rows past the pattern's end skipped in pairs behind the pair's first adds and the deferred subtract, the pending
subtract of the last row that ran done by the first skipped pair (or at the block's end), and `best` kept on m = H + gamma."""
import random

import numpy as np

import oracle_lib as O

R, C = 152, 8
CODE = {65: 0, 67: 1, 71: 2, 84: 3}   # A C G T


def rows_run(n):
    """what pwalign.hip prices (prof16_rows): n rounded up to a pair of rows, the first pair always"""
    return 2 if n <= 2 else (n + 1) // 2 * 2


def profile_row_scores(pattern, texts, match, mismatch, gap):
    """One wave task: `pattern` against every text (a lane each), in the kernel's order.  Returns (scores, rows whose chain ran)."""
    gamma = -gap
    assert mismatch - gap >= 0 and match - gap >= 0 and len(pattern) <= R
    n, L = len(pattern), len(texts)
    m = max(len(t) for t in texts)
    codes = [CODE[c] for c in pattern] + [4] * (R - n)          # 4 = the pad code: offset 32, the zero profile
    tx = np.full((L, (m + C - 1) // C * C), 12, dtype=np.int64)  # 12 = the text pad code: s' = 0
    for l, t in enumerate(texts):
        tx[l, :len(t)] = [CODE[c] for c in t]
    sub = lambda a: np.maximum(a - gamma, 0)                    # v_pk_sub_u16 clamp
    col = [np.zeros(L, dtype=np.int64) for _ in range(R)]
    best = np.zeros(L, dtype=np.int64)
    ran = 0
    for jb in range(tx.shape[1] // C):
        blk = tx[:, C * jb:C * jb + C]
        prof = lambda sigma, k: np.zeros(L, dtype=np.int64) if sigma == 4 else np.where(blk[:, k] == 12, 0, np.where(blk[:, k] == sigma, match, mismatch) + gamma)
        u = [np.zeros(L, dtype=np.int64) for _ in range(C - 1)]
        pend = np.zeros(L, dtype=np.int64)
        ran = 0
        for r in range(0, R, 2):
            for q in (r, r + 1):
                sigma = codes[q]
                # the row's adds: the diagonal of column 0 is the OLD col[q - 1] (row 0: the boundary's 0)
                t = [(col[q - 1] if q else 0) + prof(sigma, 0)] + [u[k - 1] + prof(sigma, k) for k in range(1, C)]
                if q:
                    col[q - 1] = sub(pend)                      # the deferred subtract, in place
                if q == r and r >= 2 and sigma == 4:
                    break                                       # a pad pair: nothing else of its text runs
                left = col[q]
                for k in range(C - 1):
                    mk = np.maximum(np.maximum(t[k], u[k]), left)
                    best = np.maximum(best, mk)
                    u[k] = sub(mk)
                    left = u[k]
                pend = np.maximum(np.maximum(t[C - 1], col[q - 1] if q else 0), left)
                best = np.maximum(best, pend)
                ran += 1
        col[R - 1] = sub(pend)                                  # the block's end (a pad row's col when a pair was skipped)
    return [int(x) for x in np.maximum(best - gamma, 0)], ran


def check(pattern, texts, scoring):
    got, ran = profile_row_scores(pattern, texts, *scoring)
    assert ran == rows_run(len(pattern)), (len(pattern), ran)
    want = [O.score("sw", pattern, t, *scoring)[0] for t in texts]
    assert got == want, (len(pattern), [len(t) for t in texts], scoring, got, want)


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def test_random_small_pairs():
    rng = random.Random(2601)
    scorings = [(1, -1, -1), (5, -4, -4), (2, -3, -3), (3, 0, 0), (13, -127, -127)]
    for i in range(40):   # 40 tasks x 8 lanes = 320 pairs
        pattern = rand_seq(rng, rng.randint(1, 40) if i % 4 else rng.randint(100, R))
        texts = [rand_seq(rng, rng.randint(1, 40)) for _ in range(8)]
        if i % 3 == 0:
            texts[0] = pattern[:20] + texts[0] + pattern[-20:]   # long diagonal runs
        check(pattern, texts, scorings[i % len(scorings)])


def test_edge_lengths():
    """patterns of 1, 2, 3, 149..152 rows against texts of 1, 7, 8, 9, 15, 16, 17 and 65 columns (lanes whose text ends blocks
    before their neighbour's), gap 0 and gap -127"""
    rng = random.Random(2602)
    texts = [rand_seq(rng, m) for m in (1, 7, 8, 9, 15, 16, 17, 65)]
    for n in (1, 2, 3, 149, 150, 151, 152):
        pattern = rand_seq(rng, n)
        lanes = texts + [pattern[:33], pattern[-9:] + pattern[:9]]
        for scoring in [(1, -1, -1), (3, 0, 0), (13, -127, -127), (1, -5, -127)]:
            check(pattern, lanes, scoring)


def test_the_bound_with_a_pad_row_after_the_maximum():
    """match 23, 89 rows (odd: row 89 runs as a pad row after the maximum): exactly 2047"""
    rng = random.Random(614)
    base = rand_seq(rng, 150)
    got, ran = profile_row_scores(base[:89], [base, base[:88]], 23, -1, -1)
    assert ran == 90 and got[0] == 2047 and got[1] == 88 * 23
