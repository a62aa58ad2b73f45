"""k-edit approximate search (include/pwalign.h, pwa_approx_*) restated in numpy: the test-side oracle.

Sellers' DP: D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (p[i-1] != t[j-1]), D[i-1][j] + 1, D[i][j-1] + 1), bytes compared
as bytes.  One row at a time over the whole text: with x[j] = min(diag, up) (x[0] = i), the in-row term D[i][j-1] + 1 unrolls to
D[i][j] = min_k<=j (x[k] + j - k) = np.minimum.accumulate(x - idx) + idx."""
import numpy as np


def _arr(x):
    return np.frombuffer(bytes(x), dtype=np.uint8)


def last_row(p, t, start=None):
    """D[m][0 .. n] of pattern p against text t (int64).  start: the column the DP starts from with D[i][start] = i, columns
    before it absent (the fresh start of a task); the result then covers columns start .. n."""
    p, t = _arr(p), _arr(t)
    if start:
        t = t[start:]
    n = len(t)
    idx = np.arange(n + 1, dtype=np.int64)
    prev = np.zeros(n + 1, dtype=np.int64)
    for i in range(1, len(p) + 1):
        x = np.empty(n + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(prev[:-1] + (t != p[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(x - idx) + idx
    return prev


def hits(p, t, k):
    """[(end, dist)] in ascending end: every e in 1 .. n with D[m][e] <= k"""
    row = last_row(p, t)
    e = np.nonzero(row[1:] <= k)[0] + 1
    return [(int(x), int(row[x])) for x in e]


def best(hit_list):
    """(dist, end) of the smallest distance and, at that distance, the smallest end; None without a hit"""
    return min(((d, e) for e, d in hit_list), default=None)


def plain(p, t):
    """the whole matrix by the triple loop of the definition (tiny cases only)"""
    m, n = len(p), len(t)
    d = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        d[i][0] = i
        for j in range(1, n + 1):
            d[i][j] = min(d[i - 1][j - 1] + (p[i - 1] != t[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1)
    return d


def plan(n, pat_len, max_dist, chunk):
    """The task list of pwa_approx_plan, restated: per pattern the report ranges tile [0, n) in steps of chunk; the scan starts
    at max(0, lo - w) rounded down to a multiple of 16, w = m + min(k, m)."""
    out = []
    for q, (m, k) in enumerate(zip(pat_len, max_dist)):
        w = m + min(k, m)
        for lo in range(0, n, chunk):
            out.append((q, max(0, lo - w) // 16 * 16, lo, min(lo + chunk, n)))
    return out


def mutate(rng, s, n_edits, alphabet):
    """s with n_edits random substitutions, insertions and deletions"""
    s = bytearray(s)
    for _ in range(n_edits):
        kind = rng.integers(3)
        if kind == 0 and s:
            s[rng.integers(len(s))] = alphabet[rng.integers(len(alphabet))]
        elif kind == 1:
            s.insert(rng.integers(len(s) + 1), alphabet[rng.integers(len(alphabet))])
        elif s:
            del s[rng.integers(len(s))]
    return bytes(s)


def random_seq(rng, n, alphabet):
    return bytes(np.frombuffer(bytes(alphabet), dtype=np.uint8)[rng.integers(len(alphabet), size=n)])
