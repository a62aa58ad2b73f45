"""Integer-coded row of the packed profile form (batch_scores.hip.h, PROF16 with INT = true): H stored as an integer per 16-bit half,
the diagonal add one 32-bit add for both pairs of a lane, the three-way maximum taken on the f16 reading of the halves, the gap a
packed subtract that clamps at 0.  Here without a device: the recurrence restated in numpy exactly as the kernel packs it, against
the oracle's Smith-Waterman; and the new reporter's place in the C interface.  (The host's admission rule needs a context, hence a
device: tests/test_gpu_scores_profile_int.py checks it from both sides.)"""
import os
import random
import re

import numpy as np

import oracle_lib as O
from conftest import ROOT, load_pkg


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def max3_f16x2(a, b, c):
    """v_pk_maximum3_f16 on three packed words: the maximum of the halves read as f16, returned as bits"""
    v = np.array([a, b, c], dtype=np.uint32).view(np.float16).reshape(3, 2)
    assert np.all(np.isfinite(v)) and np.all(v >= 0)
    return int(v.max(axis=0).view(np.uint32)[0])


def sub_u16x2_clamp(a, g):
    """v_pk_sub_u16 clamp: per half, max(a - g, 0)"""
    lo = max((a & 0xffff) - (g & 0xffff), 0)
    hi = max((a >> 16) - (g >> 16), 0)
    return lo | (hi << 16)


def int_form_sw2(pattern, ta, tb, match, mismatch, gap):
    """one pattern against two texts, pair A in the low halves and pair B in the high halves of every word, as a lane runs them:
    texts padded to the longer one (pad columns: s' = 0), the pattern padded by two rows (pad rows: s' = 0)"""
    gamma = -gap
    assert gamma >= 0 and mismatch + gamma >= 0 and match + gamma >= 0
    g2 = gamma | (gamma << 16)
    m = max(len(ta), len(tb))
    rows = len(pattern) + 2

    def sp(i, t, j):
        if i >= len(pattern) or j >= len(t):
            return 0
        return (match if pattern[i] == t[j] else mismatch) + gamma

    H = [0] * (m + 1)   # row -1
    best = 0
    for i in range(rows):
        new = [0] * (m + 1)   # column -1 is 0
        for j in range(m):
            s2 = sp(i, ta, j) | (sp(i, tb, j) << 16)
            t = (H[j] + s2) & 0xffffffff   # ONE 32-bit add for both halves
            assert (t & 0xffff) >= (H[j] & 0xffff)   # no carry out of the low half
            mm = max3_f16x2(t, H[j + 1], new[j])
            new[j + 1] = sub_u16x2_clamp(mm, g2)
            best = max3_f16x2(best, mm, mm)
        H = new
    return max((best & 0xffff) - gamma, 0), max((best >> 16) - gamma, 0)


SCORINGS = [(1, -1, -1), (2, -3, -5), (5, -4, -4), (3, 0, 0), (1, -127, -127), (13, -20, -127), (0, -1, -1), (-1, -2, -3)]


def test_int_form_recurrence_matches_oracle():
    rng = random.Random(610)
    for _ in range(12):
        p = rand_seq(rng, rng.randint(1, 30))
        ta = rand_seq(rng, rng.randint(0, 45))
        tb = rand_seq(rng, rng.randint(0, 45))
        for scoring in SCORINGS:
            want = tuple(O.score("sw", p, t, *scoring)[0] if t else 0 for t in (ta, tb))
            assert int_form_sw2(p, ta, tb, *scoring) == want, (p, ta, tb, scoring)


def test_int_form_at_the_admission_bound():
    """match = 127 over the longest pattern the bound admits (16 rows: 2032 <= 2047), texts that contain it: the score reaches
    16 * 127, and t reaches it plus s' = 254"""
    rng = random.Random(611)
    p = rand_seq(rng, 2047 // 127)
    ta = rand_seq(rng, 9) + p + rand_seq(rng, 5)
    tb = p[:11] + rand_seq(rng, 3) + p
    for scoring in [(127, -127, -127), (127, 0, -127), (127, -1, -1)]:
        want = tuple(O.score("sw", p, t, *scoring)[0] for t in (ta, tb))
        assert want == (127 * len(p),) * 2
        assert int_form_sw2(p, ta, tb, *scoring) == want, scoring


def test_reporter_is_exported_and_declared():
    pkg = load_pkg()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "pwalign.h")).read()
    assert "PWA_PROF16_INT" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert hasattr(L, "pwa_batch_profile_int")
    assert "pwa_batch_profile_int" in pkg.EXPORTS
    assert re.search(r"\bint\s+pwa_batch_profile_int\s*\(\s*const\s+pwa_batch\s*\*", hdr)
    assert L.pwa_batch_profile_int(None) == -1   # PWA_E_INVALID
    assert hasattr(pkg.Batch, "profile_int")
