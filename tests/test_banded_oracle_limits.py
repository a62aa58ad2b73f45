"""The banded numpy oracles at the int32 range limits of the four calls they restate, without a GPU: banded_oracle and banded_ext_oracle,
each under match / mismatch and under a substitution table, against their own scalar_dp on small pairs under the at-the-bound scorings that
test_gpu_banded_limits.py runs on the device -- A = top(n, m, 28) for the alignment calls and top(n, m, 27) for EXT, A as validate_align
(pwalign_align.hip) computes it.  The device tests lean on the numpy forms at these magnitudes, where nothing had compared them yet.

The scalar DPs hold no fixed-width value: every finite cell is a Python int (table entries go through int()), -inf is the float, and a
sum with it is -inf again -- asserted below on a whole matrix.  The numpy forms are int64 with -inf = -2^40, cut off at -2^39: the
largest sum of a real value and a sentinel here is below 2^28 - 2^40."""
import functools
import random

import numpy as np
import pytest

import banded_ext_oracle as XO
import banded_oracle as BO
from conftest import load_pkg

MODES = ["nw", "sw", "sg"]
SHAPES = [(60, 60), (57, 60), (60, 41), (1, 60), (60, 1), (24, 24)]
KINDS = ["positive", "negative", "open0", "extend0"]
XDROPS = [-1, 0, 10, 1 << 27]


def top(n, m, bits):
    """the largest A that the range rule (n + m + 2) * A < 2^bits admits"""
    t = ((1 << bits) - 1) // (n + m + 2)
    assert (n + m + 2) * t < 1 << bits <= (n + m + 2) * (t + 1)
    return t


def scoring(kind, t):
    """(match, mismatch, gap_open, gap_extend) with max(|match|, |mismatch|, |gap_open| + |gap_extend|) = t"""
    sc = {"positive": (t, -t, -(t // 3), -(t - t // 3)), "negative": (1, -t, -1, -(t - 1)), "open0": (1, -t, 0, -t),
          "extend0": (1, -t, -t, 0)}[kind]
    assert max(abs(sc[0]), abs(sc[1]), abs(sc[2]) + abs(sc[3])) == t
    return sc


def mm_table(match, mismatch):
    return load_pkg().subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), match, mismatch))


def asym_table(t, seed):
    """an asymmetric 4-symbol table with entries of both signs in [-t, t], one at each end"""
    m = np.random.RandomState(seed).randint(-t, t + 1, size=(4, 4)).astype(np.int64)
    m[np.arange(4), np.arange(4)] = np.abs(m[np.arange(4), np.arange(4)])
    m[0, 0], m[1, 2] = t, -t
    assert (m != m.T).any() and np.abs(m).max() == t
    return load_pkg().subst_table(b"ACGT", m)


@functools.lru_cache(maxsize=None)
def _pairs(n, m):
    """an exact copy (a prefix, where the lengths differ), a mutated copy, and a pair without a common symbol"""
    rng = random.Random(1000 * n + m)
    t = bytes(rng.choice(b"ACGT") for _ in range(m))
    p = (t + bytes(rng.choice(b"ACGT") for _ in range(n)))[:n]
    q = bytearray(p)
    for x in range(n):
        if rng.random() < 0.15:
            q[x] = rng.choice(b"ACGT")
    return [(p, t), (bytes(q), t), (bytes(rng.choice(b"AC") for _ in range(n)), bytes(rng.choice(b"GT") for _ in range(m)))]


def _bands(n, m, valid):
    """widths 1 and 7 (around diagonal 0, and around the corner diagonals where the lengths differ by less than 7) and the full
    cover, as far as `valid` takes them"""
    d = m - n
    cand = [("1", (0, 0)), ("1", (d, d)), ("7", (-3, 3)), ("full", (-n, m))]
    if abs(d) <= 6:
        lo = min(0, d) - (6 - abs(d)) // 2
        cand.append(("7", (lo, lo + 6)))
    seen, out = set(), []
    for w, b in cand:
        if b not in seen and valid(*b):
            seen.add(b)
            out.append((w, b))
    return out


def test_the_scalar_dps_hold_python_ints():
    t = top(24, 24, 27)
    p, q = _pairs(24, 24)[1]
    H = XO.scalar_dp(p, q, (-3, 3), asym_table(t, 3), -(t // 2), -(t - t // 2), -1, matrix=True)["H"]
    cells = [v for row in H for v in row]
    assert all(type(v) is int or v == float("-inf") for v in cells) and sum(type(v) is int for v in cells) > 100
    pos, neg = scoring("positive", t), scoring("negative", t)
    for r in (BO.scalar_dp(p, q, (-3, 3), "nw", pos[:2], *pos[2:]), XO.scalar_dp(p, q, (-3, 3), neg[:2], *neg[2:], 10)):
        assert type(r["score"]) is int


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_banded_and_banded_subst_equal_scalar_at_the_2_28_bound(mode, kind):
    widths, reach = set(), 0
    for n, m in SHAPES:
        t = top(n, m, 28)
        sc = scoring(kind, t)
        table = mm_table(sc[0], sc[1])
        named = _bands(n, m, lambda lo, hi: BO.band_valid(mode, n, m, lo, hi))
        pairs = [pt for pt in _pairs(n, m) for _ in named]
        bands = [b for _ in _pairs(n, m) for _, b in named]
        widths |= {w for w, _ in named}
        got = BO.align_many(pairs, bands, mode, sc[:2], *sc[2:])
        gots = BO.align_many(pairs, bands, mode, table, sc[2], sc[3])
        for k, ((p, q), band) in enumerate(zip(pairs, bands)):
            want = BO.scalar_dp(p, q, band, mode, sc[:2], *sc[2:])
            assert got[k] == want, (n, m, band, sc)
            assert gots[k] == want == BO.scalar_dp(p, q, band, mode, table, sc[2], sc[3]), (n, m, band, sc)
            reach = max(reach, abs(want["score"]))
    assert widths == {"1", "7", "full"}
    if kind != "extend0" and (mode != "sw" or kind == "positive"):   # (where a gap run costs per symbol, and SW's floor is not the answer)
        assert reach > 0.4 * (1 << 28)                               # the cases do reach the bound's size


@pytest.mark.parametrize("mode", MODES)
def test_banded_subst_equals_scalar_under_an_asymmetric_table_at_the_bound(mode):
    for n, m in SHAPES[:4]:
        t = top(n, m, 28)
        table = asym_table(t, n + m)
        named = _bands(n, m, lambda lo, hi: BO.band_valid(mode, n, m, lo, hi))
        for go, ge in [(-(t // 3), -(t - t // 3)), (0, -t), (-t, 0)]:
            pairs = [pt for pt in _pairs(n, m) for _ in named]
            bands = [b for _ in _pairs(n, m) for _, b in named]
            got = BO.align_many(pairs, bands, mode, table, go, ge)
            for k, ((p, q), band) in enumerate(zip(pairs, bands)):
                assert got[k] == BO.scalar_dp(p, q, band, mode, table, go, ge), (n, m, band, go, ge)


@pytest.mark.parametrize("kind", KINDS)
def test_ext_and_ext_subst_equal_scalar_at_the_2_27_bound(kind):
    widths, reach, low = set(), 0, 0
    for n, m in SHAPES:
        t = top(n, m, 27)
        sc = scoring(kind, t)
        table = mm_table(sc[0], sc[1])
        named = _bands(n, m, lambda lo, hi: XO.band_valid(n, m, lo, hi))
        pairs = [pt for pt in _pairs(n, m) for _ in named]
        bands = [b for _ in _pairs(n, m) for _, b in named]
        widths |= {w for w, _ in named}
        got = XO.extend_multi(pairs, bands, sc[:2], *sc[2:], XDROPS)
        gots = XO.extend_multi(pairs, bands, table, sc[2], sc[3], XDROPS)
        for xdrop in XDROPS:
            for k, ((p, q), band) in enumerate(zip(pairs, bands)):
                want = XO.scalar_dp(p, q, band, table, sc[2], sc[3], xdrop)
                assert gots[xdrop][k] == want, (n, m, band, sc, xdrop)
                pend = want["pend"]   # (compared with every other key: the byte compare gives the table's pattern end)
                assert got[xdrop][k] == want == XO.scalar_dp(p, q, band, sc[:2], *sc[2:], xdrop), (n, m, band, sc, xdrop)
                reach = max(reach, want["score"])
                low = min(low, pend[0] if pend else 0)
    assert widths == {"1", "7", "full"}
    assert kind != "positive" or reach > 0.4 * (1 << 27)
    assert kind == "extend0" or low < -0.4 * (1 << 27)


def test_ext_subst_equals_scalar_under_an_asymmetric_and_an_all_negative_table_at_the_bound():
    for n, m in SHAPES[:4]:
        t = top(n, m, 27)
        named = _bands(n, m, lambda lo, hi: XO.band_valid(n, m, lo, hi))
        pairs = [pt for pt in _pairs(n, m) for _ in named]
        bands = [b for _ in _pairs(n, m) for _, b in named]
        for table, go, ge in [(asym_table(t, n + m), -(t // 3), -(t - t // 3)), (load_pkg().subst_table(b"ACGT", np.full((4, 4), -t)), 0, -t)]:
            got = XO.extend_multi(pairs, bands, table, go, ge, XDROPS)
            for xdrop in XDROPS:
                for k, ((p, q), band) in enumerate(zip(pairs, bands)):
                    assert got[xdrop][k] == XO.scalar_dp(p, q, band, table, go, ge, xdrop), (n, m, band, go, ge, xdrop)
