"""banded_ext_oracle.py against itself and against banded_oracle.py, without a GPU: the numpy form equals the scalar three-matrix DP on
random small pairs, bands and drops; without a drop the score is the banded NW score where that call's band is valid and the end is
(n, m); and the two identities of include/pwalign.h that need no device."""
import random

import pytest

import banded_ext_oracle as XO
import banded_oracle as BO
from test_gpu_banded import SCORINGS

ALL_SCORINGS = SCORINGS + [(1, -1, 0, 0)]       # ... and one where everything ties
XDROPS = [-1, 0, 3, 10, 1 << 27]


def _cases(seed, count):
    rng = random.Random(seed)
    pairs, bands = [], []
    for k in range(count):
        n, m = rng.randint(1, 40), rng.randint(1, 40)
        t = bytes(rng.choice(b"ACGT") for _ in range(m))
        p = bytearray(t[:n]) if rng.random() < 0.7 else bytearray()
        for x in range(len(p)):
            if rng.random() < 0.15:
                p[x] = rng.choice(b"ACGT")
        if p and rng.random() < 0.3:   # ... with an indel
            at = rng.randrange(len(p))
            p = p[:at] + p[at + rng.randint(1, 3):] if rng.random() < 0.5 else p[:at] + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 3))) + p[at:]
        p = bytes(p[:n]) + bytes(rng.choice(b"ACGT") for _ in range(n - len(p[:n])))
        if k % 8 == 0:   # an exact copy: the extension runs to the corner
            p = t
        lo, hi = rng.choice([(0, 0), (-rng.randint(0, 5), rng.randint(0, 5)), (-rng.randint(0, 45), rng.randint(0, 45))])
        pairs.append((p, t))
        bands.append((lo, hi))
    return pairs, bands


@pytest.fixture(scope="module")
def cases():
    return _cases(101, 320)


@pytest.mark.parametrize("sc", ALL_SCORINGS)
@pytest.mark.parametrize("xdrop", XDROPS)
def test_numpy_equals_scalar(cases, sc, xdrop):
    pairs, bands = cases
    got = XO.extend_many(pairs, bands, sc[:2], *sc[2:], xdrop)
    stopped = 0
    for k, ((p, t), band) in enumerate(zip(pairs, bands)):
        want = XO.scalar_dp(p, t, band, sc[:2], *sc[2:], xdrop)
        assert got[k] == want, (k, p, t, band, sc, xdrop)
        stopped += want["rows"] < len(p)
    assert xdrop == 1 << 27 or stopped >= 10   # (the cases do stop early; with the largest drop only a band that leaves the matrix does)


@pytest.mark.parametrize("sc", ALL_SCORINGS)
def test_no_drop_is_the_banded_nw_score_where_it_ends_in_the_corner(cases, sc):
    pairs, bands = cases
    got = XO.extend_many(pairs, bands, sc[:2], *sc[2:], -1)
    hits = 0
    for k, ((p, t), band) in enumerate(zip(pairs, bands)):
        if BO.band_valid("nw", len(p), len(t), *band) and got[k]["end"] == (len(p), len(t)):
            assert got[k]["score"] == BO.align(p, t, band, "nw", sc[:2], *sc[2:])["score"], (k, band)
            hits += 1
    assert hits >= 10


@pytest.mark.parametrize("sc", ALL_SCORINGS)
def test_identity_1_score_is_the_maximum_over_the_band_with_zero(cases, sc):
    pairs, bands = cases
    got = XO.extend_many(pairs, bands, sc[:2], *sc[2:], -1)
    for k, ((p, t), band) in enumerate(zip(pairs, bands)):
        H = XO.scalar_dp(p, t, band, sc[:2], *sc[2:], -1, matrix=True)["H"]
        cells = [H[i][j] for i in range(1, len(p) + 1) for j in range(1, len(t) + 1) if band[0] <= j - i <= band[1]]
        assert got[k]["score"] == max(cells + [0]), (k, band)


@pytest.mark.parametrize("sc", ALL_SCORINGS)
@pytest.mark.parametrize("xdrop", [0, 3, 10])
def test_identity_2_a_stop_below_the_end_row_changes_nothing(cases, sc, xdrop):
    pairs, bands = cases
    free = XO.extend_many(pairs, bands, sc[:2], *sc[2:], -1)
    got = XO.extend_many(pairs, bands, sc[:2], *sc[2:], xdrop)
    same = 0
    for k, (f, g) in enumerate(zip(free, got)):
        assert g["rows"] <= f["rows"], k
        if g["rows"] >= f["end"][0]:   # the stop row r* = rows + 1 lies below the end row
            assert (g["score"], g["end"], g["ops"]) == (f["score"], f["end"], f["ops"]), (k, bands[k])
            same += 1
        else:
            assert g["score"] <= f["score"], k
    assert same >= 10


def test_empty_sides_and_the_anchor():
    z = dict(score=0, end=(0, 0), start=(0, 0), ops=b"", rows=0)
    for p, t, pend in [(b"", b"", (0, 0)), (b"ACG", b"", None), (b"", b"ACG", (0, 0))]:
        assert XO.extend(p, t, (0, 0), (1, -4), -6, -1, 5) == dict(z, pend=pend) == XO.scalar_dp(p, t, (0, 0), (1, -4), -6, -1, 5)
    # first symbols differ: nothing beats the anchor
    r = XO.extend(b"AAAA", b"CAAA", (-1, 1), (1, -4), -6, -1, -1)
    assert (r["score"], r["end"], r["ops"]) == (0, (0, 0), b"")
    assert XO.band_valid(3, 3, -1, 0) and not XO.band_valid(3, 3, 1, 2) and not XO.band_valid(3, 3, -2, -1)
