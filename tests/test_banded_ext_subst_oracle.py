"""banded_ext_oracle.py under substitution tables against itself and against banded_oracle.py, without a GPU: the numpy form equals
the scalar three-matrix DP on random small pairs, bands, drops and tables; under a match / mismatch table it is its own byte compare;
the pattern-end result is the banded NW score of the pattern against the text prefix it names; and the identities of
include/pwalign.h that need no device."""
import numpy as np
import pytest

import banded_ext_oracle as XO
import banded_oracle as BO
from conftest import load_pkg
from test_banded_ext_oracle import XDROPS, _cases

GAPS = [(-6, -1), (-1, -1)]


def _tables():
    pkg = load_pkg()
    rs = np.random.RandomState(5)
    asym = rs.randint(-5, 4, size=(4, 4))
    asym[np.arange(4), np.arange(4)] = [3, 2, 4, 1]
    assert (asym != asym.T).any()
    pos = np.full((4, 4), -3)
    pos[np.arange(4), np.arange(4)] = 4
    pos[0, 2] = pos[2, 0] = 1   # transitions score above zero
    pos[1, 3] = 2
    neg = -1 - rs.randint(0, 4, size=(4, 4))   # all negative: nothing ever beats the anchor
    mm = np.where(np.eye(4, dtype=bool), 1, -4)
    return {"asym": pkg.subst_table(b"ACGT", asym), "pos": pkg.subst_table(b"ACGT", pos), "neg": pkg.subst_table(b"ACGT", neg),
            "mm": pkg.subst_table(b"ACGT", mm)}


TABLES = _tables()


@pytest.fixture(scope="module")
def cases():
    return _cases(211, 240)


@pytest.mark.parametrize("name", ["asym", "pos", "neg"])
@pytest.mark.parametrize("gaps", GAPS)
def test_numpy_equals_scalar(cases, name, gaps):
    pairs, bands = cases
    got = XO.extend_multi(pairs, bands, TABLES[name], *gaps, XDROPS)
    stopped = with_pend = below = 0
    for xdrop in XDROPS:
        for k, ((p, t), band) in enumerate(zip(pairs, bands)):
            want = XO.scalar_dp(p, t, band, TABLES[name], *gaps, xdrop)
            assert got[xdrop][k] == want, (k, p, t, band, name, gaps, xdrop)
            stopped += want["rows"] < len(p)
            with_pend += want["pend"] is not None
            below += want["pend"] is not None and want["pend"][0] < want["score"]
            assert (want["pend"] is not None) == (want["rows"] == len(p))
            if name == "neg":
                assert (want["score"], want["end"], want["ops"]) == (0, (0, 0), b"")
    assert stopped >= 10 and with_pend >= 10 and below >= 10   # (early stops, pattern ends, and pattern ends below the best)


@pytest.mark.parametrize("sc", [(1, -4, -6, -1), (2, -3, 0, -2)])
@pytest.mark.parametrize("xdrop", XDROPS)
def test_match_mismatch_table_is_the_byte_compare_oracle(cases, sc, xdrop):
    pairs, bands = cases
    table = load_pkg().subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), sc[0], sc[1]))
    got = XO.extend_many(pairs, bands, table, sc[2], sc[3], xdrop)
    want = XO.extend_many(pairs, bands, sc[:2], sc[2], sc[3], xdrop)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, bands[k])   # (every key, the pattern end among them)


@pytest.mark.parametrize("name", ["asym", "pos"])
@pytest.mark.parametrize("xdrop", [-1, 10])
def test_pattern_end_is_the_banded_nw_score_of_the_text_prefix(cases, name, xdrop):
    pairs, bands = cases
    got = XO.extend_many(pairs, bands, TABLES[name], -6, -1, xdrop)
    ks = [k for k, g in enumerate(got) if g["pend"] is not None and g["pend"][1] >= 1]
    assert len(ks) >= 10
    for k in ks:   # the cell (n, pend_j) is in the band: NW's validity on the prefix
        assert bands[k][0] <= got[k]["pend"][1] - len(pairs[k][0]) <= bands[k][1]
    nw = BO.align_many([(pairs[k][0], pairs[k][1][:got[k]["pend"][1]]) for k in ks], [bands[k] for k in ks], "nw", TABLES[name], -6, -1)
    assert [w["score"] for w in nw] == [got[k]["pend"][0] for k in ks]
    # ... and no other in-band column of row n does better, none before it as well (the first pairs: one NW fill per column)
    for k in ks[:12]:
        (p, t), band, pe = pairs[k], bands[k], got[k]["pend"]
        js = [j for j in range(1, len(t) + 1) if band[0] <= j - len(p) <= band[1]]
        col = BO.align_many([(p, t[:j]) for j in js], [band] * len(js), "nw", TABLES[name], -6, -1)
        for j, w in zip(js, col):
            assert w["score"] < pe[0] if j < pe[1] else w["score"] <= pe[0], (k, j)


@pytest.mark.parametrize("name", ["asym", "pos", "neg"])
def test_identity_1_score_is_the_maximum_over_the_band_with_zero(cases, name):
    pairs, bands = cases
    got = XO.extend_many(pairs, bands, TABLES[name], -6, -1, -1)
    for k, ((p, t), band) in enumerate(zip(pairs, bands)):
        H = XO.scalar_dp(p, t, band, TABLES[name], -6, -1, -1, matrix=True)["H"]
        cells = [H[i][j] for i in range(1, len(p) + 1) for j in range(1, len(t) + 1) if band[0] <= j - i <= band[1]]
        assert got[k]["score"] == max(cells + [0]), (k, band)


@pytest.mark.parametrize("name", ["asym", "pos"])
@pytest.mark.parametrize("xdrop", [0, 3, 10])
def test_identity_2_a_stop_below_the_end_row_changes_nothing(cases, name, xdrop):
    pairs, bands = cases
    both = XO.extend_multi(pairs, bands, TABLES[name], -6, -1, [-1, xdrop])
    same = 0
    for k, (f, g) in enumerate(zip(both[-1], both[xdrop])):
        assert g["rows"] <= f["rows"], k
        if g["rows"] >= f["end"][0]:   # the stop row r* = rows + 1 lies below the end row
            assert (g["score"], g["end"], g["ops"]) == (f["score"], f["end"], f["ops"]), (k, bands[k])
            same += 1
        else:
            assert g["score"] <= f["score"], k
        if g["pend"] is not None:      # a row n that the drop kept is the row n of the free sweep
            assert g["pend"] == f["pend"], k
    assert same >= 10


def test_empty_sides_and_the_anchor():
    t = TABLES["mm"]
    z = dict(score=0, end=(0, 0), start=(0, 0), ops=b"", rows=0)
    for p, q, pend in [(b"", b"", (0, 0)), (b"ACG", b"", None), (b"", b"ACG", (0, 0))]:
        want = dict(z, pend=pend)
        assert XO.extend(p, q, (0, 0), t, -6, -1, 5) == want == XO.scalar_dp(p, q, (0, 0), t, -6, -1, 5)
    # first symbols differ: nothing beats the anchor, but without a drop row n is kept and has its own (negative) best
    r = XO.extend(b"AAAA", b"CAAA", (-1, 1), t, -6, -1, -1)
    assert (r["score"], r["end"], r["ops"], r["rows"]) == (0, (0, 0), b"", 4) and r["pend"] == (-1, 4)
    # the band leaves the matrix before row n: no pattern end, with or without a drop
    for xdrop in (-1, 50):
        r = XO.extend(b"ACGTACGT", b"ACG", (-2, 2), t, -6, -1, xdrop)
        assert r["rows"] == 5 and r["pend"] is None
