"""The WFA oracle (wfa_oracle.py) against the affine-gap DP oracle (gotoh_oracle.py, mode nw): the conversion to penalties, the sweep with
its trim rule, the backtrace with its tie rules and the bound, without a GPU."""
import random

import pytest

import gotoh_oracle as GO
import wfa_oracle as WO

SCORINGS = [(5, -4, -16, -4), (1, -1, 0, -1), (0, -4, -6, -2), (3, 1, -2, -1), (-1, -3, 0, -2), (1, -4, -6, -1), (2, -3, -5, -2)]


def mutate(rng, s, rate, alphabet=b"ACGT"):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice(alphabet))
            out.append(c)
        elif r < rate:
            out.append(rng.choice(alphabet))
        else:
            out.append(c)
    return bytes(out)


def pairs(seed, count=60):
    rng = random.Random(seed)
    out = [(b"", b""), (b"ACGT", b""), (b"", b"ACGTA"), (b"A", b"C"), (b"A", b"A"), (b"ACGTACGTAC", b"ACGTACGTAC")]
    for _ in range(count):
        n = rng.randint(0, 40)
        p = bytes(rng.choice(b"ACGT") for _ in range(n))
        kind = rng.randint(0, 2)
        if kind == 0:
            t = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 40)))
        elif kind == 1:
            t = mutate(rng, p, rng.choice([0.05, 0.2, 0.5]))
        else:
            cut = rng.randint(0, n)
            t = p[:cut] + bytes(rng.choice(b"AC") for _ in range(rng.randint(0, 12))) + p[cut:]
            if rng.random() < 0.5:
                p, t = t, p
        out.append((p, t))
    return out


def consumed(ops):
    return ops.count(b"M") + ops.count(b"D"), ops.count(b"M") + ops.count(b"I")


@pytest.mark.parametrize("sc", SCORINGS)
def test_score_and_ops_against_the_dp(sc):
    match, mismatch, go, ge = sc
    for p, t in pairs(sum(sc) + 17):
        want = GO.align(p, t, "nw", (match, mismatch), go, ge, want_ops=False)["score"]
        got = WO.align(p, t, match, mismatch, go, ge)
        assert got["score"] == want, (p, t)
        assert consumed(got["ops"]) == (len(p), len(t)), (p, t)
        assert GO.op_score(p, t, got["ops"], (0, 0), (match, mismatch), go, ge) == want, (p, t, got["ops"])
        x, o, e, g = WO.penalties(*sc)
        assert got["cells"] == WO.cells_to(got["penalty"], len(p), len(t), o, e)


@pytest.mark.parametrize("sc", SCORINGS[:4])
def test_bound_at_the_optimum_and_one_above(sc):
    match, mismatch, go, ge = sc
    x, o, e, g = WO.penalties(*sc)
    for p, t in pairs(sum(sc) + 5, count=25):
        best = WO.align(p, t, match, mismatch, go, ge)
        at = WO.align(p, t, match, mismatch, go, ge, min_score=best["score"])
        assert at["score"] == best["score"] and at["ops"] == best["ops"] and at["penalty"] == best["penalty"]
        above = WO.align(p, t, match, mismatch, go, ge, min_score=best["score"] + 1)
        assert above["score"] is None and above["ops"] == b"" and above["penalty"] is None
        p_max, cells = WO.plan(len(p), len(t), match, mismatch, go, ge, best["score"] + 1)
        assert above["cells"] == cells                         # 0 when the host decides, the whole plan when the sweep runs out
        far = WO.align(p, t, match, mismatch, go, ge, min_score=-(1 << 20))
        assert far == best


def test_penalties_and_invalid_scorings():
    assert WO.penalties(1, -4, -6, -1) == (10, 12, 3, 1)
    assert WO.penalties(0, -4, -6, -2) == (2, 3, 1, 4)
    assert WO.penalties(1, -1, 0, -1) == (4, 0, 3, 1)
    for bad in [(1, 1, -1, -1), (2, 3, -1, -1), (0, -1, -1, 0), (-2, -3, 0, -1), (1, 0, 1, -1), (1, 0, -1, 1)]:
        with pytest.raises(ValueError):
            WO.penalties(*bad)


def test_widths_and_host_side_not_found():
    # 1/-4/-6/-1: x, o, e = 10, 12, 3
    assert [WO.khi(s, 12, 3) for s in (0, 14, 15, 17, 18, 30)] == [0, 0, 1, 1, 2, 6]
    assert WO.span(30, 2, 4, 12, 3) == (-2, 4)
    assert WO.plan(5, 5, 1, -4, -6, -1, None) == (2 * (12 + 15), WO.cells_to(54, 5, 5, 12, 3))
    assert WO.plan(5, 5, 1, -4, -6, -1, 6) == (None, 0)               # above the score of identical sequences: P_max < 0
    assert WO.plan(5, 8, 1, -4, -6, -1, -2) == (None, 0)             # one gap of 3 costs 21, the bound leaves 17
    assert WO.plan(5, 8, 1, -4, -6, -1, -4)[0] == 21
    assert WO.plan(0, 0, 1, -4, -6, -1, None) == (0, 1)
