"""hw3's alignments of long pairs: the stripe engine's affine traceback fill and walk (pair_affine_tb.hip.h), their routing in
pwa_align_affine_batch, and hw3_amd on the reference's own long inputs (fixtures: tests/golden/make_golden_hw3_align_long.py)."""
import gzip
import hashlib
import os
import random
import re
import subprocess

import pytest

import oracle_lib as O
from conftest import GOLDEN, load_golden, switched_context

README = (5, -4, -16, -4)
SCORINGS = [README, (1, -1, -2, -1), (1, -1, 0, -1), (2, -1, -3, 1), (0, 0, 0, 0)]


def sha(ops):
    return hashlib.sha256(ops).hexdigest()


def small_file():
    return [s for _, s in O.read_fasta_hw3(os.path.join(GOLDEN, load_golden("hw3_align_long")["center_pairs"]["file"]))]


def big_seqs(tmp_path):
    path = tmp_path / "big.fa"
    path.write_bytes(gzip.decompress(open(os.path.join(GOLDEN, "hw4_input16100000.fasta.gz"), "rb").read()))
    return [s for _, s in O.read_fasta_hw3(str(path))], str(path)


def rescore(s1, s2, ops, match, mismatch, go, ge):
    """An op list in traceback order under hw3's rules: degaps to (s1, s2), a leading gap run costs go + ge (L - 1) (hw3.cpp:42-53),
    any other run go + ge L (70-82), and no 'I' run touches a 'D' run (a gap state is only ever left for V).  Returns the score."""
    fwd = ops[::-1]
    i = j = 0
    total = 0
    k = 0
    while k < len(fwd):
        op = fwd[k]
        run = 1
        while k + run < len(fwd) and fwd[k + run] == op:
            run += 1
        if op == ord("M"):
            for d in range(run):
                total += match if s1[i + d] == s2[j + d] else mismatch
            i += run
            j += run
        else:
            assert op in (ord("D"), ord("I")), op
            if k + run < len(fwd):
                assert fwd[k + run] == ord("M"), "a gap run followed by the other gap"
            total += go + ge * (run - 1) if k == 0 else go + ge * run
            if op == ord("D"):
                i += run
            else:
                j += run
        k += run
    assert (i, j) == (len(s1), len(s2)), "the op list does not degap to its inputs"
    return total


def stripe_pairs(c):
    return c.align_affine_stats()["stripe_pairs"]


def test_fixture_agrees_with_oracle_and_rescorer():
    """CPU: the committed reference results equal the oracle's alignment on two pairs, and the rescorer reproduces their scores."""
    g = load_golden("hw3_align_long")
    cp = g["center_pairs"]
    assert tuple(cp["scoring"]) == README and len(cp["pairs"]) == 15
    seqs = small_file()
    for r in (cp["pairs"][0], cp["pairs"][11]):
        w = O.affine_align(seqs[r["a"]], seqs[r["b"]], *README)
        assert (w["score"], len(w["ops"]), sha(w["ops"])) == (r["score"], r["n_ops"], r["sha256"]), r
        assert rescore(seqs[r["a"]], seqs[r["b"]], w["ops"], *README) == r["score"]
    assert g["prefix"]["length"] == 20000 and len(g["prefix"]["pairs"]) >= 3


def mutate(rng, s, rate, alphabet):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out += bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 6)))
        out.append(rng.choice(alphabet) if r > 1 - rate / 3 else c)
    return bytes(out)


def shared_center(alphabet):
    """test_affine_alignments_against_a_shared_center's shape: one string1 against many string2, a second group, an empty pair."""
    rng = random.Random(len(alphabet))
    center = bytes(rng.choice(alphabet) for _ in range(211))
    others = [mutate(rng, center, rng.choice([0.01, 0.05, 0.2, 0.6]), alphabet) for _ in range(90)]
    others += [b"", center[:1], center, center[:33], center[5:70], bytes(rng.choice(alphabet) for _ in range(150))]
    center2 = bytes(rng.choice(alphabet) for _ in range(37))
    seqs = [center, center2] + others
    pa = [0] * len(others) + [1] * 20 + [2]
    pb = list(range(2, 2 + len(others))) + list(range(2, 22)) + [0]
    return seqs, pa, pb


def geometry_cases():
    """Lengths on both sides of a stripe (256 rows) and of a workgroup's four stripes (1024 rows), n >> m and m >> n, one-symbol
    sequences, a 3000-base insertion / deletion across stripe and window boundaries, identical sequences."""
    rng = random.Random(77)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))   # noqa: E731
    seqs, pa, pb = [], [], []

    def add(a, b):
        seqs.extend([a, b])
        pa.append(len(seqs) - 2)
        pb.append(len(seqs) - 1)
    for n in (255, 256, 257, 1023, 1024, 1025):
        base = rnd(n)
        add(base, mutate(rng, base, 0.1, b"ACGT"))
        add(base, rnd(n + 300))
    add(rnd(3000), rnd(40))
    add(rnd(40), rnd(3000))
    add(rnd(1), rnd(500))
    add(rnd(500), rnd(1))
    add(rnd(1), rnd(1))
    s = rnd(4000)
    add(s, s[:1700] + rnd(3000) + s[1700:])
    add(s[:900] + rnd(3000) + s[900:], s)
    add(s, s)
    return seqs, pa, pb


def check_exact(c, seqs, pa, pb, sc):
    got = c.align_affine_batch(seqs, pa, pb, *sc)
    for k, g in enumerate(got):
        w = O.affine_align(seqs[pa[k]], seqs[pb[k]], *sc)
        assert g["score"] == w["score"], (sc, k, len(seqs[pa[k]]), len(seqs[pb[k]]))
        assert g["ops"] == w["ops"], (sc, k, len(seqs[pa[k]]), len(seqs[pb[k]]))
    return got


@pytest.mark.gpu
def test_forced_stripes_match_oracle():
    """Fails without the feature: PWA_AFFINE_TB_ROUTE=1 runs every non-empty pair on the stripe engine, with the oracle's ops and
    scores for three alphabets, five scorings and the stripe geometry's edge cases."""
    with switched_context(PWA_AFFINE_TB_ROUTE="1") as c:
        for alphabet in (b"ACGT", b"AC", bytes(range(33, 127))):
            seqs, pa, pb = shared_center(alphabet)
            live = sum(1 for a, b in zip(pa, pb) if seqs[a] and seqs[b])
            for sc in SCORINGS:
                check_exact(c, seqs, pa, pb, sc)
                assert stripe_pairs(c) == live, (alphabet, sc)
        seqs, pa, pb = geometry_cases()
        for sc in (README, (2, -1, -3, 1)):
            check_exact(c, seqs, pa, pb, sc)
            st = c.align_affine_stats()
            assert st["stripe_pairs"] == len(pa) and st["band_bytes"] > 0 and st["fill_ms"] > 0 and st["walk_ms"] > 0, st


@pytest.mark.gpu
def test_strip_route_and_small_chunks(capfd):
    """PWA_AFFINE_TB_ROUTE=0 keeps every pair on the strips; a small PWA_RANGE_BYTES cuts the stripe pairs into several chunks.  Both
    give the oracle's results."""
    seqs, pa, pb = geometry_cases()
    with switched_context(PWA_AFFINE_TB_ROUTE="0") as c:
        check_exact(c, seqs, pa, pb, README)
        assert stripe_pairs(c) == 0
    with switched_context(PWA_AFFINE_TB_ROUTE="1", PWA_RANGE_BYTES=str(1 << 20), PWA_DEBUG="1") as c:
        capfd.readouterr()
        check_exact(c, seqs, pa, pb, README)
        assert stripe_pairs(c) == len(pa)
        err = capfd.readouterr().err
    m = re.search(r"align_affine stripes: (\d+) pairs in (\d+) chunk", err)
    assert m and int(m.group(1)) == len(pa) and int(m.group(2)) > 3, err[-2000:]


@pytest.mark.gpu
def test_10kb_center_pairs_default_route(ctx):
    """The 15 alignments hw3 builds against the center of the 10 kb file run on the stripe engine by default, with the reference's
    op lists."""
    cp = load_golden("hw3_align_long")["center_pairs"]
    seqs = small_file()
    pa = [r["a"] for r in cp["pairs"]]
    pb = [r["b"] for r in cp["pairs"]]
    got = ctx.align_affine_batch(seqs, pa, pb, *README)
    assert stripe_pairs(ctx) == 15
    for g, r in zip(got, cp["pairs"]):
        assert (g["score"], len(g["ops"]), sha(g["ops"])) == (r["score"], r["n_ops"], r["sha256"]), r


@pytest.mark.gpu
def test_20kb_prefixes_of_100kb_file(ctx, tmp_path):
    """20 000-base prefixes of the 100 kb file: many super-stripes, hand-offs through HBM; op lists equal the reference's."""
    g = load_golden("hw3_align_long")["prefix"]
    big, _ = big_seqs(tmp_path)
    L = g["length"]
    for r in g["pairs"]:
        got = ctx.align_affine_batch([big[r["a"]][:L], big[r["b"]][:L]], [0], [1], *r["scoring"])[0]
        assert stripe_pairs(ctx) == 1
        assert (got["score"], len(got["ops"]), sha(got["ops"])) == (r["score"], r["n_ops"], r["sha256"]), r


@pytest.mark.gpu
def test_100kb_file_center_alignments_and_cli(ctx, pkg, tmp_path):
    """Fails without the feature (PWA_E_NOMEM on the strips): sequence 0 of the 100 kb file against the other 15, plus the pinned
    pairs of hw3_long.json.  The reference runs out of memory at this size, so tie-break parity cannot be pinned here: the
    pinned scores equal the oracle's, and every op list degaps to its inputs and rescores to its score (optimality).  Then
    hw3_amd on the file exits 0 and writes 16 rows of equal width that degap to the inputs."""
    pinned = load_golden("hw3_long")["oracle_full"]["pairs"]
    big, path = big_seqs(tmp_path)
    pa = [0] * 15 + [r["a"] for r in pinned if r["a"] != 0]
    pb = list(range(1, 16)) + [r["b"] for r in pinned if r["a"] != 0]
    got = ctx.align_affine_batch(big, pa, pb, *README)
    assert stripe_pairs(ctx) == len(pa)
    for r in pinned:
        assert tuple(r["scoring"]) == README
        k = next(q for q in range(len(pa)) if (pa[q], pb[q]) == (r["a"], r["b"]))
        assert got[k]["score"] == r["score"], r
    for k, g in enumerate(got):
        assert rescore(big[pa[k]], big[pb[k]], g["ops"], *README) == g["score"], k
    pr = subprocess.run([pkg.HW3_CLI_PATH, "-i", path, "-o", "out.phy", "-s", ":".join(str(x) for x in README)], cwd=tmp_path,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    rows = (tmp_path / "out.phy").read_bytes().split(b"\n")
    assert rows[-1] == b"" and len(rows) == 18, len(rows)
    width = int(rows[0].split(b" ")[1])
    bodies = sorted(row[10:].replace(b" ", b"") for row in rows[1:-1])
    assert all(len(b) == width for b in bodies)
    assert sorted(b.replace(b"-", b"") for b in bodies) == sorted(big)


@pytest.mark.gpu
def test_lists_outside_the_guard_stay_on_the_strips():
    """(n + m + 2) * max(|score|) >= 2^26: even PWA_AFFINE_TB_ROUTE=1 keeps the list on the strips, and it stays exact."""
    rng = random.Random(5)
    s1 = bytes(rng.choice(b"ACGT") for _ in range(400))
    seqs = [s1, mutate(rng, s1, 0.1, b"ACGT"), bytes(rng.choice(b"ACGT") for _ in range(300))]
    with switched_context(PWA_AFFINE_TB_ROUTE="1") as c:
        check_exact(c, seqs, [0, 0], [1, 2], (200000, -150000, -300000, -1000))
        assert stripe_pairs(c) == 0
        check_exact(c, seqs, [0, 0], [1, 2], README)   # the same list inside the guard moves
        assert stripe_pairs(c) == 2
