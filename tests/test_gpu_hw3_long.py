"""hw3's score pass on few long sequences: the stripe engine's affine fill (pair_affine.hip.h), its routing in batch_create_impl,
and the hw3-compatible CLI on the reference's own long inputs (fixtures: tests/golden/make_golden_hw3_long.py)."""
import gzip
import os
import random
import subprocess

import pytest

import oracle_lib as O
from conftest import GOLDEN, load_golden, switched_context

STRIPE = "pair_affine_kernel<"
STRIP = "batch_affine_kernel"
README = (5, -4, -16, -4)


def long_file():
    g = load_golden("hw3_long")
    recs = O.read_fasta_hw3(os.path.join(GOLDEN, g["file"]))
    return g, recs


def big_seqs(tmp_path):
    path = tmp_path / "big.fa"
    path.write_bytes(gzip.decompress(open(os.path.join(GOLDEN, "hw4_input16100000.fasta.gz"), "rb").read()))
    return [s for _, s in O.read_fasta_hw3(str(path))]


def all_pairs(n):
    pa = [i for i in range(n) for j in range(i + 1, n)]
    pb = [j for i in range(n) for j in range(i + 1, n)]
    return pa, pb


def key(sc):
    return "%d,%d,%d,%d" % tuple(sc)


def test_long_fixture_is_self_consistent():
    """CPU: the committed reference scores of the 10 kb file agree with the oracle on a few pairs, the stored center is the
    oracle's pick from them, and every row of the committed output.phy is its input sequence once the gaps are removed."""
    g, recs = long_file()
    seqs = [s for _, s in recs]
    n = len(seqs)
    assert n == 16 and all(10000 <= len(s) <= 10010 for s in seqs)
    pa, pb = all_pairs(n)
    assert [tuple(p) for p in g["pairs"]] == list(zip(pa, pb))
    for k, want in g["scores"].items():
        sc = [int(x) for x in k.split(",")]
        assert len(want) == 120
        for q in (0, 57, 119):
            assert O.affine_score(seqs[pa[q]], seqs[pb[q]], *sc) == want[q], (k, q)
        assert O.center(want, n)[0] == g["center"][k], k
    phy = g["phy"]["output"].encode("latin-1").split(b"\n")
    assert phy[-1] == b"" and len(phy) == n + 2
    c = g["center"][key(g["phy"]["scoring"])]
    order = list(range(n))
    order[0], order[c] = order[c], order[0]   # hw3.cpp:328-329: the center is written first
    width = int(phy[0].split(b" ")[1])
    for row, k in zip(phy[1:-1], order):
        h, s = recs[k]
        assert row[:10] == h[:10].ljust(10)
        body = row[10:].replace(b" ", b"")
        assert len(body) == width and body.replace(b"-", b"") == s, k


@pytest.mark.gpu
def test_long_pairs_and_forced_route_report_the_stripe_kernel(ctx):
    """Fails without the feature: 16 x 10 kb all-pairs runs on the stripe engine by default, and a forced route moves a
    short list off the strips entirely, exact against the oracle."""
    _, recs = long_file()
    seqs = [s for _, s in recs]
    pa, pb = all_pairs(len(seqs))
    b = ctx.batch_affine(seqs, pa, pb, *README)
    assert STRIPE in b.info()["kernel"], b.info()["kernel"]
    b.close()
    short = [O.gen(5, 2, i, 300 + 7 * i) for i in range(10)]
    spa, spb = all_pairs(len(short))
    with switched_context(PWA_SCORES_ROUTE="1") as c:
        b = c.batch_affine(short, spa, spb, *README)
        kern = b.info()["kernel"]
        b.close()
        assert kern.startswith(STRIPE) and STRIP not in kern, kern
        assert c.scores_affine(short, spa, spb, *README) == [O.affine_score(short[a], short[b2], *README) for a, b2 in zip(spa, spb)]


@pytest.mark.gpu
def test_reference_long_file_scores(ctx):
    """16 x 10 kb (the reference's input1610000.fasta): both calls against the compiled reference's 120 scores, two scorings."""
    g, recs = long_file()
    seqs = [s for _, s in recs]
    pa, pb = all_pairs(len(seqs))
    for k, want in g["scores"].items():
        sc = [int(x) for x in k.split(",")]
        assert ctx.scores_affine(seqs, pa, pb, *sc) == want, k
        assert ctx.scores_affine_oneshot(seqs, pa, pb, *sc) == want, k


@pytest.mark.gpu
def test_reference_long_file_output_phy(pkg, tmp_path):
    """hw3_amd on the 10 kb file writes the reference's output.phy byte for byte (the alignment phase is the untouched
    one-wave traceback kernel: a generous time limit)."""
    g, _ = long_file()
    sc = ":".join(str(x) for x in g["phy"]["scoring"])
    pr = subprocess.run([pkg.HW3_CLI_PATH, "-i", os.path.join(GOLDEN, g["file"]), "-o", "out.phy", "-s", sc], cwd=tmp_path,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    assert pr.returncode == 0, pr.stderr
    assert (tmp_path / "out.phy").read_bytes() == g["phy"]["output"].encode("latin-1")


@pytest.mark.gpu
def test_long_prefixes_beyond_one_workgroup(ctx, tmp_path):
    """Pairs of the 100 kb file across many super-stripes (the (M, G) row hand-off through HBM): 20 000-base prefixes pinned
    by the compiled reference, 40 000-base prefixes and whole 100 kb pairs by the oracle."""
    g = load_golden("hw3_long")
    big = big_seqs(tmp_path)
    cases = [(big[r["a"]][:g["prefix"]["length"]], big[r["b"]][:g["prefix"]["length"]], r) for r in g["prefix"]["pairs"]]
    cases += [(big[r["a"]][:g["oracle_prefix"]["length"]], big[r["b"]][:g["oracle_prefix"]["length"]], r) for r in g["oracle_prefix"]["pairs"]]
    cases += [(big[r["a"]], big[r["b"]], r) for r in g["oracle_full"]["pairs"]]
    for s1, s2, r in cases:
        b = ctx.batch_affine([s1, s2], [0], [1], *r["scoring"])
        assert STRIPE in b.info()["kernel"], b.info()["kernel"]
        b.close()
        assert ctx.scores_affine([s1, s2], [0], [1], *r["scoring"]) == [r["score"]], (len(s1), r)


@pytest.mark.gpu
def test_full_100kb_file_all_pairs(ctx, tmp_path):
    """16 x 100 kb, all 120 pairs (the reference runs out of memory): the pass completes on the stripe engine and equals the
    oracle on the pinned pairs."""
    g = load_golden("hw3_long")["oracle_full"]
    big = big_seqs(tmp_path)
    pa, pb = all_pairs(len(big))
    b = ctx.batch_affine(big, pa, pb, *README)
    assert STRIPE in b.info()["kernel"] and STRIP not in b.info()["kernel"], b.info()["kernel"]
    b.close()
    got = ctx.scores_affine(big, pa, pb, *README)
    for r in g["pairs"]:
        assert r["scoring"] == list(README)
        assert got[pa.index(r["a"]) + (r["b"] - r["a"] - 1)] == r["score"], r


def forced_cases():
    """(sequences, pair_a, pair_b): the edge lengths of the stripe geometry (RL = 2: 128-row stripes, 512-row workgroups; RL = 4
    above 32k rows is covered by the prefixes), one and many workgroups, m shorter and longer than n, a self-pair."""
    rng = random.Random(381)
    lens = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1025, 1537, 2049, 2900]
    cases = []
    for alpha in (b"ACGT", b"AC"):
        seqs = [bytes(rng.choice(alpha) for _ in range(n)) for n in lens]
        seqs += [bytes(rng.choice(alpha) for _ in range(n)) for n in (1, 5, 40, 63)]   # m < 64, m = 1
        k = len(seqs)
        pa, pb = [], []
        for a in range(k):
            for b in rng.sample(range(k), 4):
                pa.append(a)
                pb.append(b)
        pa += [k - 3, 0, len(lens) - 1, len(lens)]   # self-pair, 1 x 2900, 2900 x 1, 1 x 1
        pb += [k - 3, len(lens) - 1, 0, len(lens)]
        cases.append((seqs, pa, pb))
    return cases


# inside the guard: README's, positive gap open / extend, mismatch > match, zeros
FORCED_SCORINGS = [README, (2, -3, -5, -2), (1, 3, 2, 1), (-2, 4, 3, -1), (0, 0, 0, 0), (7, -7, 5, 6), (1, -1, 0, -1)]


@pytest.mark.gpu
def test_forced_stripe_route_matches_oracle():
    """Every pair on the stripe engine (PWA_SCORES_ROUTE=1) against the oracle, for every edge of the geometry."""
    with switched_context(PWA_SCORES_ROUTE="1") as c:
        for seqs, pa, pb in forced_cases():
            for sc in FORCED_SCORINGS:
                b = c.batch_affine(seqs, pa, pb, *sc)
                kern = b.info()["kernel"]
                b.close()
                assert kern.startswith(STRIPE) and STRIP not in kern, (sc, kern)
                got = c.scores_affine(seqs, pa, pb, *sc)
                want = [O.affine_score(seqs[a], seqs[b2], *sc) for a, b2 in zip(pa, pb)]
                bad = [k for k in range(len(pa)) if got[k] != want[k]]
                assert not bad, (sc, [(len(seqs[pa[k]]), len(seqs[pb[k]]), got[k], want[k]) for k in bad[:5]])


@pytest.mark.gpu
def test_lists_outside_the_guard_stay_on_the_strips():
    """A raw-byte alphabet (more than 7 symbols) and scores past 2^28 stay on batch_affine_kernel even when forced, exact."""
    rng = random.Random(11)
    wide = [bytes(rng.choice(bytes(range(65, 91))) for _ in range(n)) for n in (2500, 2400, 1700)]
    dna = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (2500, 2400, 1700)]
    with switched_context(PWA_SCORES_ROUTE="1") as c:
        for seqs, sc in ((wide, README), (dna, (100, -90, -300, -70)), (dna, (5, -4, -16, -60000))):
            b = c.batch_affine(seqs, [0, 1], [1, 2], *sc)
            kern = b.info()["kernel"]
            b.close()
            assert kern.startswith(STRIP) and STRIPE not in kern, (sc, kern)
            assert c.scores_affine(seqs, [0, 1], [1, 2], *sc) == [O.affine_score(seqs[a], seqs[b2], *sc) for a, b2 in [(0, 1), (1, 2)]], sc


@pytest.mark.gpu
def test_split_batch_matches_oracle(ctx):
    """A few 10 kb pairs among many 300 bp pairs: the long pairs leave the strips, the short ones -- full wave tasks, where the
    strips are the cheaper engine per cell -- stay; both engines write into the one score vector in pair order."""
    rng = random.Random(98)
    longs = [bytes(rng.choice(b"ACGT") for _ in range(10000)) for _ in range(4)]
    texts = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(290, 310))) for _ in range(64)]
    pats = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(280, 320))) for _ in range(1200)]
    seqs = longs + texts + pats
    pa = [68 + p for t in range(64) for p in range(1200)]
    pb = [4 + t for t in range(64) for p in range(1200)]
    for at, (a, b) in zip((17, 40000, 40001, len(pa)), ((0, 1), (2, 3), (1, 2), (3, 0))):
        pa.insert(at, a)
        pb.insert(at, b)
    b = ctx.batch_affine(seqs, pa, pb, *README)
    kern = b.info()["kernel"]
    b.close()
    assert " + " in kern and kern.startswith(STRIP) and STRIPE in kern, kern
    got = ctx.scores_affine(seqs, pa, pb, *README)
    want = [O.affine_score(seqs[a], seqs[b2], *README) for a, b2 in zip(pa, pb)]
    assert got == want
