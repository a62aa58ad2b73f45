"""hw4 on few long sequences: the stripe engine's distance fill (pair_dist.hip.h), its routing in batch_create_impl, and the
hw4-compatible CLI on the reference's own long inputs (fixtures: tests/golden/make_golden_hw4_long.py)."""
import gzip
import os
import random
import subprocess

import pytest

import oracle_lib as O
from conftest import GOLDEN, load_golden, switched_context
from test_gpu_hw4 import SCORINGS

STRIPE = "pair_dist_kernel<"
STRIP = "batch_nwdist"


def read_fasta_hw4(data):
    """hw4.cpp:109-134: '>' starts a record, every other non-empty line (one trailing CR dropped) is appended."""
    recs, name, seq = [], None, []
    for line in data.split(b"\n"):
        if not line:
            continue
        if line.endswith(b"\r"):
            line = line[:-1]
        if line[:1] == b">":
            if name is not None:
                recs.append((name, b"".join(seq)))
            name, seq = line[1:], []
        else:
            seq.append(line)
    if name is not None:
        recs.append((name, b"".join(seq)))
    return recs


def long_file():
    g = load_golden("hw4_long")
    recs = read_fasta_hw4(open(os.path.join(GOLDEN, g["file"]), "rb").read())
    return g, recs


def big_file():
    return read_fasta_hw4(gzip.decompress(open(os.path.join(GOLDEN, "hw4_input16100000.fasta.gz"), "rb").read()))


def all_pairs(n):
    pa = [i for i in range(n) for j in range(i + 1, n)]
    pb = [j for i in range(n) for j in range(i + 1, n)]
    return pa, pb


def test_long_fixture_tree_is_upgma_of_its_distances():
    """CPU: the committed reference tree is the oracle UPGMA of the committed reference distances (self-consistent fixture)."""
    g, recs = long_file()
    n = len(recs)
    assert n == 16 and all(10000 <= len(s) <= 10010 for _, s in recs)
    for key, tree in g["tree"].items():
        d = [[0.0] * n for _ in range(n)]
        for (i, j), v in zip(g["pairs"], g["dist"][key]):
            d[i][j] = d[j][i] = float(v)
        assert O.upgma(d, [h for h, _ in recs]) + b"\n" == tree.encode("latin-1"), key   # hw4.cpp writes the tree and endl


@pytest.mark.gpu
def test_long_pairs_and_forced_route_report_the_stripe_kernel(ctx):
    """Fails without the feature: 16 x 10 kb all-pairs runs on the stripe engine by default, and a forced route moves a list
    of short pairs (two-value form) off the strips entirely."""
    _, recs = long_file()
    seqs = [s for _, s in recs]
    pa, pb = all_pairs(len(seqs))
    b = ctx.batch_distances(seqs, pa, pb, 1, -1, -1)
    assert STRIPE in b.info()["kernel"] and "PACKED" not in b.info()["kernel"]
    b.close()
    short = [O.gen(5, 2, i, 300 + 7 * i) for i in range(10)]
    spa, spb = all_pairs(len(short))
    with switched_context(PWA_SCORES_ROUTE="1", PWA_NO_PACKED_DIST="1") as c:
        b = c.batch_distances(short, spa, spb, 1, -1, -1)
        kern = b.info()["kernel"]
        b.close()
        assert kern.startswith(STRIPE) and STRIP not in kern, kern
        assert c.distances(short, spa, spb, 1, -1, -1) == [O.nw_distance(short[a], short[c2], 1, -1, -1)[0] for a, c2 in zip(spa, spb)]


@pytest.mark.gpu
def test_reference_long_file_distances_and_tree(ctx, pkg, tmp_path):
    """16 x 10 kb (the reference's input1610000.fasta): both calls against the compiled reference's distances, and hw4_amd's
    tree bytes against the tree the reference writes."""
    g, recs = long_file()
    seqs = [s for _, s in recs]
    pa, pb = all_pairs(len(seqs))
    assert [tuple(p) for p in g["pairs"]] == list(zip(pa, pb))
    for key, want in g["dist"].items():
        sc = [int(x) for x in key.split(",")]
        assert ctx.distances(seqs, pa, pb, *sc) == want, key
        assert ctx.distances_oneshot(seqs, pa, pb, *sc) == want, key
        pr = subprocess.run([pkg.CLI4_PATH, "-i", os.path.join(GOLDEN, g["file"]), "-t", "tree.txt", "-s"] + [str(x) for x in sc],
                            cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert pr.returncode == 0, pr.stderr
        assert (tmp_path / "tree.txt").read_bytes() == g["tree"][key].encode("latin-1"), key


@pytest.mark.gpu
def test_long_prefixes_beyond_one_workgroup(ctx):
    """40 000-base prefixes of pairs of the 100 kb file: ~40 super-stripes per pair, the row hand-off through HBM; pinned by
    the compiled reference (~8 GB of its matrices per pair)."""
    g = load_golden("hw4_long")["prefix"]
    big = [s for _, s in big_file()]
    L = g["length"]
    for rec in g["pairs"]:
        seqs = [big[rec["a"]][:L], big[rec["b"]][:L]]
        b = ctx.batch_distances(seqs, [0], [1], *rec["scoring"])
        assert STRIPE in b.info()["kernel"]
        b.close()
        assert ctx.distances(seqs, [0], [1], *rec["scoring"]) == [rec["dist"]], rec


@pytest.mark.gpu
def test_full_100kb_file_completes_parity_unpinned_by_the_reference(ctx, pkg, tmp_path):
    """16 x 100 kb: parity unpinned by the reference (its matrices would take ~50 GB per pair).  The run completes, and
    hw4_amd's tree is the UPGMA of the library's own distance matrix."""
    recs = big_file()
    seqs = [s for _, s in recs]
    n = len(seqs)
    pa, pb = all_pairs(n)
    got = ctx.distances(seqs, pa, pb, 1, -1, -1)
    assert all(0 < v <= 200000 for v in got)
    d = [[0.0] * n for _ in range(n)]
    for i, j, v in zip(pa, pb, got):
        d[i][j] = d[j][i] = float(v)
    path = tmp_path / "in.fa"
    path.write_bytes(gzip.decompress(open(os.path.join(GOLDEN, "hw4_input16100000.fasta.gz"), "rb").read()))
    pr = subprocess.run([pkg.CLI4_PATH, "-i", str(path), "-t", "tree.txt", "-s", "1", "-1", "-1"], cwd=tmp_path,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert pr.returncode == 0, pr.stderr
    assert (tmp_path / "tree.txt").read_bytes() == pkg.upgma_newick(d, [h for h, _ in recs]) + b"\n"


def forced_cases():
    """(sequences, pair_a, pair_b): the edge lengths of the stripe geometry (RL = 2: 128-row stripes, 512-row workgroups;
    RL = 4 above 32k rows is covered by the prefixes), a self-pair, tie-heavy repeats, in ACGT and AC."""
    rng = random.Random(481)
    lens = [1, 2, 63, 64, 65, 127, 129, 511, 513, 1023, 1025, 1535, 1537, 2047, 2049, 2900]
    cases = []
    for alpha in (b"ACGT", b"AC"):
        seqs = [bytes(rng.choice(alpha) for _ in range(n)) for n in lens]
        seqs += [bytes(rng.choice(alpha) for _ in range(n)) for n in (1, 5, 40, 63)]   # m < 64, m = 1
        unit = alpha[:1] * 3 + alpha + alpha[-1:] * 9                                  # GATTACACCCC... in this alphabet
        rep = (unit * 200)[:1700]
        mut = bytearray(rep)
        for _ in range(30):
            mut[rng.randrange(len(mut))] = rng.choice(alpha)
        seqs += [rep, bytes(mut), rep[:1650] + alpha[:1] * 40]
        k = len(seqs)
        pa, pb = [], []
        for a in range(k):
            for b in rng.sample(range(k), 4):
                pa.append(a)
                pb.append(b)
        pa += [k - 3, k - 3, k - 2, 0, len(lens)]        # self-pair, the repeats against each other, 1 x 2900, 1 x 1
        pb += [k - 3, k - 2, k - 1, len(lens) - 1, len(lens)]
        cases.append((seqs, pa, pb))
    return cases


def key_range_ok(seqs, pa, pb, sc):
    amax = max(1, *(abs(x) for x in sc))
    return all((len(seqs[a]) + len(seqs[b]) + 2) * amax < (1 << 28) for a, b in zip(pa, pb))


@pytest.mark.gpu
def test_forced_stripe_route_matches_oracle():
    """Every eligible pair on the stripe engine (PWA_SCORES_ROUTE=1, two-value form forced for the short pairs) against
    the oracle, for every scoring of test_gpu_hw4 whose keys are in range."""
    with switched_context(PWA_SCORES_ROUTE="1", PWA_NO_PACKED_DIST="1") as c:
        for seqs, pa, pb in forced_cases():
            for sc in SCORINGS:
                b = c.batch_distances(seqs, pa, pb, *sc)
                kern = b.info()["kernel"]
                b.close()
                got = c.distances(seqs, pa, pb, *sc)
                want = [O.nw_distance(seqs[a], seqs[b2], *sc)[0] for a, b2 in zip(pa, pb)]
                bad = [k for k in range(len(pa)) if got[k] != want[k]]
                assert not bad, (sc, [(len(seqs[pa[k]]), len(seqs[pb[k]]), got[k], want[k]) for k in bad[:5]])
                # (100, -90, -70): match - gap leaves the byte table, the arena is not coded -> strips
                if sc == (100, -90, -70):
                    assert STRIPE not in kern, kern
                else:
                    assert key_range_ok(seqs, pa, pb, sc) and kern.startswith(STRIPE) and STRIP not in kern, (sc, kern)


@pytest.mark.gpu
def test_forced_route_without_packed_switch_and_ineligible_lists():
    """n + m > 4000 takes the two-value form by itself; PWA_SCORES_ROUTE=1 alone then moves it.  An alphabet of more than
    7 symbols and an out-of-range scoring stay on the strips, exact."""
    rng = random.Random(7)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (2500, 2400, 1700, 3000)]
    pa, pb = [0, 0, 1, 3, 2], [1, 3, 2, 3, 0]
    wide = [bytes(rng.choice(bytes(range(65, 91))) for _ in range(n)) for n in (2500, 2400, 1700)]
    with switched_context(PWA_SCORES_ROUTE="1") as c:
        for sc in [(1, -1, -1), (5, -4, -4), (100, -90, -70)]:
            b = c.batch_distances(seqs, pa, pb, *sc)
            kern = b.info()["kernel"]
            b.close()
            assert (STRIPE in kern) == (sc != (100, -90, -70)), (sc, kern)
            assert c.distances(seqs, pa, pb, *sc) == [O.nw_distance(seqs[a], seqs[b2], *sc)[0] for a, b2 in zip(pa, pb)], sc
        b = c.batch_distances(wide, [0, 1], [1, 2], 1, -1, -1)
        assert STRIPE not in b.info()["kernel"]
        b.close()
        assert c.distances(wide, [0, 1], [1, 2], 1, -1, -1) == [O.nw_distance(wide[a], wide[b2], 1, -1, -1)[0] for a, b2 in [(0, 1), (1, 2)]]


@pytest.mark.gpu
def test_split_batch_matches_oracle(ctx):
    """A few 10 kb pairs among many 300 bp pairs (the list is in the two-value form): the long pairs leave the strips, the
    short ones -- full wave tasks, where the strips are the cheaper engine per cell -- stay; both engines write into the one
    score vector in pair order."""
    rng = random.Random(99)
    longs = [bytes(rng.choice(b"ACGT") for _ in range(10000)) for _ in range(4)]
    texts = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(290, 310))) for _ in range(64)]
    pats = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(280, 320))) for _ in range(1200)]
    seqs = longs + texts + pats
    pa = [68 + p for t in range(64) for p in range(1200)]
    pb = [4 + t for t in range(64) for p in range(1200)]
    for at, (a, b) in zip((17, 40000, 40001, len(pa)), ((0, 1), (2, 3), (1, 2), (3, 0))):
        pa.insert(at, a)
        pb.insert(at, b)
    b = ctx.batch_distances(seqs, pa, pb, 1, -1, -1)
    kern = b.info()["kernel"]
    b.close()
    assert " + " in kern and kern.startswith(STRIP) and STRIPE in kern, kern
    got = ctx.distances(seqs, pa, pb, 1, -1, -1)
    want = [O.nw_distance(seqs[a], seqs[b2], 1, -1, -1)[0] for a, b2 in zip(pa, pb)]
    assert got == want
