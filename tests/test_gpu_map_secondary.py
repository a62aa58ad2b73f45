"""Context.map_reads(secondary=S) on the GPU: the primary against map_reads(secondary=0) on the planted reads of test_gpu_map_reads.py,
mapq 60 for the reads that touch no repeat, and on a text with a unit in three copies the primary at the best copy, the secondaries
at the other two, every alignment's score against the unbanded semi-global score of its window, its CIGAR re-scored, and mapq against
mapq() of the two chain scores."""
import random

import pytest

import chain_oracle as CO
import chain_top_oracle as TO
from test_gpu_map_reads import K, SC, W, cigar_score, planted

pytestmark = pytest.mark.gpu

TODAY = ("pos", "end", "score", "cigar", "mdz", "strand", "chain_score")
_cache = {}


def test_the_primary_is_the_placement_without_secondaries(ctx):
    text, planted_reads = planted()
    reads = [r for r, _, _ in planted_reads]
    plain = ctx.map_reads(text, reads, K, *SC, w=W, both_strands=True)
    assert all(set(p) == set(TODAY) for p in plain)                     # secondary = 0: no new keys
    assert ctx.map_reads(text, reads, K, *SC, w=W, both_strands=True, secondary=0, min_chain_score=1, min_chain_count=1) == plain
    got = ctx.map_reads(text, reads, K, *SC, w=W, both_strands=True, secondary=2, min_chain_score=1, min_chain_count=1)
    assert set(ctx.map_stats) == {"seed_s", "chain_s", "align_s"}
    for k, (g, p) in enumerate(zip(got, plain)):
        assert set(g) == set(TODAY) | {"mapq", "secondary"}, k
        assert {key: g[key] for key in TODAY} == p, k
        assert len(g["secondary"]) <= 2 and all(set(s) == set(TODAY) for s in g["secondary"])
        assert all(s["chain_score"] <= g["chain_score"] for s in g["secondary"])
    # under the default thresholds a read that touches no copy of the 400-base unit is unique: mapq 60 and no secondary
    got = ctx.map_reads(text, reads, K, *SC, w=W, both_strands=True, secondary=2)
    copies = [c * (len(text) - 400) // 4 for c in range(5)]
    unique = [k for k, (r, at, _) in enumerate(planted_reads) if not any(at < c + 400 and c < at + len(r) for c in copies)]
    assert len(unique) > 50
    for k in unique:
        assert got[k]["mapq"] == 60 and got[k]["secondary"] == [], k
        assert {key: got[k][key] for key in TODAY} == plain[k]
    assert any(g["secondary"] for g in got) and any(g["mapq"] < 60 for g in got)
    with pytest.raises(ValueError):
        ctx.map_reads(text, reads[:1], K, *SC, secondary=16)


def three_copies():
    """a 30 kb text with a 600-base unit at 3000 (2 % substitutions), at 12000 (as it is) and at 24000 (5 %), and a second text with the
    unit at 2000 and the reverse complement of its 2 % copy at 12000"""
    if "copies" not in _cache:
        rng = random.Random(78)
        unit = bytes(rng.choice(b"ACGT") for _ in range(600))

        def copy(rate):
            c = bytearray(unit)
            for i in rng.sample(range(600), int(600 * rate)):
                c[i] = rng.choice([b for b in b"ACGT" if b != c[i]])
            return bytes(c)
        text = bytearray(CO.random_text(rng, 30000))
        loci = (12000, 3000, 24000)   # best copy first
        for at, rate in zip(loci, (0.0, 0.02, 0.05)):
            text[at:at + 600] = copy(rate)
        both = bytearray(CO.random_text(rng, 20000))
        both[2000:2600] = unit
        both[12000:12600] = CO.revcomp(copy(0.02))
        _cache["copies"] = bytes(text), unit, loci, bytes(both)
    return _cache["copies"]


def check_alignments(ctx, text, fw, placements):
    """every placement of read fw (as given) -> its score is the unbanded semi-global score of its window and its CIGAR re-scores to it"""
    pats, wins = [], []
    for g, c in placements:
        read = fw if g["strand"] == "+" else CO.revcomp(fw)
        ws, we, lo, hi = CO.window_and_band(c, len(read), len(text), W)
        assert ws <= g["pos"] <= g["end"] <= we and g["chain_score"] == c["score"]
        assert cigar_score(g["cigar"], read, text[ws:we], g["pos"] - ws) == (g["score"], len(read), g["end"] - ws)
        pats.append(read)
        wins.append(text[ws:we])
    n = len(pats)
    assert [g["score"] for g, _ in placements] == list(ctx.scores_gotoh("sg", pats + wins, list(range(n)), list(range(n, 2 * n)), *SC))


def test_three_copies_give_a_primary_and_two_secondaries(ctx, pkg):
    text, unit, loci, _ = three_copies()
    rng = random.Random(5)
    reads = [unit, CO.revcomp(unit), CO.mutate(rng, unit, 0.03), CO.revcomp(CO.mutate(rng, unit, 0.03)), text[11900:12500]]
    got = ctx.map_reads(text, reads, 12, *SC, w=W, both_strands=True, secondary=2)
    strands = [reads, [CO.revcomp(r) for r in reads]]
    tops = ctx.chain_top(ctx.seed(text, strands[0] + strands[1], 12), 3, 40, 3, rooted=True)
    for k, (read, g) in enumerate(zip(reads, got)):
        strand = "+-"[k % 2] if k < 4 else "+"
        s = "+-".index(strand)
        chains = tops[s * len(reads) + k]["chains"]
        assert len(chains) == 3 and tops[(1 - s) * len(reads) + k]["chains"] == [], k
        assert g["strand"] == strand and [x["strand"] for x in g["secondary"]] == [strand] * 2
        shift = 100 if k == 4 else 0                 # the last read starts 100 before the unit
        for x, at in zip([g] + g["secondary"], loci):
            assert abs(x["pos"] - (at - shift)) <= W, (k, x["pos"], at)
        assert g["chain_score"] > g["secondary"][0]["chain_score"] >= g["secondary"][1]["chain_score"]
        assert g["mapq"] == pkg.mapq(g["chain_score"], g["secondary"][0]["chain_score"], chains[0]["count"])
        assert g["mapq"] == TO.mapq(chains[0]["score"], chains[1]["score"], chains[0]["count"]) < 60
        check_alignments(ctx, text, read, list(zip([g] + g["secondary"], chains)))
    one = ctx.map_reads(text, reads[:1], 12, *SC, w=W, secondary=1)[0]
    assert len(one["secondary"]) == 1 and {k: one[k] for k in TODAY} == {k: got[0][k] for k in TODAY} and one["mapq"] == got[0]["mapq"]
    assert one["secondary"][0] == got[0]["secondary"][0]


def test_a_forward_and_a_reverse_copy_return_both_strands(ctx, pkg):
    _, unit, _, both = three_copies()
    for read, first in ((unit, "+"), (CO.revcomp(unit), "-")):
        g = ctx.map_reads(both, [read], 12, *SC, w=W, both_strands=True, secondary=2)[0]
        other = "-" if first == "+" else "+"
        assert (g["strand"], [x["strand"] for x in g["secondary"]]) == (first, [other])
        assert abs(g["pos"] - 2000) <= W and abs(g["secondary"][0]["pos"] - 12000) <= W
        assert g["score"] == 600 and g["chain_score"] == 600 > g["secondary"][0]["chain_score"] > 400
        assert 0 < g["mapq"] == pkg.mapq(600, g["secondary"][0]["chain_score"], 10) < 10
        tops = ctx.chain_top(ctx.seed(both, [read, CO.revcomp(read)], 12), 3, 40, 3, rooted=True)
        check_alignments(ctx, both, read, [(g, tops["+-".index(first)]["chains"][0]), (g["secondary"][0], tops["+-".index(other)]["chains"][0])])
        h = ctx.map_reads(both, [read], 12, *SC, w=W, secondary=2)[0]   # the forward strand alone: one copy each, and so unique
        assert h == (dict(g, secondary=[], mapq=60) if first == "+" else dict(g["secondary"][0], secondary=[], mapq=60))
