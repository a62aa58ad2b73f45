"""Context.map_reads over a canonical MinimizerIndex on the GPU: the planted reads of test_gpu_map_reads.py placed from one sketch of
each read as given (K = 13, w = 10) -- strand, position, the score against the unbanded semi-global score of the window, the CIGAR
re-scored -- the both-strand text of test_gpu_map_secondary.py with a primary on one strand and a secondary on the other, the
forward half alone without both_strands, and the refusals."""
import pytest

import canonical_oracle as KO
import chain_oracle as CO
import gotoh_oracle as GO
from test_gpu_map_reads import K, SC, W, cigar_score, planted
from test_gpu_map_secondary import check_alignments, three_copies

pytestmark = pytest.mark.gpu

WIN = 10


def test_map_reads_places_planted_reads_from_one_sketch_each(ctx, pkg):
    text, planted_reads = planted()
    reads = [r for r, _, _ in planted_reads]
    n = len(reads)
    want, looked = KO.seed(text, reads, K, WIN)
    with ctx.index(text, minimizers=(K, WIN), canonical=True) as ix:
        got = ctx.map_reads(ix, reads, K, *SC, w=W, both_strands=True)
        assert set(ctx.map_stats) == {"seed_s", "chain_s", "align_s"}
        assert ix.seed_stats["minimizers"] == looked and ix.seed_stats["hits"] == sum(len(lst) for lst in want) < 10000
        assert ix.seed_stats["slots"] == sum(len(r) - K + 1 for r in reads)        # the n reads as given, no reverse complement among them
        assert len(got) == n and all(g is not None for g in got)
        anchors = ix.seed_strands(reads)
        assert anchors == KO.by_strand(want)
        chains = ctx.chain(anchors)
        pats, wins, short = [], [], []
        for k, ((read, at, strand), g) in enumerate(zip(planted_reads, got)):
            s = "+-".index(strand)
            fw = read if s == 0 else pkg.revcomp(read)                                # as the text has it
            c = chains[s * n + k]
            assert g["strand"] == strand and c["score"] > chains[(1 - s) * n + k]["score"], k
            assert abs(g["pos"] - at) <= W, (k, g["pos"], at)
            assert c["score"] == g["chain_score"]
            ws, we, lo, hi = CO.window_and_band(c, len(fw), len(text), W)
            assert ws <= g["pos"] <= g["end"] <= we
            sc, i, j = cigar_score(g["cigar"], fw, text[ws:we], g["pos"] - ws)
            assert (sc, i, j) == (g["score"], len(fw), g["end"] - ws), k
            if len(fw) <= 1024:
                short.append(k)
                pats.append(fw)
                wins.append(text[ws:we])
            else:   # beyond scores_gotoh's pattern length: the oracle that call is tested against
                assert g["score"] == GO.align(fw, text[ws:we], "sg", SC[:2], SC[2], SC[3], want_ops=False)["score"], k
        full = ctx.scores_gotoh("sg", pats + wins, list(range(len(pats))), list(range(len(pats), 2 * len(pats))), *SC)
        assert [got[k]["score"] for k in short] == list(full) and len(short) > 20
        # both_strands=False: the forward half only -- the '+' reads as above, the '-' reads as their forward lists have them
        half = ctx.map_reads(ix, reads, K, *SC, w=W)
        assert ix.seed_stats["minimizers"] == looked
        for k, ((_, _, strand), g, h) in enumerate(zip(planted_reads, got, half)):
            assert (h == g) if strand == "+" else (h is None or (h["strand"] == "+" and h["chain_score"] == chains[k]["score"] < g["chain_score"])), k
        assert sum(1 for h in half if h is not None) >= n // 2
        for bad in (dict(k=K + 1), dict(k=K - 1), dict(k=K, step=2)):
            for secondary in (0, 2):
                with pytest.raises(ValueError):
                    ctx.map_reads(ix, reads[:2], bad["k"], *SC, w=W, step=bad.get("step", 1), secondary=secondary)
        for call in (lambda: ctx.seed(ix, reads[:2], K), lambda: ix.seed(reads[:2])):
            with pytest.raises(ValueError):
                call()


def test_the_both_strand_text_gives_a_primary_on_one_strand_and_a_secondary_on_the_other(ctx, pkg):
    _, unit, _, both = three_copies()
    reads = [unit, CO.revcomp(unit)]
    with ctx.index(both, minimizers=(12, 5), canonical=True) as ix:
        got = ctx.map_reads(ix, reads, 12, *SC, w=W, both_strands=True, secondary=2)
        assert set(ctx.map_stats) == {"seed_s", "chain_s", "align_s"}
        anchors = ix.seed_strands(reads)
        assert anchors == KO.by_strand(KO.seed(both, reads, 12, 5)[0])
        tops = ctx.chain_top(anchors, 3, 40, 3, rooted=True)
        forward_only = ctx.map_reads(ix, reads, 12, *SC, w=W, secondary=2)
    assert [c["score"] for c in tops[0]["chains"]] == [595] and [c["score"] for c in tops[2]["chains"]] == [531]
    for k, (read, g) in enumerate(zip(reads, got)):
        first, second = ("+", "-") if k == 0 else ("-", "+")       # the exact copy is forward at 2000, the 2 % copy reverse at 12000
        assert g["strand"] == first and [x["strand"] for x in g["secondary"]] == [second]
        assert abs(g["pos"] - 2000) <= W and abs(g["secondary"][0]["pos"] - 12000) <= W
        assert g["chain_score"] > g["secondary"][0]["chain_score"]
        mine = {s: tops[s * 2 + k]["chains"] for s in (0, 1)}
        assert len(mine[0]) == len(mine[1]) == 1
        assert g["mapq"] == pkg.mapq(g["chain_score"], g["secondary"][0]["chain_score"], mine["+-".index(first)][0]["count"])
        check_alignments(ctx, both, read, [(g, mine["+-".index(first)][0]), (g["secondary"][0], mine["+-".index(second)][0])])
        # without both_strands: the forward placement only
        f = forward_only[k]
        assert f["strand"] == "+" and f["secondary"] == [] and abs(f["pos"] - (2000 if k == 0 else 12000)) <= W
        assert f["chain_score"] == mine[0][0]["score"]
