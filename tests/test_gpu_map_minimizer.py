"""Context.map_reads over a MinimizerIndex on the GPU: the planted reads of test_gpu_map_reads.py placed from a tenth of the anchors
(K = 13, w = 10) -- strand, position, the score against the unbanded semi-global score of the window, the CIGAR re-scored -- and the
three-copy text of test_gpu_map_secondary.py with a primary and two secondaries; a wrong k or step is refused."""
import pytest

import chain_oracle as CO
import gotoh_oracle as GO
import minimizer_oracle as MO
from test_gpu_map_reads import K, SC, W, cigar_score, planted
from test_gpu_map_secondary import check_alignments, three_copies

pytestmark = pytest.mark.gpu

WIN = 10


def test_map_reads_places_planted_reads_from_minimizers(ctx, pkg):
    text, planted_reads = planted()
    reads = [r for r, _, _ in planted_reads]
    with ctx.index(text, minimizers=(K, WIN)) as ix:
        got = ctx.map_reads(ix, reads, K, *SC, w=W, both_strands=True)
        assert set(ctx.map_stats) == {"seed_s", "chain_s", "align_s"}
        assert ix.seed_stats["minimizers"] < ix.seed_stats["slots"] // 4 and ix.seed_stats["hits"] < 10000
        assert len(got) == len(reads) and all(g is not None for g in got)
        fws = [read if strand == "+" else pkg.revcomp(read) for read, _, strand in planted_reads]   # as the text has them
        anchors = ctx.seed(ix, fws, K)
        assert anchors == MO.seed(text, fws, K, WIN)[0]
        chains = ctx.chain(anchors)
        pats, wins, short = [], [], []
        for k, ((read, at, strand), g, fw, c) in enumerate(zip(planted_reads, got, fws, chains)):
            assert g["strand"] == strand, k
            assert abs(g["pos"] - at) <= W, (k, g["pos"], at)
            assert c["score"] == g["chain_score"]
            ws, we, lo, hi = CO.window_and_band(c, len(fw), len(text), W)
            assert ws <= g["pos"] <= g["end"] <= we
            s, i, j = cigar_score(g["cigar"], fw, text[ws:we], g["pos"] - ws)
            assert (s, i, j) == (g["score"], len(fw), g["end"] - ws), k
            if len(fw) <= 1024:
                short.append(k)
                pats.append(fw)
                wins.append(text[ws:we])
            else:   # beyond scores_gotoh's pattern length: the oracle that call is tested against
                assert g["score"] == GO.align(fw, text[ws:we], "sg", SC[:2], SC[2], SC[3], want_ops=False)["score"], k
        full = ctx.scores_gotoh("sg", pats + wins, list(range(len(pats))), list(range(len(pats), 2 * len(pats))), *SC)
        assert [got[k]["score"] for k in short] == list(full) and len(short) > 20
        for bad in (dict(k=K + 1), dict(k=K - 1), dict(k=K, step=2)):
            for secondary in (0, 2):
                with pytest.raises(ValueError):
                    ctx.map_reads(ix, reads[:2], bad["k"], *SC, w=W, step=bad.get("step", 1), secondary=secondary)
            with pytest.raises(ValueError):
                ctx.seed(ix, reads[:2], bad["k"], step=bad.get("step", 1))


def test_three_copies_give_a_primary_and_two_secondaries_from_minimizers(ctx, pkg):
    text, unit, loci, _ = three_copies()
    reads = [unit, CO.revcomp(unit), text[11900:12500]]
    with ctx.index(text, minimizers=(12, 5)) as ix:
        got = ctx.map_reads(ix, reads, 12, *SC, w=W, both_strands=True, secondary=2)
        assert set(ctx.map_stats) == {"seed_s", "chain_s", "align_s"}
        strands = [reads, [CO.revcomp(r) for r in reads]]
        tops = ctx.chain_top(ctx.seed(ix, strands[0] + strands[1], 12), 3, 40, 3, rooted=True)
    for k, (read, g) in enumerate(zip(reads, got)):
        strand = "+-+"[k]
        s = "+-".index(strand)
        chains = tops[s * len(reads) + k]["chains"]
        assert len(chains) == 3, k
        assert g["strand"] == strand and [x["strand"] for x in g["secondary"]] == [strand] * 2
        shift = 100 if k == 2 else 0                 # the last read starts 100 before the unit
        assert sorted(min(abs(x["pos"] - (at - shift)) for at in loci) <= W for x in [g] + g["secondary"]) == [True] * 3
        assert abs(g["pos"] - (loci[0] - shift)) <= W                                 # the exact copy is the primary
        assert {min(loci, key=lambda at: abs(x["pos"] - (at - shift))) for x in [g] + g["secondary"]} == set(loci)
        assert g["chain_score"] > g["secondary"][0]["chain_score"] >= g["secondary"][1]["chain_score"]
        assert g["mapq"] == pkg.mapq(g["chain_score"], g["secondary"][0]["chain_score"], chains[0]["count"]) < 60
        check_alignments(ctx, text, read, list(zip([g] + g["secondary"], chains)))
