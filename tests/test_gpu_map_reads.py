"""Context.seed and Context.map_reads on the GPU: the seeds against chain_oracle.py's seeder over a dict of k-mers, and seed -> chain ->
banded semi-global alignment end to end on planted reads: strand, position, the score against the unbanded semi-global score of the
same window, and the CIGAR re-scored."""
import random
import re

import pytest

import chain_oracle as CO
import gotoh_oracle as GO

pytestmark = pytest.mark.gpu

K, W = 13, 100
SC = (1, -4, -6, -1)   # match, mismatch, gap_open, gap_extend
_cache = {}


def planted():
    """a 30 kb text with a 400-base unit in five copies, and 64 reads of 300 .. 1500 symbols planted at 0, 5 and 10 % divergence, every
    other one on the reverse strand.  chain_oracle + banded_oracle + gotoh_oracle on the CPU say of every one of them: it has a chain,
    its band is valid, the banded and the unbanded semi-global score of its window agree, and it starts within W of where it was
    planted (checked when the reads were chosen; the GPU test asserts all of it again)"""
    if "planted" not in _cache:
        rng = random.Random(41)
        text = CO.random_text(rng, 30000, repeat=400, copies=5)
        reads = []
        for i in range(64):
            reads += CO.planted_reads(rng, text, 1, (300, 1500), (0.0, 0.05, 0.10)[i % 3], both_strands=False)
            if i % 2:
                r, at, _ = reads[-1]
                reads[-1] = (CO.revcomp(r), at, "-")
        _cache["planted"] = text, reads
    return _cache["planted"]


def cigar_score(cigar, read, window, j):
    """the affine score of a CIGAR ('M' read symbol against text symbol, 'D' read symbol against a gap, 'I' text symbol against a gap)
    from cell (0, j) of the window -> (score, end i, end j)"""
    match, mismatch, go, ge = SC
    i, s = 0, 0
    for cnt, op in re.findall(r"(\d+)([MID])", cigar.decode()):
        cnt = int(cnt)
        if op == "M":
            s += sum(match if read[i + x] == window[j + x] else mismatch for x in range(cnt))
            i += cnt
            j += cnt
        else:
            s += go + cnt * ge
            if op == "D":
                i += cnt
            else:
                j += cnt
    return s, i, j


def test_seed_matches_the_oracles_seeder(ctx):
    text, reads = planted()
    reads = [r for r, _, _ in reads[:12]] + [b"", b"ACGT", text[:K], text[7:7 + K - 1], text[-K:], text[0:400], text[100:900]]
    index = CO.kmer_index(text, K)
    unit = sorted(len(index[text[q:q + K]]) for q in range(400 - K + 1))
    assert unit[0] == 5 and unit[-1] == 6                      # the repeat's k-mers: five copies, and one that also occurs elsewhere
    for step, max_occ in [(1, 64), (1, 4), (3, 5), (1, 1), (K, 64)]:
        got = ctx.seed(text, reads, K, step=step, max_occ=max_occ)
        want = [CO.seed(index, r, K, step, max_occ) for r in reads]
        assert got == want, (step, max_occ)
        assert CO.validate(got) == (0, None)
        arrays = ctx.seed(text, reads, K, step=step, max_occ=max_occ, as_arrays=True)
        assert [[tuple(a) for a in arr.tolist()] for arr in arrays] == want
    biting = ctx.seed(text, [text[0:400]], K, max_occ=4)[0]    # the whole read is the repeat unit: every k-mer occurs five times or more
    assert biting == [] and len(ctx.seed(text, [text[0:400]], K, max_occ=5)[0]) == 5 * unit.count(5)
    assert ctx.seed(b"ACGT", [b"ACGTACGTACGTACGT"], K) == [[]] and ctx.seed(text, [], K) == []
    assert ctx.seed(b"GATTACAGATTACA", [b"TTACAG", b"TACA"], 4) == [[(2, 0, 4), (3, 1, 4), (4, 2, 4), (9, 0, 4), (10, 1, 4)], [(3, 0, 4), (10, 0, 4)]]


def test_map_reads_places_planted_reads(ctx, pkg):
    text, planted_reads = planted()
    reads = [r for r, _, _ in planted_reads]
    got = ctx.map_reads(text, reads, K, *SC, w=W, both_strands=True)
    assert len(got) == len(reads) and all(g is not None for g in got)
    assert set(ctx.map_stats) == {"seed_s", "chain_s", "align_s"}
    pats, wins, short = [], [], []
    fws = [read if strand == "+" else pkg.revcomp(read) for read, _, strand in planted_reads]   # as the text has them
    chains = ctx.chain(ctx.seed(text, fws, K))
    for k, ((read, at, strand), g, fw, c) in enumerate(zip(planted_reads, got, fws, chains)):
        assert g["strand"] == strand, k
        assert abs(g["pos"] - at) <= W, (k, g["pos"], at)
        assert c["score"] == g["chain_score"]
        # the window map_reads aligned in, from the chain of the same seeds
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
    assert [got[k]["score"] for k in short] == list(full)
    assert len(short) > 20 and len(short) < 60
    one_strand = ctx.map_reads(text, reads, K, *SC, w=W)
    for (read, at, strand), g, h in zip(planted_reads, got, one_strand):
        if strand == "+":
            assert h == g
        else:
            assert h is None or h["chain_score"] < g["chain_score"]


def test_unmappable_reads_come_back_none(ctx):
    text, planted_reads = planted()
    rng = random.Random(2)
    noise = bytes(rng.randrange(256) for _ in range(700))
    repeat_only = text[0:400]                      # every k-mer of it occurs five times
    good = planted_reads[0][0]
    got = ctx.map_reads(text, [noise, good, repeat_only, b"", b"ACG"], K, *SC, w=W, max_occ=4, both_strands=True)
    assert [g is None for g in got] == [True, False, True, True, True]
    assert ctx.map_reads(text, [repeat_only], K, *SC, w=W, max_occ=5)[0] is not None
    assert ctx.map_reads(text, [], K, *SC) == []
    # a chain whose diagonals spread wider than the banded call's 4096: two halves of a read planted 6000 apart
    split = text[2000:2400 + 200] + text[9000:9600]
    assert ctx.map_reads(text, [split], K, *SC, w=W, max_dist=8000, bandwidth=7000, gap_scale=0)[0] is None
