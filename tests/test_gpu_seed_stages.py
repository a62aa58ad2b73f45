"""The stages behind the minimizer sketch on the GPU, on the inputs of seed_stage_cases.py: the hash lookup with its max_occ probe, the
scan of the hit counts, the two gathers, the sort, the list cuts taken from the sorted keys, and the split that turns the reverse
lists' tied runs round -- every result whole against the oracles (the lists, chain_oracle.validate, chain()'s acceptance, the
byte-for-byte meaning of every anchor, the stats), and beside each comparison the shape its builder promises: the run lengths and
where the runs lie among the sorted keys, the probe index relative to the index's size, the exact counts of minimizers, hits and
entries on 255 .. 257 and 4095 .. 4097, the pattern of empty lists, and q' at both ends of a read."""
import numpy as np
import pytest

import canonical_oracle as KO
import chain_oracle as CO
import minimizer_oracle as MO
import seed_stage_cases as SC
import test_gpu_canonical as GC
import test_gpu_minimizer as GM
import test_gpu_seed as GS
from conftest import switched_context

pytestmark = pytest.mark.gpu

EDGES = [255, 256, 257, 4095, 4096, 4097]


def check_plain(ctx, ix, reads, max_occ=64, entries=None, budget=0):
    """test_gpu_minimizer.check_seed, and what test_gpu_canonical.check_seed adds to it: every anchor's bytes and chain()'s verdict"""
    got = GM.check_seed(ix, reads, max_occ, entries, budget)
    for r, lst in zip(reads, got):
        assert all(ix.text[t:t + ln] == r[q:q + ln] for t, q, ln in lst)
    assert len(ctx.chain(got)) == len(reads)
    return got


def check(ctx, ix, reads, max_occ=64, entries=None, budget=0):
    """either index kind against its oracle -> the lists in the call's order"""
    if ix.canonical:
        return GC.check_seed(ctx, ix, reads, max_occ, entries, budget)
    return check_plain(ctx, ix, reads, max_occ, entries, budget)


def check_entries(ix, want):
    if ix.canonical:
        return GC.check_entries(ix, want)
    h, p = ix.entries()
    assert list(zip(h.tolist(), p.tolist())) == want and ix.stats["minimizers"] == len(want)


def alone_calls(case, run, per):
    """the calls that put a run on key 0 and on key total - 1: the longest read alone, the read of one unit alone (total = 2), and a
    single hit (total = 1: the sort runs no pass).  run(reads) -> the lists, stats; per: lists per read"""
    big, one = case["runs"].index(4097), case["runs"].index(1)
    lists, st = run([case["reads"][big]])
    assert lists == case["lists"][per * big:per * big + per] and st["hits"] == 2 * 4097
    tied = [(s, e) for i, _, s, e in SC.runs_of(lists) if per == 1 or i % 2]
    assert all(e - s == 4097 for s, e in tied) and tied[-1][1] == st["hits"]          # the last run ends on key total - 1
    assert tied[0][0] == (4097 if per == 2 and lists[0] else 0)                        # ... and the first starts on key 0, but for "both"
    lists, st = run([case["reads"][one]])
    assert lists == case["lists"][per * one:per * one + per] and st["hits"] == 2
    read, t = SC.single_hit_read(case, per == 2)
    lists, st = run([read])
    assert lists == ([[], [(t, 1, SC.K)]] if per == 2 else [[(t, 1, SC.K)]]) and st["hits"] == 1


def run_tied_strands(c, variant, w, arrays):
    case = SC.tied_runs(variant)
    with c.index(case["text"], minimizers=(SC.K, w), canonical=True) as ix:
        want = GC.check_seed(c, ix, case["reads"])
        assert want == case["lists"] and ix.seed_stats["hits"] == 29642 and ix.seed_stats["minimizers"] == sum(SC.RUNS)
        lengths = sorted(e - s for i, _, s, e in SC.runs_of(want) if i % 2)
        assert lengths == sorted(SC.RUNS * (1 if variant == "both" else 2))
        if arrays:
            got = ix.seed_strands(case["reads"], as_arrays=True)
            assert all(a.dtype == np.uint32 and a.shape == (len(x), 3) for a, x in zip(got, KO.by_strand(want)))
            assert [[tuple(x) for x in a.tolist()] for a in got] == KO.by_strand(want)
            assert len(c.chain(got)) == 2 * len(case["reads"])

        def run(reads):
            return GC.check_seed(c, ix, reads), ix.seed_stats
        alone_calls(case, run, 2)


@pytest.mark.parametrize("w", [1, 8])
@pytest.mark.parametrize("variant", ["reverse", "swapped", "both"])
def test_tied_runs_of_every_length_are_turned_round(ctx, variant, w):
    if variant == "both":
        assert SC.four_pairings(SC.tied_runs(variant)) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    run_tied_strands(ctx, variant, w, arrays=w == 8)


def test_tied_runs_on_a_poisoned_context():
    with switched_context(PWA_POISON="0xA5") as c:
        run_tied_strands(c, "reverse", 8, arrays=False)
        run_tied_strands(c, "both", 1, arrays=True)
        assert c.poison_stats()["buffers"] > 0


@pytest.mark.parametrize("w", [1, 8])
def test_tied_runs_keep_their_q_order_on_a_plain_index(ctx, w):
    case = SC.tied_runs("forward")
    with ctx.index(case["text"], minimizers=(SC.K, w)) as ix:
        got = check_plain(ctx, ix, case["reads"])
        assert got == case["lists"] and ix.seed_stats["hits"] == 29642
        assert sorted(e - s for _, _, s, e in SC.runs_of(got)) == sorted(SC.RUNS * 2)
        alone_calls(case, lambda reads: (check_plain(ctx, ix, reads), ix.seed_stats), 1)


def test_tied_runs_keep_their_q_order_on_the_suffix_array(ctx):
    case = SC.tied_runs("forward", sep=b"R")
    with ctx.index(case["text"]) as ix:
        got = GS.check(ix, case["reads"], SC.K)
        assert got == case["lists"] and ix.seed_stats["hits"] == 29642
        assert len(ctx.chain(got)) == len(case["reads"])
        alone_calls(case, lambda reads: (GS.check(ix, reads, SC.K), ix.seed_stats), 1)


@pytest.mark.parametrize("canonical", [False, True])
def test_the_max_occ_probe_inside_the_index_on_its_end_and_past_it(ctx, canonical):
    p = SC.probe_cases(canonical)
    c, n = p["c"], len(p["reads"])
    with ctx.index(p["text"], minimizers=(p["k"], 1), canonical=canonical) as ix:
        check_entries(ix, p["entries"])
        n_min = ix.stats["minimizers"]
        hashes = [e[0] for e in p["entries"]]
        top, bottom = p["names"].index("top"), p["names"].index("bottom")
        lo = hashes.index(hashes[-1])                   # of the top k-mer; the bottom k-mer's is 0, "above" is looked up at lo = n_min
        assert lo == n_min - c and hashes.count(hashes[0]) == c
        for m in p["max_occs"]:
            lists = check(ctx, ix, p["reads"], m, p["entries"])
            sizes = [len(lists[2 * i]) + len(lists[2 * i + 1]) for i in range(n)] if canonical else [len(a) for a in lists]
            assert sizes == p["hits"][m], m
            assert ix.seed_stats["minimizers"] == n and ix.seed_stats["hits"] == sum(p["hits"][m])
            # the probe lo + max_occ against n_min: below it the top k-mer is dropped, on it and past it kept
            assert (lo + m < n_min) == (sizes[top] == 0) and (m < c) == (sizes[bottom] == 0)
            if canonical and sizes[top]:
                assert lists[2 * top] and lists[2 * top + 1]         # its count is over both strands
        assert [lo + m - n_min for m in p["max_occs"][:3]] == [-1, 0, 1]
        # every read alone at max_occ = c: each a lookup of one lane
        for i, r in enumerate(p["reads"]):
            lists = check(ctx, ix, [r], c, p["entries"])
            assert sum(len(a) for a in lists) == p["hits"][c][i]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("target", EDGES)
def test_minimizers_hits_and_entries_on_block_and_tile_edges(ctx, target, canonical):
    e, text, entries = SC.edge_counts(target, canonical), SC.edge_text(), SC.edge_entries(canonical)
    with ctx.index(text, minimizers=(e["k"], 1), canonical=canonical) as ix:
        check_entries(ix, entries)
        for reads in ([e["one"]], e["spread"]):            # the minimizers looked up: lookup_kernel's blocks, the scan over nm + 1
            check(ctx, ix, reads, entries=entries)
            assert ix.seed_stats["minimizers"] == target == ix.seed_stats["slots"]
        lists = check(ctx, ix, [e["walk"]], e["walk_occ"], entries)      # the hits: the gathers' and the splits' blocks, the sort's tiles
        assert ix.seed_stats["hits"] == target == sum(len(a) for a in lists) and all(lists)
    with ctx.index(e["small"], minimizers=(e["k"], 1), canonical=canonical) as ix:   # the entries: the sort of the build
        want = (KO.index if canonical else MO.index)(e["small"], e["k"], 1)
        check_entries(ix, want)
        assert ix.stats["minimizers"] == target == len(want)
        lists = check(ctx, ix, [e["small"][5:70], CO.revcomp(e["small"][-80:]), e["small"][-e["k"]:]], entries=want)
        assert (lists[0] and lists[3] and lists[4]) if canonical else (lists[0] and lists[2])


def run_list_shapes(c, canonical, n, budget):
    case = SC.list_shapes(canonical, n)
    k, w = case["k"], case["w"]
    entries = (KO.index if canonical else MO.index)(case["text"], k, w)
    with c.index(case["text"], minimizers=(k, w), canonical=canonical) as ix:
        check_entries(ix, entries)
        for name, (reads, kinds) in case["shapes"].items():
            assert len(reads) == n
            lists = check(c, ix, reads, entries=entries, budget=budget)
            assert len(lists) == (2 * n if canonical else n)
            assert [bool(a) for a in lists] == SC.filled(kinds, canonical), name
            ends = SC.end_anchors(case, reads, kinds)
            assert all(lists[i] == a for i, a in ends.items()), name
            assert name not in ("ends_empty", "reverse_only") or len(ends) > n // 8
            if budget == 1:
                assert ix.seed_stats["ranges"] == sum(1 for r in reads if len(r) >= k)      # every read with a k-mer runs alone
        if canonical:
            first, last = (case["shapes"][name] for name in ("first", "last"))
            assert SC.filled(first[1], True) == [True] + [False] * (2 * n - 1) and SC.filled(last[1], True) == [False] * (2 * n - 1) + [True]
        assert {a[0][1] for a in ends.values() if a} == {0, 31}           # q' (plain: q) = 0 and = L - k, of reads of 46 symbols


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("n", [127, 128, 255, 256])
def test_degenerate_lists_and_the_mirror_at_both_ends(ctx, n, canonical):
    run_list_shapes(ctx, canonical, n, 0)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("n", [127, 128, 255, 256])
def test_degenerate_lists_with_every_read_a_range_of_its_own(n, canonical):
    with switched_context(PWA_OCC_CHUNK_HITS=1) as c:
        run_list_shapes(c, canonical, n, 1)
