"""Both-strand mapping from one canonical sketch per read (Context.index(text, minimizers=(k, w), canonical=True),
MinimizerIndex.seed_strands, pwa_mm_seed_strands) beside the plain MinimizerIndex of §3.27, which seeds the reads
and their reverse complements as 2 n unrelated reads, inside the mapper both feed (Context.map_reads(both_strands=True)), scoring
(1, -4, -6, -1).

The two lists of tools/minimizer_batch.py, drawn the same way from the same generator -- 4096 and 65 536 reads of 1500 symbols cut out
of a random 1 Mb text and mutated at 8 %, k = 15, max_occ 64, the defaults of Context.chain, placement window 100 -- with every other
read reverse-complemented.  Per list and per w in 5, 10, 19, one plain and one canonical index, each kept over all its passes, in the
same process: in slices of --slice reads, after one warm-up pass, medians over --reps passes of the sums over the slices:
  - the index: device ms of its build, its entries;
  - map_reads: wall seconds of its three stages and in all; the device ms of the sketch passes, of the lookup and of gather + sort +
    split; k-mers examined, read minimizers looked up, hits, ranges; the reads placed, and placed on the strand they were cut from
    within the window of where they were cut.
Lines go to profiles/canonical_batch.jsonl.

    python tools/canonical_batch.py [--reads 4096,65536] [--reps 3] [--slice 4096] [--w 5,10,19]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from banded_batch import gen_dna, mutate  # noqa: E402

SC = (1, -4, -6, -1)
K, W, LEN, RATE, TEXT = 15, 100, 1500, 0.08, 1000000
OUT = os.path.join(ROOT, "profiles", "canonical_batch.jsonl")
SEED_KEYS = ("sketch_ms", "search_ms", "sort_ms", "slots", "minimizers", "hits", "ranges")


def emit(row):
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def one_pass(ctx, index, reads, at, strand, cut):
    """map_reads(both_strands=True) over the list in slices on a kept index -> the sums over the slices"""
    tot = dict.fromkeys(("seed_s", "chain_s", "align_s") + SEED_KEYS, 0.0)
    tot.update(placed=0, right_strand_within_w=0)
    t0 = time.perf_counter()
    for s0 in range(0, len(reads), cut):
        got = ctx.map_reads(index, reads[s0:s0 + cut], K, *SC, w=W, both_strands=True)
        for k in ("seed_s", "chain_s", "align_s"):
            tot[k] += ctx.map_stats[k]
        for k in SEED_KEYS:
            tot[k] += ctx.seed_stats[k]
        tot["placed"] += sum(g is not None for g in got)
        tot["right_strand_within_w"] += sum(g is not None and g["strand"] == s and abs(g["pos"] - int(p)) <= W
                                            for g, p, s in zip(got, at[s0:s0 + cut], strand[s0:s0 + cut]))
    tot["total_s"] = time.perf_counter() - t0
    return tot


def medians(passes):
    return {k: statistics.median(p[k] for p in passes) for k in passes[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="4096,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice", type=int, default=4096)
    ap.add_argument("--w", default="5,10,19")
    a = ap.parse_args()
    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(7)
    text_arr = gen_dna(rng, TEXT)
    text = text_arr.tobytes()
    for n_reads in [int(x) for x in a.reads.split(",")]:
        at = rng.integers(0, TEXT - LEN, n_reads)
        reads = [mutate(rng, text_arr[p:p + LEN], RATE).tobytes() for p in at]
        reads = [pkg.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
        strand = ["+-"[i % 2] for i in range(n_reads)]
        cut = min(a.slice, n_reads)
        for w in (int(x) for x in a.w.split(",")):
            for canonical in (False, True):
                t0 = time.perf_counter()
                with ctx.index(text, minimizers=(K, w), canonical=canonical) as ix:
                    build_s = time.perf_counter() - t0
                    head = dict(index="canonical" if canonical else "plain", w=w, reads=n_reads, slices=(n_reads + cut - 1) // cut, reps=a.reps,
                                index_build_ms=ix.stats["build_ms"], index_build_s=build_s, index_entries=ix.stats["minimizers"])
                    passes = [one_pass(ctx, ix, reads, at, strand, cut) for _ in range(a.reps + 1)][1:]
                    emit(dict(head, what="map_reads(both_strands=True)", **medians(passes)))
    ctx.close()


if __name__ == "__main__":
    main()
