"""Minimizer seeding (Context.index(text, minimizers=(k, w)), MinimizerIndex.seed, pwa_mm_seed) beside the
suffix-array seeding of §3.25, inside the mapper both feed (Context.map_reads), scoring (1, -4, -6, -1).

The two lists of tools/seed_batch.py, drawn the same way from the same generator: 4096 and 65 536 reads of 1500 symbols cut out of a
random 1 Mb text and mutated at 8 %, k = 15, max_occ 64, the defaults of Context.chain, placement window 100.  Per list and per index
-- one TextIndex (step 1), then one MinimizerIndex at w = 5, 10 and 19 -- in slices of --slice reads, after one warm-up pass, medians
over --reps passes of the sums over the slices:
  - the index: device ms of its build, its entries (text positions for the suffix array);
  - map_reads: wall seconds of its three stages and in all, the device ms of the seeding stages, k-mers examined, read minimizers looked
    up, hits, ranges, the chain kernel's device ms, the reads placed and placed within the window of where they were cut;
  - map_reads(secondary=2): the device ms of the chain and of the top-N passes.
Lines go to profiles/minimizer_batch.jsonl.

    python tools/minimizer_batch.py [--reads 4096,65536] [--reps 3] [--slice 4096] [--w 5,10,19]
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
OUT = os.path.join(ROOT, "profiles", "minimizer_batch.jsonl")
SEED_KEYS = ("sketch_ms", "search_ms", "sort_ms", "slots", "minimizers", "hits", "ranges")


def emit(row):
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def one_pass(ctx, index, reads, at, cut, secondary):
    """map_reads over the list in slices on a kept index -> the sums over the slices"""
    tot = dict.fromkeys(("seed_s", "chain_s", "align_s", "chain_ms", "top_ms") + SEED_KEYS, 0.0)
    tot.update(placed=0, within_w=0)
    t0 = time.perf_counter()
    for s0 in range(0, len(reads), cut):
        got = ctx.map_reads(index, reads[s0:s0 + cut], K, *SC, w=W, secondary=secondary)
        for k in ("seed_s", "chain_s", "align_s"):
            tot[k] += ctx.map_stats[k]
        for k in SEED_KEYS:
            tot[k] += ctx.seed_stats.get(k, 0)   # (the suffix-array seeding has no sketch pass and looks up every k-mer)
        stats = ctx.chain_top_stats if secondary else ctx.chain_stats
        tot["chain_ms"] += stats["chain_ms"]
        tot["top_ms"] += stats.get("top_ms", 0.0)
        tot["placed"] += sum(g is not None for g in got)
        tot["within_w"] += sum(g is not None and abs(g["pos"] - int(p)) <= W for g, p in zip(got, at[s0:s0 + cut]))
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
    kinds = [("suffix array", None)] + [("minimizers w=%d" % w, (K, w)) for w in (int(x) for x in a.w.split(","))]
    for n_reads in [int(x) for x in a.reads.split(",")]:
        at = rng.integers(0, TEXT - LEN, n_reads)
        reads = [mutate(rng, text_arr[p:p + LEN], RATE).tobytes() for p in at]
        cut = min(a.slice, n_reads)
        for name, minimizers in kinds:
            t0 = time.perf_counter()
            with ctx.index(text, minimizers=minimizers) as ix:
                build_s = time.perf_counter() - t0
                head = dict(index=name, reads=n_reads, slices=(n_reads + cut - 1) // cut, reps=a.reps, index_build_ms=ix.stats["build_ms"],
                            index_build_s=build_s, index_entries=ix.stats.get("minimizers", len(text)))
                for secondary in (0, 2):
                    passes = [one_pass(ctx, ix, reads, at, cut, secondary) for _ in range(a.reps + 1)][1:]
                    emit(dict(head, what="map_reads" if not secondary else "map_reads(secondary=2)", **medians(passes)))
    ctx.close()


if __name__ == "__main__":
    main()
