"""Seeding read lists on the device against a kept text index (Context.index, TextIndex.seed, pwa_sa_seed), inside the
mapper it feeds (Context.map_reads), scoring (1, -4, -6, -1).

The lists of tools/chain_batch.py, drawn the same way from the same generator: reads of 1500 symbols cut out of a random 1 Mb text and
mutated at 8 % (substitutions, insertions and deletions in equal parts), k = 15, step 1, max_occ 64, the defaults of Context.chain,
w = 100.  Per list (4096 and 65 536 reads), in slices of --slice reads as chain_batch.py runs them, after one warm-up pass, medians over
--reps passes of the sums over the slices:
  - map_reads on the text's bytes (every call builds its own index): wall seconds of its three stages (seed_s holds the index build),
    device ms of the search kernel and of gather + sort + split (pwa_sa_seed_last_stats), slots, hits, ranges, the build's device ms;
  - map_reads on ONE TextIndex for all the slices: the same figures, and the one build's device ms and wall seconds;
  - TextIndex.seed alone on that index (as_arrays): wall seconds per list.
Lines go to profiles/seed_batch.jsonl.

    python tools/seed_batch.py [--reads 4096,65536] [--reps 3] [--slice 4096]
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
OUT = os.path.join(ROOT, "profiles", "seed_batch.jsonl")
SUMS = ("seed_s", "chain_s", "align_s", "search_ms", "sort_ms", "slots", "hits", "ranges", "build_ms")


def emit(row):
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def one_pass(ctx, text, reads, at, cut):
    """map_reads over the list in slices; text: bytes or a TextIndex -> the sums over the slices"""
    tot = dict.fromkeys(SUMS, 0.0)
    tot.update(placed=0, within_w=0)
    t0 = time.perf_counter()
    for s0 in range(0, len(reads), cut):
        got = ctx.map_reads(text, reads[s0:s0 + cut], K, *SC, w=W)
        for k in ("seed_s", "chain_s", "align_s"):
            tot[k] += ctx.map_stats[k]
        for k in ("search_ms", "sort_ms", "slots", "hits", "ranges"):
            tot[k] += ctx.seed_stats[k]
        if isinstance(text, bytes):
            tot["build_ms"] += ctx.sa_stats["build_ms"]
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
        cut = min(a.slice, n_reads)
        n_slices = (n_reads + cut - 1) // cut
        passes = [one_pass(ctx, text, reads, at, cut) for _ in range(a.reps + 1)][1:]
        emit(dict(what="map_reads, an index per call", reads=n_reads, slices=n_slices, reps=a.reps, **medians(passes)))
        t0 = time.perf_counter()
        with ctx.index(text) as ix:
            build_s = time.perf_counter() - t0
            passes = [one_pass(ctx, ix, reads, at, cut) for _ in range(a.reps + 1)][1:]
            emit(dict(what="map_reads, one TextIndex", reads=n_reads, slices=n_slices, reps=a.reps, index_build_ms=ix.stats["build_ms"],
                      index_build_s=build_s, **medians(passes)))
            wall = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                for s0 in range(0, n_reads, cut):
                    ix.seed(reads[s0:s0 + cut], K, as_arrays=True)
                wall.append(time.perf_counter() - t0)
            emit(dict(what="TextIndex.seed alone", reads=n_reads, slices=n_slices, reps=a.reps, seed_s=statistics.median(wall[1:])))
    ctx.close()


if __name__ == "__main__":
    main()
