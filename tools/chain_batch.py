"""Seed -> chain -> align on planted reads (Context.map_reads, pwa_chain_anchors), scoring (1, -4, -6, -1).

Reads of 1500 symbols cut out of a random 1 Mb text and mutated at 8 % (substitutions, insertions and deletions in equal parts), k = 15,
the defaults of Context.chain (lookback 64, max_dist 5000, bandwidth 500, gap_scale 38), w = 100.  Per list (4096 and 65 536 reads):
  - one chain call on the whole list's seeds: device ms of the chain kernel (pwa_chain_last_stats), anchors, anchors per second, the whole
    call's wall ms; medians over --reps repetitions after one warm-up call;
  - map_reads: wall seconds of its three stages (seed, chain, align), reads placed, reads whose start lies within w of the planted one.
    A list larger than --slice reads goes through map_reads in slices of that many (every call builds its own suffix-array index; the
    seeds of one call are held in host arrays), and the stage times are the sums over the slices;
  - on the first --wfa reads: device ms of scores_wfa_sg of each read against the WHOLE text, the way to place a read without a chain.
Lines go to profiles/chain_batch.jsonl.

    python tools/chain_batch.py [--reads 4096,65536] [--reps 3] [--slice 4096] [--wfa 16]
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
from banded_batch import gen_dna, mutate, stat  # noqa: E402

SC = (1, -4, -6, -1)
K, W, LEN, RATE, TEXT = 15, 100, 1500, 0.08, 1000000
OUT = os.path.join(ROOT, "profiles", "chain_batch.jsonl")


def emit(row):
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="4096,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice", type=int, default=4096)
    ap.add_argument("--wfa", type=int, default=16)
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
        # the chain call alone, on the seeds of the whole list (seeded slice by slice: the k-mers of one seed call are host arrays)
        anchors = []
        for s0 in range(0, n_reads, cut):
            anchors += ctx.seed(text, reads[s0:s0 + cut], K, as_arrays=True)
        wall, dev = [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            ctx.chain(anchors)
            t1 = time.perf_counter()
            if r:
                wall.append((t1 - t0) * 1e3)
                dev.append(ctx.chain_stats["chain_ms"])
        st = ctx.chain_stats
        ms = statistics.median(dev)
        emit(dict(what="chain", reads=n_reads, anchors=st["anchors"], ranges=st["ranges"], chain_ms=stat(dev), call_ms=stat(wall),
                  anchors_per_s=st["anchors"] / (ms * 1e-3), anchors_per_read=st["anchors"] / n_reads))
        del anchors
        # the whole mapper
        stages = dict(seed_s=0.0, chain_s=0.0, align_s=0.0)
        placed = near = 0
        chain_ms, n_anchors, fill_ms, walk_ms = 0.0, 0, 0.0, 0.0
        t0 = time.perf_counter()
        for s0 in range(0, n_reads, cut):
            got = ctx.map_reads(text, reads[s0:s0 + cut], K, *SC, w=W)
            for k in stages:
                stages[k] += ctx.map_stats[k]
            chain_ms += ctx.chain_stats["chain_ms"]
            n_anchors += ctx.chain_stats["anchors"]
            bs = ctx.align_banded_stats()
            fill_ms += bs["fill_ms"]
            walk_ms += bs["walk_ms"]
            placed += sum(g is not None for g in got)
            near += sum(g is not None and abs(g["pos"] - int(p)) <= W for g, p in zip(got, at[s0:s0 + cut]))
        total = time.perf_counter() - t0
        emit(dict(what="map_reads", reads=n_reads, slices=(n_reads + cut - 1) // cut, total_s=total, **stages, chain_device_ms=chain_ms, anchors=n_anchors,
                  align_fill_ms=fill_ms, align_walk_ms=walk_ms, sa_build_ms_last=ctx.sa_stats["build_ms"], placed=placed, within_w=near))
        # the same reads against the whole text, without a chain
        if a.wfa:
            sub = reads[:a.wfa]
            bound = [len(r) - int(1.5 * 6.67 * RATE * LEN) for r in sub]   # 1.5 x the expected penalty, as tools/wfa_batch.py leaves it
            dev = []
            for r in range(2):
                sc = ctx.scores_wfa_sg(sub + [text], list(range(len(sub))), [len(sub)] * len(sub), *SC, min_score=bound)
                dev.append(ctx.align_wfa_stats()["sweep_ms"])
            emit(dict(what="scores_wfa_sg whole text", reads=len(sub), text=TEXT, sweep_ms=dev[-1], ms_per_read=dev[-1] / len(sub),
                      found=sum(s is not None for s in sc)))
            a.wfa = 0   # once
    ctx.close()


if __name__ == "__main__":
    main()
