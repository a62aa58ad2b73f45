"""Top-N chains, mapping quality and secondary placements on planted reads (Context.chain_top, Context.map_reads(secondary=);
DESIGN.md §3.26), scoring (1, -4, -6, -1).

The two lists of tools/chain_batch.py (4096 and 65 536 reads of 1500 symbols cut out of a random 1 Mb text and mutated at 8 %, k = 15)
and a repeat list: 4096 such reads cut around the eight copies (2 % apart from each other) of a 1.5 kb unit in the same text.  Per list:
  - chain_top (max_chains 4, min_score 40, min_count 3) on the whole list's seeds: device ms of the chain kernel and of the selection
    behind it from the same call (pwa_chain_top_last_stats), rounds per read, the call's wall ms; medians over --reps repetitions after
    one warm-up call;
  - the same call with min_score = 2^30, where no anchor is a candidate and the selection kernel leaves after one block a read: what
    the keys and the sort cost alone, and so the sort's share of top_ms;
  - Context.chain on the same seeds in the same process, for chain_ms and the wall of the call without a selection;
  - map_reads(secondary=0) and map_reads(secondary=2) in the same process on the first --map reads of the list: wall seconds by stage,
    reads placed, reads with a secondary, reads of mapq 0 and of mapq 60.
Lines go to --out (profiles/chain_top_batch.jsonl).

    python tools/chain_top_batch.py [--reads 4096,65536] [--repeat 4096] [--reps 3] [--slice 4096] [--map 4096] [--out FILE]
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
K, W, LEN, RATE, TEXT, UNIT, COPIES = 15, 100, 1500, 0.08, 1000000, 1500, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="4096,65536")
    ap.add_argument("--repeat", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice", type=int, default=4096)
    ap.add_argument("--map", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_top_batch.jsonl"))
    a = ap.parse_args()

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(7)
    text_arr = gen_dna(rng, TEXT)
    lists = []
    for n_reads in [int(x) for x in a.reads.split(",") if x]:
        at = rng.integers(0, TEXT - LEN, n_reads)
        lists.append(("random", text_arr, at))
    if a.repeat:
        rep = text_arr.copy()
        unit = gen_dna(rng, UNIT)
        loci = [(c + 1) * TEXT // (COPIES + 1) for c in range(COPIES)]
        for p in loci:
            c = unit if p == loci[0] else mutate(rng, unit, 0.02)
            rep[p:p + len(c)] = c
        at = np.array([loci[i % COPIES] + int(rng.integers(-LEN // 2, LEN // 2)) for i in range(a.repeat)])
        lists.append(("repeat", rep, at))
    for name, arr, at in lists:
        n_reads = len(at)
        text = arr.tobytes()
        reads = [mutate(rng, arr[p:p + LEN], RATE).tobytes() for p in at]
        cut = min(a.slice, n_reads)
        with ctx.index(text) as index:
            anchors = []
            for s0 in range(0, n_reads, cut):
                anchors += ctx.seed(index, reads[s0:s0 + cut], K, as_arrays=True)
            rows = {}
            for what, call in (("chain", lambda: ctx.chain(anchors)), ("chain_top", lambda: ctx.chain_top(anchors)),
                               ("chain_top, no candidate", lambda: ctx.chain_top(anchors, min_score=1 << 30))):
                wall, dev, top = [], [], []
                for r in range(a.reps + 1):
                    t0 = time.perf_counter()
                    call()
                    t1 = time.perf_counter()
                    if r:
                        st = ctx.chain_stats if what == "chain" else ctx.chain_top_stats
                        wall.append((t1 - t0) * 1e3)
                        dev.append(st["chain_ms"])
                        top.append(st.get("top_ms", 0.0))
                rows[what] = dict(what=what, list=name, reads=n_reads, anchors=st["anchors"], ranges=st["ranges"], chain_ms=stat(dev), call_ms=stat(wall))
                if what != "chain":
                    rows[what].update(top_ms=stat(top), rounds_per_read=st["rounds"] / n_reads)
            rows["chain_top"]["sort_share"] = rows["chain_top, no candidate"]["top_ms"]["median"] / rows["chain_top"]["top_ms"]["median"]
            for row in rows.values():
                emit(row)
            del anchors
            m = min(a.map, n_reads)
            for secondary in (0, 2, 0, 2):   # each twice: the first pair warms up
                t0 = time.perf_counter()
                got = ctx.map_reads(index, reads[:m], K, *SC, w=W, secondary=secondary)
                total = time.perf_counter() - t0
                row = dict(what="map_reads", list=name, reads=m, secondary=secondary, total_s=total, **ctx.map_stats, placed=sum(g is not None for g in got),
                           within_w=sum(g is not None and abs(g["pos"] - int(p)) <= W for g, p in zip(got, at[:m])))
                if secondary:
                    row.update(with_secondary=sum(g is not None and len(g["secondary"]) > 0 for g in got), mapq_0=sum(g is not None and g["mapq"] == 0 for g in got),
                               mapq_60=sum(g is not None and g["mapq"] == 60 for g in got))
                rows["map-%d" % secondary] = row   # the second of each stays
            emit(rows["map-0"])
            emit(rows["map-2"])
    ctx.close()


if __name__ == "__main__":
    main()
