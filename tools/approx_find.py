"""k-edit approximate search (pwa_approx_find: the count pass), DESIGN.md §3.18.

Shapes (random DNA; every pattern is a piece of the text with 5 % edits):
  a   4 096 patterns of 150 against 1 Mb, k = 8
  b   64 patterns of 150 against 16 Mb, k = 8
  c   256 patterns of 500 against 4 Mb, k = 25
Per shape: device ms of the count pass (HIP events inside the library: coding the text, building the masks, the scan; median of
--reps calls after one warm-up call), the columns the tasks scanned (warm-up included), cells = m x columns and cells per second, and
the wall ms of the whole call.
Shape a also runs its 4 096 (pattern, text) pairs through the semi-global score pass Context.scores("sg", ..., 0, -1, -1) runs -- a
prepared batch of it, so that its device ms (events) can be read -- which answers a smaller question (one best end per pair) with a
DP cell per (row, column); `ratio` = count pass ms / that.  Where a pattern has a hit, its best distance must equal minus that score.

One GPU process at a time: the parent never touches the GPU; it runs every shape in a child of its own under a time limit, one after
the other, stops at the first that fails, and appends the children's JSON lines to --out.

    python tools/approx_find.py [--reps 5] [--shapes a,b,c] [--limit 400] [--out profiles/approx_find.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from banded_batch import fit, gen_dna, mutate  # noqa: E402

SHAPES = dict(a=(4096, 150, 1 << 20, 8), b=(64, 150, 16 << 20, 8), c=(256, 500, 4 << 20, 25))


def run_shape(shape, reps):
    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    n_pat, m, n, k = SHAPES[shape]
    rng = np.random.default_rng(2031)
    text = gen_dna(rng, n)
    pats = []
    for s in rng.integers(0, n - m, size=n_pat):
        pats.append(fit(rng, mutate(rng, text[s:s + m], 0.05), m))
    text = text.tobytes()
    packed = pkg.pack_sequences(pats)
    dev, wall, res = [], [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        res = ctx.count_approx(text, packed, k)
        t1 = time.perf_counter()
        if r:
            dev.append(ctx.approx_stats["count_ms"])
            wall.append(1e3 * (t1 - t0))
    counts, best = res
    st = ctx.approx_stats
    ms = statistics.median(dev)
    cells = m * st["columns"]
    row = dict(shape=shape, patterns=n_pat, m=m, n=n, k=k, tasks=st["tasks"], columns=st["columns"], cells=cells, count_ms=ms,
               count_ms_min=min(dev), count_ms_max=max(dev), cells_per_s=cells / (ms * 1e-3), call_wall_ms=statistics.median(wall),
               hits=int(sum(counts)), patterns_with_a_hit=sum(b is not None for b in best), reps=reps)
    ok = True
    if shape == "a":
        seqs = pats + [text]
        pa, pb = list(range(n_pat)), [n_pat] * n_pat
        b = ctx.batch("sg", seqs, pa, pb, 0, -1, -1)
        sg = []
        for r in range(reps + 1):
            b.run()
            sc = b.fetch()
            if r:
                sg.append(b.last_ms())
        b.close()
        t0 = time.perf_counter()
        sc2 = ctx.scores("sg", seqs, pa, pb, 0, -1, -1)
        sg_wall = 1e3 * (time.perf_counter() - t0)
        ok = sc == sc2 and all(bq is None or bq[0] == -s for bq, s in zip(best, sc)) and all((bq is None) == (-s > k) for bq, s in zip(best, sc))
        sg_ms = statistics.median(sg)
        row.update(sg_scores_ms=sg_ms, sg_scores_ms_min=min(sg), sg_scores_ms_max=max(sg), sg_call_wall_ms=sg_wall, sg_cells=n_pat * m * n,
                   ratio=ms / sg_ms, best_equals_minus_sg_score=ok)
    ctx.close()
    print(json.dumps(row), flush=True)
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--limit", type=int, default=400, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_find.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_shape(a.child, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        with open(a.out, "a") as f:
            for x in r.stdout.splitlines():
                if x.startswith("{"):
                    f.write(x + "\n")
                    print(x, flush=True)
        if r.returncode != 0:
            print("shape %s ended with status %d: stopping" % (shape, r.returncode), file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
