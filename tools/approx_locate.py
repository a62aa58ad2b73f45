"""From k-edit hits to placements (pwa_approx_starts, Context.locate_approx / align_approx), DESIGN.md §3.19.

The shapes of tools/approx_find.py (random DNA; every pattern is a piece of the text with 5 % edits):
  a   4 096 patterns of 150 against 1 Mb, k = 8
  b   64 patterns of 150 against 16 Mb, k = 8
  c   256 patterns of 500 against 4 Mb, k = 25
Per shape and per selection ("all": every hit, "minima": the locally minimal ends): the number of hits, the device ms of the starts
pass (HIP events inside the library: coding the text, the reversed masks, the scans; median of --reps calls after one warm-up call,
with min and max), the text columns it scanned, cells = m x columns and cells per second; from the same run the count pass's ms and
its cells per second (find_approx, median of the same number of calls), and the wall ms of the whole locate_approx call.
Shape a with "minima" also runs align_approx and records the fill and walk ms of the alignment call (align_gotoh_stats).

One GPU process at a time: the parent never touches the GPU; it runs every shape in a child of its own under a time limit, one after
the other, stops at the first that fails, and appends the children's JSON lines to --out.

    python tools/approx_locate.py [--reps 5] [--shapes a,b,c] [--limit 400] [--out profiles/approx_locate.jsonl]
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

from approx_find import SHAPES  # noqa: E402
from banded_batch import fit, gen_dna, mutate  # noqa: E402


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
    count, every = [], None
    for r in range(reps + 1):
        every = ctx.find_approx(text, packed, k)
        if r:
            count.append(ctx.approx_stats["count_ms"])
    count_ms = statistics.median(count)
    count_rate = m * ctx.approx_stats["columns"] / (count_ms * 1e-3)
    ok = True
    for select in ("all", "minima"):
        hits = every if select == "all" else pkg.approx_minima(every, [m] * n_pat, k, n)
        dev, starts = [], None
        for r in range(reps + 1):
            starts = ctx.starts_approx(text, packed, hits)
            if r:
                dev.append(ctx.approx_starts_stats["ms"])
        st = ctx.approx_starts_stats
        ok = ok and all(s is not None and m - d <= e - s <= m + d for h, ss in zip(hits, starts) for (e, d), s in zip(h, ss))
        wall = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            placed = ctx.locate_approx(text, packed, k, select=select)
            t1 = time.perf_counter()
            if r:
                wall.append(1e3 * (t1 - t0))
        ok = ok and [[s for s, _, _ in x] for x in placed] == starts
        ms = statistics.median(dev)
        cells = m * st["columns"]
        row = dict(shape=shape, select=select, patterns=n_pat, m=m, n=n, k=k, hits=st["hits"], columns=st["columns"], cells=cells, starts_ms=ms,
                   starts_ms_min=min(dev), starts_ms_max=max(dev), cells_per_s=cells / (ms * 1e-3), count_ms=count_ms, count_ms_min=min(count),
                   count_ms_max=max(count), count_cells_per_s=count_rate, rate_ratio=cells / (ms * 1e-3) / count_rate,
                   locate_wall_ms=statistics.median(wall), starts_within_bounds=ok, reps=reps)
        if shape == "a" and select == "minima":
            fill, walk, al = [], [], None
            for r in range(reps + 1):
                t0 = time.perf_counter()
                al = ctx.align_approx(text, packed, k, select=select)
                t1 = time.perf_counter()
                if r:
                    gs = ctx.align_gotoh_stats()
                    fill.append(gs["fill_ms"])
                    walk.append(gs["walk_ms"])
            ok = ok and all(a["score"] == -a["dist"] for x in al for a in x)
            row.update(align_fill_ms=statistics.median(fill), align_walk_ms=statistics.median(walk), align_wall_ms=1e3 * (t1 - t0),
                       alignments=sum(len(x) for x in al), score_is_minus_dist=ok)
        print(json.dumps(row), flush=True)
    ctx.close()
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--limit", type=int, default=400, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_locate.jsonl"))
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
