"""Banded X-drop extension (pwa_scores_extend_banded, pwa_extend_banded_batch_cigar), DESIGN.md §3.16, scoring (1, -4, -6, -1).

Shapes:
  stop    4096 pairs 10 000 x 10 000 at half-width 128; text rows 1..2000 are a copy of the pattern at ~3 % divergence, the rest is
          unrelated random DNA; xdrop = 100.  The sweep ends in stripe 9 of 40 (256-row stripes).
  nostop  the same shape with the whole text related, xdrop = -1: the cost of the EXT cell and the stripe-end test with nothing saved.
  seeded  65 536 reads 1500 x 4000 (64 shared texts), as extension from a seed at (0, 0) of the region cut out at the read's diagonal:
          band +- 100, xdrop = 100.
The yardstick is always the SW form on the same pairs and bands, in the same child: scores_banded("sw") for the score pass,
align_banded_batch_cigar("sw")'s fill and walk for the alignment.  Per form: device ms (median of --reps after one warm-up call) of the
score pass, the fill and the walk, the EXT / SW ratios and the mean `rows`.

Condition (shape `stop`): the EXT score pass takes at most 0.5 x the SW score pass, and the EXT fill at most 0.5 x the SW fill; the
child -- and the tool -- end with status 3 if it fails.  The other shapes have none.

One GPU process at a time: the parent never touches the GPU; it runs every shape in a child of its own under a time limit, one after
the other, stops at the first that fails, and appends the children's JSON lines to profiles/banded_ext.jsonl.

    python tools/banded_ext.py [--reps 3] [--shapes stop,nostop,seeded] [--limit 420]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from banded_batch import fit, gen_dna, mutate  # noqa: E402

SC = (1, -4, -6, -1)
OUT = os.path.join(ROOT, "profiles", "banded_ext.jsonl")


def timed(reps, call, stats):
    """median of each device figure of stats() over reps calls after a warm-up call; the last call's result"""
    got, res = [], None
    for r in range(reps + 1):
        res = call()
        if r:
            got.append(stats())
    return res, {k: statistics.median(x[k] for x in got) for k in got[0] if k.endswith("_ms")}


def run_shape(shape, reps):
    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(2027)
    if shape in ("stop", "nostop"):
        n, count, w, xdrop = 10000, 4096, 128, (100 if shape == "stop" else -1)
        seqs = []
        for k in range(count):
            p = gen_dna(rng, n)
            t = fit(rng, mutate(rng, p, 0.03), n) if shape == "nostop" else fit(rng, mutate(rng, p[:2000], 0.03)[:2000], n)
            seqs += [p.tobytes(), t]
        pa, pb = list(range(0, 2 * count, 2)), list(range(1, 2 * count, 2))
        bands = [(-w, w)] * count
    else:
        xdrop = 100
        texts = [gen_dna(rng, 6400) for _ in range(64)]
        seqs, pa, pb = [], [], []
        for k in range(65536):
            d = int(rng.integers(0, 2400))
            seqs += [fit(rng, mutate(rng, texts[k % 64][d:d + 1500], 0.03), 1500), texts[k % 64][d:d + 4000].tobytes()]   # the region from the seed on
            pa.append(2 * k)
            pb.append(2 * k + 1)
        bands = [(-100, 100)] * 65536
    sw_s, t_sw_s = timed(reps, lambda: ctx.scores_banded("sw", seqs, pa, pb, *SC, bands, want_end=True), ctx.scores_banded_stats)
    ex_s, t_ex_s = timed(reps, lambda: ctx.scores_extend_banded(seqs, pa, pb, *SC, bands, xdrop, want_end=True), ctx.extend_banded_stats)
    sw_a, t_sw_a = timed(reps, lambda: ctx.align_banded_batch_cigar("sw", seqs, pa, pb, *SC, bands), ctx.align_banded_stats)
    ex_a, t_ex_a = timed(reps, lambda: ctx.extend_banded_batch_cigar(seqs, pa, pb, *SC, bands, xdrop), ctx.extend_banded_stats)
    ctx.close()
    equal = [(x["score"], x["end"], x["rows"]) for x in ex_a] == list(zip(ex_s[0], zip(ex_s[1], ex_s[2]), ex_s[3]))
    row = dict(shape=shape, scoring=SC, pairs=len(pa), xdrop=xdrop, half_width=bands[0][1], mean_rows=float(np.mean(ex_s[3])),
               mean_score_ext=float(np.mean(ex_s[0])), mean_score_sw=float(np.mean(sw_s[0])),
               sw_scores_ms=t_sw_s["fill_ms"], ext_scores_ms=t_ex_s["fill_ms"], scores_ratio=t_ex_s["fill_ms"] / t_sw_s["fill_ms"],
               sw_fill_ms=t_sw_a["fill_ms"], ext_fill_ms=t_ex_a["fill_ms"], fill_ratio=t_ex_a["fill_ms"] / t_sw_a["fill_ms"],
               sw_walk_ms=t_sw_a["walk_ms"], ext_walk_ms=t_ex_a["walk_ms"], scores_equal_alignments=equal, reps=reps)
    print(json.dumps(row), flush=True)
    ok = equal
    if shape == "stop":
        holds = row["scores_ratio"] <= 0.5 and row["fill_ratio"] <= 0.5
        print(json.dumps(dict(shape=shape, verdict="EXT score pass <= 0.5 x SW score pass and EXT fill <= 0.5 x SW fill (device ms)", holds=holds,
                              scores_ratio=row["scores_ratio"], fill_ratio=row["fill_ratio"], mean_rows=row["mean_rows"])), flush=True)
        ok = ok and holds
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="stop,nostop,seeded")
    ap.add_argument("--limit", type=int, default=420, help="seconds per shape")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_shape(a.child, a.reps)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        with open(OUT, "a") as f:
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
