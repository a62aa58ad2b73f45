"""Wavefront (WFA) global affine-gap alignments of long pairs (pwa_align_wfa_batch, pwa_scores_wfa) beside the banded calls
on the same pairs (pwa_align_banded_batch at half-width 128, pwa_scores_banded), scoring (1, -4, -6, -1).

Shapes:
  d1    4096 pairs 10 000 x 10 000 at 1 % divergence;
  d3    4096 pairs 10 000 x 10 000 at 3 % divergence;
  k30   1024 pairs 30 000 x 30 000 at 1 % divergence.
The WFA alignment call gets a bound per pair (min_score) that leaves room for 1.5 times the penalty the divergence lets one expect
(13.3 per edited symbol: a third substitutions at 10, two thirds one-symbol gaps at 15): without a bound the plan reaches the penalty
of "all D then all I" and 12 bytes per planned cell are gigabytes per pair.  The score call runs without a bound: its ring does not
grow with the plan.

Per (shape, call): whole-call wall ms and device ms (pwa_wfa_last_stats / pwa_align_banded_last_stats / pwa_scores_banded_last_stats),
medians over --reps repetitions after one warm-up call; the cells the call computed (wavefront cells up to each pair's penalty, resp.
in-band cells); the WFA workspace; and whether the banded score equals the exact one for every pair.  Nothing is asserted about which
is faster: the lines say what was measured.

--legs codes runs the WFA calls alone -- pwa_scores_wfa, pwa_align_wfa_batch and pwa_align_wfa_codes_batch (the ring sweep with one code
byte per planned cell) with the same bound, in one process, so that the three stand next to each other -- and appends
to profiles/wfa_codes_batch.jsonl; the codes line also says whether every op list equals the offsets form's.  --legs all (the default)
runs every call, the codes form included.

--legs sg runs the semi-global form (pwa_scores_wfa_sg, pwa_align_wfa_sg_batch) on seeded reads in their regions --
  s15   65 536 reads 1500 in regions of 4000 at 1 % divergence;
  s50   4096 reads 5000 in regions of 7000 at 1 %;
  s50d3 4096 reads 5000 in regions of 7000 at 3 %
-- with a bound of 1.5 times the expected penalty (6.67 per edited symbol on the per-pattern-symbol scale: substitutions at 5, one-symbol
gaps at 7 and 8), beside pwa_scores_banded / pwa_align_banded_batch in mode sg at +-100 and +-256 diagonals around the read's seed, and
appends to profiles/wfa_sg_batch.jsonl; the banded lines say for how many pairs the banded score equals the exact one.

One GPU process at a time: the parent never touches the GPU; it runs every shape in a child of its own under a time limit, one after
the other, stops at the first that fails, and appends the children's JSON lines to --out (profiles/wfa_batch.jsonl).

    python tools/wfa_batch.py [--reps 3] [--shapes d1,d3,k30] [--legs all|codes|sg] [--limit 420] [--out FILE]
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

SC = (1, -4, -6, -1)
OUT = os.path.join(ROOT, "profiles", "wfa_batch.jsonl")
OUT_CODES = os.path.join(ROOT, "profiles", "wfa_codes_batch.jsonl")
SHAPES = dict(d1=(10000, 4096, 0.01), d3=(10000, 4096, 0.03), k30=(30000, 1024, 0.01))
HALF_WIDTH = 128
OUT_SG = os.path.join(ROOT, "profiles", "wfa_sg_batch.jsonl")
SHAPES_SG = dict(s15=(1500, 4000, 65536, 0.01), s50=(5000, 7000, 4096, 0.01), s50d3=(5000, 7000, 4096, 0.03))
HALF_WIDTHS_SG = (100, 256)


def gen_dna(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n)


def mutate(rng, s, rate):
    s = s.copy()
    sub = rng.random(len(s)) < rate / 3
    s[sub] = gen_dna(rng, int(sub.sum()))
    at = np.flatnonzero(rng.random(len(s)) < rate / 3)
    s = np.insert(s, at, gen_dna(rng, len(at)))
    return s[rng.random(len(s)) >= rate / 3]


def fit(rng, s, n):
    return (s[:n] if len(s) >= n else np.concatenate([s, gen_dna(rng, n - len(s))])).tobytes()


def band_cells(n, m, lo, hi):
    i = np.arange(1, n + 1, dtype=np.int64)
    return int(np.maximum(0, np.minimum(m, i + hi) - np.maximum(1, i + lo) + 1).sum())


def stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), n=len(xs)) if xs else None


def timed(reps, call, stats):
    wall, rows, res = [], [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        res = call()
        st = stats()
        t1 = time.perf_counter()
        if r:
            wall.append((t1 - t0) * 1e3)
            rows.append(st)
    return res, wall, rows


def run_shape_sg(shape, reps):
    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(2026)
    n, m, count, rate = SHAPES_SG[shape]
    seqs, seeds = [], []
    for k in range(count):
        t = gen_dna(rng, m)
        at = int(rng.integers(0, m - n + 1))
        seqs += [fit(rng, mutate(rng, t[at:at + n], rate), n), t.tobytes()]
        seeds.append(at)
    pa, pb = list(range(0, 2 * count, 2)), list(range(1, 2 * count, 2))
    head = dict(shape=shape, scoring=SC, pairs=count, n=n, m=m, divergence=rate)
    x, o, ei, ed, g = pkg.wfa_sg_plan(*SC, [])["pen"]
    budget = int(1.5 * 6.67 * rate * n)      # penalty the bound leaves room for
    bound = SC[0] * n - g * budget           # ... as a score
    plan = pkg.wfa_sg_plan(*SC, [(n, m)], bound)
    out = []
    (scores, ends), wall, rows = timed(reps, lambda: ctx.scores_wfa_sg(seqs, pa, pb, *SC, min_score=bound, want_end=True), ctx.align_wfa_stats)
    found = [s is not None for s in scores]
    out.append(dict(head, call="scores_wfa_sg", min_score=bound, p_max=plan["p_max"][0], call_ms=stat(wall), device_ms=statistics.median(r["sweep_ms"] for r in rows),
                    device_ms_all=[r["sweep_ms"] for r in rows], cells=rows[-1]["cells"], workspace_bytes=rows[-1]["workspace_bytes"], found=sum(found),
                    mean_score=float(np.mean([s for s in scores if s is not None]))))
    al, wall, rows = timed(reps, lambda: ctx.align_wfa_sg_batch(seqs, pa, pb, *SC, min_score=bound), ctx.align_wfa_stats)
    out.append(dict(head, call="align_wfa_sg_batch", min_score=bound, p_max=plan["p_max"][0], planned_cells_per_pair=plan["cells"][0], call_ms=stat(wall),
                    sweep_ms=stat([r["sweep_ms"] for r in rows]), walk_ms=stat([r["walk_ms"] for r in rows]),
                    device_ms=statistics.median(r["sweep_ms"] + r["walk_ms"] for r in rows), device_ms_all=[r["sweep_ms"] + r["walk_ms"] for r in rows],
                    cells=rows[-1]["cells"], workspace_bytes=rows[-1]["workspace_bytes"], found=sum(a["score"] is not None for a in al),
                    scores_and_ends_equal_the_score_call=[(a["score"], a["end"]) for a in al] == list(zip(scores, ends))))
    del al
    for hw in HALF_WIDTHS_SG:
        bands = [pkg.band_around(n, m, hw, diag=at) for at in seeds]
        cells = sum(band_cells(n, m, *b) for b in bands[:64]) * (count // 64)   # (from the first 64 pairs: the seeds are uniform)
        bsc, wall, rows = timed(reps, lambda: ctx.scores_banded("sg", seqs, pa, pb, *SC, bands), ctx.scores_banded_stats)
        exact = sum(b == s for b, s in zip(bsc, scores))
        out.append(dict(head, call="scores_banded", mode="sg", half_width=hw, call_ms=stat(wall), device_ms=statistics.median(r["fill_ms"] for r in rows),
                        device_ms_all=[r["fill_ms"] for r in rows], cells=rows[-1]["in_band_cells"], pairs_with_the_exact_score=exact, every_score_exact=exact == count))
        bal, wall, rows = timed(reps, lambda: ctx.align_banded_batch("sg", seqs, pa, pb, *SC, bands), ctx.align_banded_stats)
        exact = sum(b["score"] == s for b, s in zip(bal, scores))
        out.append(dict(head, call="align_banded_batch", mode="sg", half_width=hw, call_ms=stat(wall), fill_ms=stat([r["fill_ms"] for r in rows]),
                        walk_ms=stat([r["walk_ms"] for r in rows]), device_ms=statistics.median(r["fill_ms"] + r["walk_ms"] for r in rows),
                        device_ms_all=[r["fill_ms"] + r["walk_ms"] for r in rows], cells=cells, band_bytes=rows[-1]["band_bytes"],
                        pairs_with_the_exact_score=exact, every_score_exact=exact == count))
        del bal
    ctx.close()
    for r in out:
        print(json.dumps(r), flush=True)
    return 0


def run_shape(shape, reps, legs):
    if legs == "sg":
        return run_shape_sg(shape, reps)
    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(2026)
    n, count, rate = SHAPES[shape]
    seqs = []
    for k in range(count):
        p = gen_dna(rng, n)
        seqs += [p.tobytes(), fit(rng, mutate(rng, p, rate), n)]
    pa, pb = list(range(0, 2 * count, 2)), list(range(1, 2 * count, 2))
    head = dict(shape=shape, scoring=SC, pairs=count, n=n, m=n, divergence=rate)
    x, o, e, g = pkg.wfa_plan(*SC, [])["pen"]
    budget = int(1.5 * 13.3 * rate * n)                 # penalty the bound leaves room for
    bound = (SC[0] * 2 * n - g * budget) // 2            # ... as a score
    plan = pkg.wfa_plan(*SC, [(n, n)], bound)

    out = []
    scores, wall, rows = timed(reps, lambda: ctx.scores_wfa(seqs, pa, pb, *SC), ctx.align_wfa_stats)
    out.append(dict(head, call="scores_wfa", min_score=None, call_ms=stat(wall), device_ms=statistics.median(r["sweep_ms"] for r in rows),
                    cells=rows[-1]["cells"], workspace_bytes=rows[-1]["workspace_bytes"], mean_score=float(np.mean(scores))))
    al, wall, rows = timed(reps, lambda: ctx.align_wfa_batch(seqs, pa, pb, *SC, min_score=bound), ctx.align_wfa_stats)
    found = [a["score"] is not None for a in al]
    out.append(dict(head, call="align_wfa_batch", min_score=bound, p_max=plan["p_max"][0], planned_cells_per_pair=plan["cells"][0], call_ms=stat(wall),
                    sweep_ms=stat([r["sweep_ms"] for r in rows]), walk_ms=stat([r["walk_ms"] for r in rows]),
                    device_ms=statistics.median(r["sweep_ms"] + r["walk_ms"] for r in rows), cells=rows[-1]["cells"],
                    workspace_bytes=rows[-1]["workspace_bytes"], found=sum(found),
                    scores_equal_the_score_call=[a["score"] for a in al if a["score"] is not None] == [s for s, f in zip(scores, found) if f]))
    ops = [a["ops"] for a in al]
    del al
    al, wall, rows = timed(reps, lambda: ctx.align_wfa_batch(seqs, pa, pb, *SC, min_score=bound, form="codes"), ctx.align_wfa_stats)
    out.append(dict(head, call="align_wfa_codes_batch", min_score=bound, p_max=plan["p_max"][0], planned_cells_per_pair=plan["cells"][0], call_ms=stat(wall),
                    sweep_ms=stat([r["sweep_ms"] for r in rows]), walk_ms=stat([r["walk_ms"] for r in rows]),
                    device_ms=statistics.median(r["sweep_ms"] + r["walk_ms"] for r in rows), cells=rows[-1]["cells"],
                    workspace_bytes=rows[-1]["workspace_bytes"], found=sum(a["score"] is not None for a in al),
                    ops_equal_the_offsets_form=[a["ops"] for a in al] == ops))
    del al, ops
    if legs == "codes":
        ctx.close()
        for r in out:
            print(json.dumps(r), flush=True)
        return 0
    band = pkg.band_around(n, n, HALF_WIDTH)
    cells = count * band_cells(n, n, *band)
    bal, wall, rows = timed(reps, lambda: ctx.align_banded_batch("nw", seqs, pa, pb, *SC, [band] * count), ctx.align_banded_stats)
    exact = sum(b["score"] == s for b, s in zip(bal, scores))
    out.append(dict(head, call="align_banded_batch", half_width=HALF_WIDTH, call_ms=stat(wall), fill_ms=stat([r["fill_ms"] for r in rows]),
                    walk_ms=stat([r["walk_ms"] for r in rows]), device_ms=statistics.median(r["fill_ms"] + r["walk_ms"] for r in rows), cells=cells,
                    band_bytes=rows[-1]["band_bytes"], pairs_with_the_exact_score=exact, every_score_exact=exact == count))
    del bal
    bsc, wall, rows = timed(reps, lambda: ctx.scores_banded("nw", seqs, pa, pb, *SC, [band] * count), ctx.scores_banded_stats)
    exact = sum(b == s for b, s in zip(bsc, scores))
    out.append(dict(head, call="scores_banded", half_width=HALF_WIDTH, call_ms=stat(wall), device_ms=statistics.median(r["fill_ms"] for r in rows),
                    cells=rows[-1]["in_band_cells"], pairs_with_the_exact_score=exact, every_score_exact=exact == count))
    ctx.close()
    for r in out:
        print(json.dumps(r), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=None, help="default: d1,d3,k30, or s15,s50,s50d3 with --legs sg")
    ap.add_argument("--limit", type=int, default=420, help="seconds per shape")
    ap.add_argument("--legs", default="all", choices=["all", "codes", "sg"])
    ap.add_argument("--out", default=None, help="default: profiles/wfa_batch.jsonl, profiles/wfa_codes_batch.jsonl with --legs codes, profiles/wfa_sg_batch.jsonl with --legs sg")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_shape(a.child, a.reps, a.legs)
    a.out = a.out or (OUT_CODES if a.legs == "codes" else OUT_SG if a.legs == "sg" else OUT)
    a.shapes = a.shapes or ("s15,s50,s50d3" if a.legs == "sg" else "d1,d3,k30")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--legs", a.legs]
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
