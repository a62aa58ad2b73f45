"""Banded affine-gap alignments of long pairs (pwa_align_banded_batch_cigar) and their scores-only form (pwa_scores_banded), DESIGN.md
§3.14, scoring (1, -4, -6, -1).

Shapes:
  k1   4096 pairs 1000 x 1000, NW, w = 32 -- and the same pairs through align_gotoh_batch_cigar (the unbanded fill + walk) in the same run;
  k10  4096 pairs 10 000 x 10 000, NW, w = 128;
  k30  1024 pairs 30 000 x 30 000, NW, w = 256;
  sg   65 536 reads 1500 x 4000, SG, band = the read's seeded diagonal +- 100 (64 shared texts).
Per (shape, form): whole-call wall ms, device ms of the fills and the walks, band bytes (pwa_align_banded_last_stats /
pwa_align_gotoh_last_stats), in-band cells and cells per second of fill + walk; medians over --reps repetitions after one warm-up call.

Every shape is also run through the scores form (scores_banded with end cells), on the same pairs in the same child, right after the
alignment form: device ms of the score pass (pwa_scores_banded_last_stats), in-band cells per second, its ratio to the alignment call's
fill, and whether every score equals the alignment call's.  The child ends with status 3 unless the score pass took less device time
than the alignment fill and the scores agree; those lines and their verdicts go to profiles/banded_scores.jsonl.

The k1 child compares the two medians and ends with status 3 unless banded fill + walk took less device time than the unbanded ones
(its verdict goes into the file as a line of its own).  k10 is also run with PWA_BANDED_RL=4 and =8, every pair on 256- and on 512-row
stripes: the data points of the stripe-height rule.

One GPU process at a time: the parent never touches the GPU; it runs every shape in a child of its own under a time limit, one after
the other, stops at the first that fails, and appends the children's JSON lines to profiles/banded_batch.jsonl.

    python tools/banded_batch.py [--reps 3] [--shapes k1,k10,k30,sg] [--limit 420]
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
OUT = os.path.join(ROOT, "profiles", "banded_batch.jsonl")
OUT_SCORES = os.path.join(ROOT, "profiles", "banded_scores.jsonl")


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


def measure(ctx, shape, form, mode, seqs, pa, pb, bands, reps, cells):
    wall, fill, walk, band = [], [], [], 0
    for r in range(reps + 1):
        t0 = time.perf_counter()
        if form == "banded":
            res = ctx.align_banded_batch_cigar(mode, seqs, pa, pb, *SC, bands)
            st = ctx.align_banded_stats()
        else:
            res = ctx.align_gotoh_batch_cigar(mode, seqs, pa, pb, *SC)
            st = ctx.align_gotoh_stats()
        t1 = time.perf_counter()
        if r:
            wall.append((t1 - t0) * 1e3)
            fill.append(st["fill_ms"])
            walk.append(st["walk_ms"])
            band = st["band_bytes"]
    dev = statistics.median(fill) + statistics.median(walk) if fill else None
    return dict(shape=shape, mode=mode, form=form, scoring=SC, pairs=len(pa), call_ms=stat(wall), fill_ms=stat(fill), walk_ms=stat(walk),
                device_ms=dev, band_bytes=band, cells=cells, cells_per_s=cells / (dev * 1e-3) if dev else None,
                mean_score=float(np.mean([x["score"] for x in res])))


def measure_scores(ctx, shape, mode, seqs, pa, pb, bands, reps, cells, align_row):
    """the scores form on the pairs of align_row (the banded alignment form measured just before)"""
    wall, fill, st = [], [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        scores, ei, ej = ctx.scores_banded(mode, seqs, pa, pb, *SC, bands, want_end=True)
        st = ctx.scores_banded_stats()
        t1 = time.perf_counter()
        if r:
            wall.append((t1 - t0) * 1e3)
            fill.append(st["fill_ms"])
    dev = statistics.median(fill) if fill else None
    return dict(shape=shape, mode=mode, form="scores", scoring=SC, pairs=len(pa), call_ms=stat(wall), fill_ms=stat(fill), device_ms=dev,
                cells=cells, in_band_cells=st["in_band_cells"], cells_per_s=cells / (dev * 1e-3) if dev else None,
                align_fill_ms=align_row["fill_ms"]["median"], ratio_to_align_fill=dev / align_row["fill_ms"]["median"] if dev else None,
                mean_score=float(np.mean(scores)))


def scores_verdict(shape, srow, arow):
    ok = srow["device_ms"] < arow["fill_ms"]["median"] and srow["mean_score"] == arow["mean_score"] and srow["in_band_cells"] == srow["cells"]
    return dict(shape=shape, form="scores", verdict="score pass < alignment fill (device ms), equal scores, host cell count = the tool's", holds=ok,
                scores_device_ms=srow["device_ms"], align_fill_ms=arow["fill_ms"]["median"], stripe_rows=None)


def run_shape(shape, reps, rl):
    import __graft_entry__ as G
    if rl:
        os.environ["PWA_BANDED_RL"] = str(rl)   # (read once, by the context)
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(2026)
    rows = []
    if shape in ("k1", "k10", "k30"):
        n, count, w = dict(k1=(1000, 4096, 32), k10=(10000, 4096, 128), k30=(30000, 1024, 256))[shape]
        seqs = []
        for k in range(count):
            p = gen_dna(rng, n)
            seqs += [p.tobytes(), fit(rng, mutate(rng, p, 0.03), n)]
        pa, pb = list(range(0, 2 * count, 2)), list(range(1, 2 * count, 2))
        band = pkg.band_around(n, n, w)
        cells = count * band_cells(n, n, *band)
        rows.append(measure(ctx, shape, "banded", "nw", seqs, pa, pb, [band] * count, reps, cells))
        rows.append(measure_scores(ctx, shape, "nw", seqs, pa, pb, [band] * count, reps, cells, rows[0]))
        if shape == "k1":
            rows.append(measure(ctx, shape, "gotoh", "nw", seqs, pa, pb, None, reps, count * n * n))
    else:
        texts = [gen_dna(rng, 4000) for _ in range(64)]
        seqs = [t.tobytes() for t in texts]
        pa, pb, bands, cells = [], [], [], 0
        for k in range(65536):
            d = int(rng.integers(0, 2400))
            seqs.append(fit(rng, mutate(rng, texts[k % 64][d:d + 1500], 0.03), 1500))
            pa.append(64 + k)
            pb.append(k % 64)
            bands.append(pkg.band_around(1500, 4000, 100, diag=d))
            cells += band_cells(1500, 4000, *bands[-1])
        rows.append(measure(ctx, shape, "banded", "sg", seqs, pa, pb, bands, reps, cells))
        rows.append(measure_scores(ctx, shape, "sg", seqs, pa, pb, bands, reps, cells, rows[0]))
    ctx.close()
    rows.append(scores_verdict(shape, rows[1], rows[0]))
    ok = rows[-1]["holds"]
    for r in rows:
        r["stripe_rows"] = 64 * rl if rl else "by band width"
        print(json.dumps(r), flush=True)
    if shape == "k1":
        faster = rows[0]["device_ms"] < rows[2]["device_ms"]
        print(json.dumps(dict(shape="k1", verdict="banded fill + walk < unbanded fill + walk", holds=faster, banded_device_ms=rows[0]["device_ms"],
                              gotoh_device_ms=rows[2]["device_ms"])), flush=True)
        ok = ok and faster
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="k1,k10,k30,sg")
    ap.add_argument("--limit", type=int, default=420, help="seconds per shape")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rl", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_shape(a.child, a.reps, a.rl)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    steps = []
    for shape in a.shapes.split(","):
        steps += [(shape, 0)] + ([(shape, 4), (shape, 8)] if shape == "k10" else [])
    for shape, rl in steps:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--rl", str(rl)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        with open(OUT, "a") as f, open(OUT_SCORES, "a") as fs:
            for x in lines:
                (fs if json.loads(x).get("form") == "scores" else f).write(x + "\n")
                print(x, flush=True)
        if r.returncode != 0:
            print("shape %s ended with status %d: stopping" % (shape, r.returncode), file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
