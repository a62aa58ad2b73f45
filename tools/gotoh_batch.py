"""Affine-gap (gotoh) batch alignments next to the linear mode on the same inputs.

Shapes (pwa_align_gotoh_batch_cigar against pwa_align_batch_cigar, scoring (1, -4, -6, -1) against linear (1, -4, -1)):
  g      4096 pairs 150 x 10k (64 reads cut from 64 texts at ~3 % divergence, every read against every text): NW, SW, SG;
  reads  65 536 reads 150 x 400 (each read against its own region), SG;
  wide   1024 pairs 1000 x 10k (one pair per wave: 64 lanes x 16 rows), NW.
Per (shape, mode, form): whole-call wall ms, device ms of the fills and the walks, band bytes (pwa_align_gotoh_last_stats /
pwa_align_last_stats); median and min over --reps repetitions after one warm-up call.  One JSON line each.

    python tools/gotoh_batch.py [--reps 3] [--shapes g,reads,wide]
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
import __graft_entry__ as G  # noqa: E402

GOTOH = (1, -4, -6, -1)
LINEAR = (1, -4, -1)


def gen_dna(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n)


def mutate(rng, s, rate):
    s = s.copy()
    sub = rng.random(len(s)) < rate / 3
    s[sub] = gen_dna(rng, int(sub.sum()))
    at = np.flatnonzero(rng.random(len(s)) < rate / 3)
    s = np.insert(s, at, gen_dna(rng, len(at)))
    return s[rng.random(len(s)) >= rate / 3].tobytes()


def stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), n=len(xs)) if xs else None   # (--reps 0: the warm-up call only)


def rows_for(ctx, shape, mode, seqs, pa, pb, reps):
    out = []
    for form in ("gotoh", "linear"):
        wall, fill, walk, band = [], [], [], 0
        for r in range(reps + 1):
            t0 = time.perf_counter()
            if form == "gotoh":
                res = ctx.align_gotoh_batch_cigar(mode, seqs, pa, pb, *GOTOH)
                st = ctx.align_gotoh_stats()
            else:
                res = ctx.align_batch_cigar(mode, seqs, pa, pb, *LINEAR)
                st = ctx.align_stats()
                st["walk_ms"] = st["traceback_ms"]
            t1 = time.perf_counter()
            if r:
                wall.append((t1 - t0) * 1e3)
                fill.append(st["fill_ms"])
                walk.append(st["walk_ms"])
                band = st["band_bytes"]
        out.append(dict(shape=shape, mode=mode, form=form, scoring=GOTOH if form == "gotoh" else LINEAR, pairs=len(pa), call_ms=stat(wall),
                        fill_ms=stat(fill), walk_ms=stat(walk), band_bytes=band, mean_score=float(np.mean([x["score"] for x in res]))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="g,reads,wide")
    a = ap.parse_args()
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(2026)
    for shape in a.shapes.split(","):
        rows = []
        if shape == "g":
            texts = [gen_dna(rng, 10000) for _ in range(64)]
            pats = [mutate(rng, texts[k][at:at + 150], 0.03)[:150] for k, at in enumerate(rng.integers(0, 9850, 64))]
            seqs = pats + [t.tobytes() for t in texts]
            pa, pb = [i % 64 for i in range(4096)], [64 + i // 64 for i in range(4096)]
            for mode in ("nw", "sw", "sg"):
                rows += rows_for(ctx, shape, mode, seqs, pa, pb, a.reps)
        elif shape == "reads":
            seqs, pa, pb = [], [], []
            for k in range(65536):
                region = gen_dna(rng, 400)
                at = int(rng.integers(0, 250))
                seqs += [mutate(rng, region[at:at + 150], 0.03)[:150], region.tobytes()]
                pa.append(2 * k)
                pb.append(2 * k + 1)
            rows += rows_for(ctx, shape, "sg", seqs, pa, pb, a.reps)
        elif shape == "wide":
            seqs, pa, pb = [], [], []
            for k in range(1024):
                t = gen_dna(rng, 10000)
                at = int(rng.integers(0, 9000))
                seqs += [mutate(rng, t[at:at + 1000], 0.03)[:1000], t.tobytes()]
                pa.append(2 * k)
                pb.append(2 * k + 1)
            rows += rows_for(ctx, shape, "nw", seqs, pa, pb, max(1, a.reps - 1))
        for r in rows:
            print(json.dumps(r), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
