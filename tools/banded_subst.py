"""Banded affine-gap alignments and scores under a substitution matrix (pwa_align_banded_subst_batch_cigar, pwa_scores_banded_subst)
next to the byte-compare banded calls, DESIGN.md §3.15.

The four shapes of tools/banded_batch.py (k1, k10, k30, sg: its generators, seeds and scoring (1, -4, -6, -1)), with the table that
says the same thing: match on the diagonal and mismatch off it, over ACGT.  Per shape, in ONE child process, on the same pairs, each
call repeated --reps times after a warm-up call, medians:
  align_banded_batch_cigar, then align_banded_subst_batch_cigar right after it  -> fill ms, walk ms of both and their ratios;
  scores_banded, then scores_banded_subst right after it (end cells wanted)     -> score-pass ms of both and their ratio.
The yardstick is the byte-compare kernels in the same run.  There is no threshold on the times; the child ends with status 3 if any
score (or end cell of the score calls) differs between the two forms.

One more shape, `protein`: 1024 pairs 5000 x 5000, NW, half-width 128, under a 24-symbol protein-like table (entries in [-4, 11],
asymmetric) with gaps (-11, -1): a list that no call could run before the banded table calls (patterns above 1024 symbols under a
table); the two new calls only.

One GPU process at a time: the parent never touches the GPU; it runs every shape in a child of its own under a time limit, one after
the other, stops at the first that fails, and appends the children's JSON lines to profiles/banded_subst.jsonl.

    python tools/banded_subst.py [--reps 3] [--shapes k1,k10,k30,sg,protein] [--limit 420]
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

from banded_batch import SC, band_cells, fit, gen_dna, mutate, stat   # noqa: E402

OUT = os.path.join(ROOT, "profiles", "banded_subst.jsonl")
PROTEIN = b"ARNDCQEGHILKMFPSTWYVBZX*"


def timed(reps, call, stats):
    """call() reps + 1 times (the first is the warm-up) -> (last result, wall ms list, [stats() after every measured call])"""
    wall, st, res = [], [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        res = call()
        t1 = time.perf_counter()
        if r:
            wall.append((t1 - t0) * 1e3)
            st.append(stats())
    return res, wall, st


def med(st, key):
    return statistics.median(x[key] for x in st)


def align_row(shape, mode, form, pairs, cells, res, wall, st):
    fill, walk = med(st, "fill_ms"), med(st, "walk_ms")
    return dict(shape=shape, mode=mode, form=form, pairs=pairs, call_ms=stat(wall), fill_ms=fill, walk_ms=walk, device_ms=fill + walk,
                band_bytes=st[-1]["band_bytes"], cells=cells, cells_per_s=cells / ((fill + walk) * 1e-3),
                mean_score=float(np.mean([x["score"] for x in res])))


def scores_row(shape, mode, form, pairs, cells, res, wall, st):
    fill = med(st, "fill_ms")
    return dict(shape=shape, mode=mode, form=form, pairs=pairs, call_ms=stat(wall), score_pass_ms=fill, cells=cells,
                in_band_cells=st[-1]["in_band_cells"], cells_per_s=cells / (fill * 1e-3), mean_score=float(np.mean(res[0])))


def run_shape(shape, reps):
    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    rng = np.random.default_rng(2026)
    rows = []
    if shape == "protein":
        n, count, w = 5000, 1024, 128
        alpha = np.frombuffer(PROTEIN[:20], np.uint8)
        seqs = []
        for k in range(count):
            p = rng.choice(alpha, n)
            t = p.copy()
            sub = rng.random(n) < 0.1
            t[sub] = rng.choice(alpha, int(sub.sum()))
            seqs += [p.tobytes(), t.tobytes()]
        pa, pb = list(range(0, 2 * count, 2)), list(range(1, 2 * count, 2))
        band = pkg.band_around(n, n, w)
        bands, cells, mode, go, ge = [band] * count, count * band_cells(n, n, *band), "nw", -11, -1
        table = pkg.subst_table(PROTEIN, np.random.RandomState(24).randint(-4, 12, size=(24, 24)), unknown=22)
        res, wall, st = timed(reps, lambda: ctx.align_banded_subst_batch_cigar(mode, seqs, pa, pb, table, go, ge, bands), ctx.align_banded_stats)
        rows.append(align_row(shape, mode, "banded_subst", count, cells, res, wall, st))
        sres, wall, st = timed(reps, lambda: ctx.scores_banded_subst(mode, seqs, pa, pb, table, go, ge, bands, want_end=True), ctx.scores_banded_stats)
        rows.append(scores_row(shape, mode, "scores_banded_subst", count, cells, sres, wall, st))
        equal = [x["score"] for x in res] == sres[0]
        rows.append(dict(shape=shape, verdict="alignment scores = score-pass scores", holds=equal))
    else:
        if shape in ("k1", "k10", "k30"):
            n, count, w = dict(k1=(1000, 4096, 32), k10=(10000, 4096, 128), k30=(30000, 1024, 256))[shape]
            seqs = []
            for k in range(count):
                p = gen_dna(rng, n)
                seqs += [p.tobytes(), fit(rng, mutate(rng, p, 0.03), n)]
            pa, pb = list(range(0, 2 * count, 2)), list(range(1, 2 * count, 2))
            band = pkg.band_around(n, n, w)
            bands, cells, mode = [band] * count, count * band_cells(n, n, *band), "nw"
        else:
            texts = [gen_dna(rng, 4000) for _ in range(64)]
            seqs = [t.tobytes() for t in texts]
            pa, pb, bands, cells, mode = [], [], [], 0, "sg"
            for k in range(65536):
                d = int(rng.integers(0, 2400))
                seqs.append(fit(rng, mutate(rng, texts[k % 64][d:d + 1500], 0.03), 1500))
                pa.append(64 + k)
                pb.append(k % 64)
                bands.append(pkg.band_around(1500, 4000, 100, diag=d))
                cells += band_cells(1500, 4000, *bands[-1])
        match, mismatch, go, ge = SC
        table = pkg.subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), match, mismatch))
        a0, wall, st = timed(reps, lambda: ctx.align_banded_batch_cigar(mode, seqs, pa, pb, *SC, bands), ctx.align_banded_stats)
        rows.append(align_row(shape, mode, "banded", len(pa), cells, a0, wall, st))
        a1, wall, st = timed(reps, lambda: ctx.align_banded_subst_batch_cigar(mode, seqs, pa, pb, table, go, ge, bands), ctx.align_banded_stats)
        rows.append(align_row(shape, mode, "banded_subst", len(pa), cells, a1, wall, st))
        s0, wall, st = timed(reps, lambda: ctx.scores_banded(mode, seqs, pa, pb, *SC, bands, want_end=True), ctx.scores_banded_stats)
        rows.append(scores_row(shape, mode, "scores_banded", len(pa), cells, s0, wall, st))
        s1, wall, st = timed(reps, lambda: ctx.scores_banded_subst(mode, seqs, pa, pb, table, go, ge, bands, want_end=True), ctx.scores_banded_stats)
        rows.append(scores_row(shape, mode, "scores_banded_subst", len(pa), cells, s1, wall, st))
        equal = [x["score"] for x in a0] == [x["score"] for x in a1] == s0[0] and s0 == s1 and a0 == a1
        rows.append(dict(shape=shape, verdict="table form = byte-compare form: scores, end cells, strings", holds=equal,
                         fill_ratio=rows[1]["fill_ms"] / rows[0]["fill_ms"], walk_ratio=rows[1]["walk_ms"] / rows[0]["walk_ms"],
                         score_pass_ratio=rows[3]["score_pass_ms"] / rows[2]["score_pass_ms"]))
    ctx.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    return 0 if equal else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="k1,k10,k30,sg,protein")
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
