"""Semi-global (PWA_MODE_SG) next to NW on the same inputs.

Shapes:
  g       4096 pairs 150 x 10k (hw2 -g's workload: 64 patterns x 64 texts): pwa_align_batch_cigar whole-call wall ms, and the device
          ms of the fills and the walks (pwa_align_last_stats); NW also with PWA_NO_GAP_SHIFT=1, the cell form SG uses;
  scores  262 144 pairs 150 x 1000 (1024 patterns x 256 texts): device ms of pwa_batch_run -- SG, NW with end cells (the same
          band-less mini-stripe route, also with PWA_NO_GAP_SHIFT=1) and NW without (the strip engine);
  long    64 pairs 10k x 10k (mutated copies): the fill / walk ms of pwa_align_batch_cigar and the pwa_batch_run ms of scores.
Times: median and min over --reps repetitions after one warm-up call.  One JSON line per (shape, variant).

    python tools/semiglobal_batch.py [--reps 5] [--shapes g,scores,long]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G  # noqa: E402


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
    return dict(median=statistics.median(xs), min=min(xs), n=len(xs))


def context(pkg, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


VARIANTS = [("sg", {}), ("nw", {}), ("nw", {"PWA_NO_GAP_SHIFT": "1"})]


def align_rows(pkg, shape, seqs, pa, pb, sc, reps):
    out, ref = [], None
    for mode, env in VARIANTS:
        c = context(pkg, env)
        wall, fill, walk = [], [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = c.align_batch_cigar(mode, seqs, pa, pb, *sc)
            t1 = time.perf_counter()
            st = c.align_stats()
            if r:
                wall.append((t1 - t0) * 1e3)
                fill.append(st["fill_ms"])
                walk.append(st["traceback_ms"])
        if mode == "sg":
            ref = res
        out.append(dict(shape=shape, mode=mode, env=env, pairs=len(pa), call_ms=stat(wall), fill_ms=stat(fill), walk_ms=stat(walk),
                        mean_score=float(np.mean([x["score"] for x in res]))))
        c.close()
    return out, ref


def scores_rows(pkg, shape, seqs, pa, pb, sc, reps, variants):
    out = []
    for mode, env, want_end in variants:
        c = context(pkg, env)
        b = c.batch(mode, seqs, pa, pb, *sc, want_end)
        b.run()
        b.last_ms()
        t = []
        for _ in range(reps):
            b.run()
            t.append(b.last_ms())
        kern = b.info()["kernel"]
        b.close()
        c.close()
        out.append(dict(shape=shape, mode=mode, env=env, want_end=want_end, pairs=len(pa), run_ms=stat(t), kernel=kern))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="g,scores,long")
    a = ap.parse_args()
    pkg = G.load_pkg()
    rng = np.random.default_rng(2026)
    sc = (1, -1, -1)
    rows = []
    for shape in a.shapes.split(","):
        if shape == "g":   # patterns cut from the texts (a read and its region) at ~3 % divergence
            texts = [gen_dna(rng, 10000) for _ in range(64)]
            pats = [mutate(rng, texts[k][at:at + 150], 0.03)[:150] for k, at in enumerate(rng.integers(0, 9850, 64))]
            seqs = pats + [t.tobytes() for t in texts]
            pa, pb = [i % 64 for i in range(4096)], [64 + i // 64 for i in range(4096)]
            rows += align_rows(pkg, shape, seqs, pa, pb, sc, a.reps)[0]
        elif shape == "scores":
            pats = [gen_dna(rng, 150).tobytes() for _ in range(1024)]
            txts = [gen_dna(rng, 1000).tobytes() for _ in range(256)]
            pa = np.repeat(np.arange(1024, dtype=np.uint32), 256)
            pb = (1024 + np.tile(np.arange(256, dtype=np.uint32), 1024)).astype(np.uint32)
            rows += scores_rows(pkg, shape, pats + txts, pa, pb, sc, a.reps,
                                [("sg", {}, False), ("sg", {}, True), ("nw", {}, True), ("nw", {"PWA_NO_GAP_SHIFT": "1"}, True), ("nw", {}, False)])
        elif shape == "long":
            seqs = []
            for _ in range(64):
                t = gen_dna(rng, 10000)
                seqs += [mutate(rng, t, 0.05)[:10000], t.tobytes()]
            pa, pb = list(range(0, 128, 2)), list(range(1, 128, 2))
            rows += align_rows(pkg, shape, seqs, pa, pb, sc, max(1, a.reps // 2))[0]
            rows += scores_rows(pkg, shape, seqs, np.array(pa, np.uint32), np.array(pb, np.uint32), sc, a.reps,
                                [("sg", {}, True), ("nw", {}, True), ("nw", {"PWA_NO_GAP_SHIFT": "1"}, True)])
        for r in rows:
            if r.get("shape") == shape:
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
