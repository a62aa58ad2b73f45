#!/usr/bin/env python3
"""hw3's alignment phase on few long sequences -- the N-1 alignments against the center (pwa_align_affine_batch) -- on the strips and
on the stripe engine ("hw3 on few long sequences"), and the probe behind the route constants of affine_tb_route.

    python tools/hw3_align_long.py --shape 16x10000 [--shape 16x100000 ...] [--route -1|0|1] [--repeats 3] [--cli]
    python tools/hw3_align_long.py --probe

Sequences as tools/hw3_long.py (NxL: the reference's 16 x 10 kb file, or slices of the 16 x 100 kb file); the center is
sequence 0 (the phase's cost does not depend on which one).  --route sets PWA_AFFINE_TB_ROUTE (-1: the default, by cost).  Per
repeat: wall time of the call, and the stripe engine's event-timed fill / walk ms and band bytes (pwa_align_affine_last_stats).
--cli also times hw3_amd on the shape's FASTA (the score pass, the alignment phase and the host merge).  --probe times synthetic
center-star lists on both engines (strips only where they finish in seconds).  One JSON line per measurement."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hw3_long import shape_records  # noqa: E402


def stats(xs):
    return dict(min=min(xs), median=statistics.median(xs), max=max(xs), n=len(xs))


def context(pkg, route):
    if route >= 0:
        os.environ["PWA_AFFINE_TB_ROUTE"] = str(route)
    try:
        return pkg.Context(0)
    finally:
        os.environ.pop("PWA_AFFINE_TB_ROUTE", None)


def measure(ctx, seqs, pa, pb, sc, repeats):
    wall, fill, walk, first = [], [], [], None
    st = None
    for r in range(repeats + 1):   # (one warm-up call: workspaces, code objects)
        t0 = time.perf_counter()
        got = ctx.align_affine_batch(seqs, pa, pb, *sc)
        w = (time.perf_counter() - t0) * 1e3
        st = ctx.align_affine_stats()
        if first is None:
            first = got
            continue
        assert got == first, "repeats disagree"
        wall.append(w)
        fill.append(st["fill_ms"])
        walk.append(st["walk_ms"])
    return dict(stripe_pairs=st["stripe_pairs"], band_bytes=st["band_bytes"], fill_ms=stats(fill), walk_ms=stats(walk),
                wall_ms=stats(wall), ops=sum(len(g["ops"]) for g in first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[])
    ap.add_argument("--route", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scoring", default="5,-4,-16,-4")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--probe", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_pkg()
    sc = [int(x) for x in a.scoring.split(",")]
    for shape in a.shape:
        n, length = (int(x) for x in shape.lower().split("x"))
        recs = shape_records(n, length)
        seqs = [s for _, s in recs]
        ctx = context(pkg, a.route)
        row = dict(shape=shape, route=a.route, scoring=sc, pairs=n - 1,
                   **measure(ctx, seqs, [0] * (n - 1), list(range(1, n)), sc, a.repeats))
        ctx.close()
        if a.cli:
            with tempfile.TemporaryDirectory() as td:
                with open(os.path.join(td, "in.fa"), "wb") as f:
                    for h, s in recs:
                        f.write(b">" + h + b"\n" + s + b"\n")
                env = dict(os.environ)
                if a.route >= 0:
                    env["PWA_AFFINE_TB_ROUTE"] = str(a.route)
                t0 = time.perf_counter()
                pr = subprocess.run([pkg.HW3_CLI_PATH, "-i", "in.fa", "-o", "out.phy", "-s", ":".join(str(x) for x in sc)], cwd=td,
                                    stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1800, env=env)
                row["hw3_amd_wall_ms"] = (time.perf_counter() - t0) * 1e3
                row["hw3_amd_rc"] = pr.returncode
                if pr.returncode:
                    row["hw3_amd_stderr"] = pr.stderr.decode("latin-1")[-400:]
        print(json.dumps(row), flush=True)
    if a.probe:
        rng = random.Random(3)
        # (pairs, length, strips too): one wave task of `pairs` pairs sharing string1
        for pairs, length, strips in [(64, 1000, True), (16, 2000, True), (4, 4000, True), (1, 10000, False), (1, 20000, False),
                                      (15, 10000, False)]:
            base = bytes(rng.choice(b"ACGT") for _ in range(length))
            seqs = [base] + [bytes(c if rng.random() > 0.1 else rng.choice(b"ACGT") for c in base) for _ in range(pairs)]
            for route in ([0, 1] if strips else [1]):
                ctx = context(pkg, route)
                row = dict(probe="%dx%d" % (pairs, length), route=route, **measure(ctx, seqs, [0] * pairs, list(range(1, pairs + 1)), sc, 2))
                ctx.close()
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
