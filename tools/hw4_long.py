#!/usr/bin/env python3
"""hw4's all-pairs distances on few long sequences: device time of the distance pass, wall time of pwa_distances and of the
hw4-compatible CLI ("hw4 on few long sequences").

    python tools/hw4_long.py --shape 16x10000 [--shape 16x100000 ...] [--route -1|0|1] [--repeats 5] [--cli]

Sequences: NxL = the reference's 16 x 10 kb file for 16x10000 (tests/golden/hw4_input1610000.fasta), otherwise slices of
the 16 x 100 kb file (sequence k = record k % 16, bases (k // 16) L .. (k // 16 + 1) L).  --route sets PWA_SCORES_ROUTE for
the library context and the CLI (-1: leave the default, by estimated cost).  Device time: events around the batch's kernels
(pwa_batch_run_times) after one warm-up run; wall times by the host clock.  Prints one JSON line per shape."""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def read_fasta_hw4(data):
    recs, name, seq = [], None, []
    for line in data.split(b"\n"):
        if not line:
            continue
        if line.endswith(b"\r"):
            line = line[:-1]
        if line[:1] == b">":
            if name is not None:
                recs.append((name, b"".join(seq)))
            name, seq = line[1:], []
        else:
            seq.append(line)
    if name is not None:
        recs.append((name, b"".join(seq)))
    return recs


def shape_records(n, length):
    if (n, length) == (16, 10000):
        return read_fasta_hw4(open(os.path.join(GOLDEN, "hw4_input1610000.fasta"), "rb").read())
    big = read_fasta_hw4(gzip.decompress(open(os.path.join(GOLDEN, "hw4_input16100000.fasta.gz"), "rb").read()))
    out = []
    for k in range(n):
        h, s = big[k % len(big)]
        lo = (k // len(big)) * length
        assert lo + length <= len(s), "shape beyond the 100 kb file"
        out.append((b"%s_%d" % (h, k), s[lo:lo + length]))
    return out


def stats(xs):
    return dict(min=min(xs), median=statistics.median(xs), max=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", required=True, help="NxL, e.g. 16x10000")
    ap.add_argument("--route", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scoring", default="1,-1,-1")
    ap.add_argument("--cli", action="store_true", help="also time hw4_amd on the shape's FASTA")
    a = ap.parse_args()
    if a.route >= 0:
        os.environ["PWA_SCORES_ROUTE"] = str(a.route)
    import __graft_entry__ as g
    pkg = g.load_pkg()
    sc = [int(x) for x in a.scoring.split(",")]
    ctx = pkg.Context(0)
    for shape in a.shape:
        n, length = (int(x) for x in shape.lower().split("x"))
        recs = shape_records(n, length)
        seqs = [s for _, s in recs]
        pa = [i for i in range(n) for j in range(i + 1, n)]
        pb = [j for i in range(n) for j in range(i + 1, n)]
        cells = sum(len(seqs[i]) * len(seqs[j]) for i, j in zip(pa, pb))
        b = ctx.batch_distances(seqs, pa, pb, *sc)
        info = b.info()
        b.run()
        first = b.fetch()
        for _ in range(a.repeats):
            b.run()
        b.fetch()
        dev = b.run_times()[-a.repeats:]
        b.close()
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got = ctx.distances_oneshot(seqs, pa, pb, *sc)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert got == first, "pwa_distances and the batch disagree"
        row = dict(shape=shape, route=a.route, scoring=sc, kernel=info["kernel"], pairs=len(pa), cells=cells,
                   device_ms=stats(dev), pwa_distances_wall_ms=stats(wall), gcups=cells / (min(dev) * 1e-3) / 1e9)
        if a.cli:
            with tempfile.TemporaryDirectory() as td:
                with open(os.path.join(td, "in.fa"), "wb") as f:
                    for h, s in recs:
                        f.write(b">" + h + b"\n" + s + b"\n")
                cw = []
                for _ in range(min(a.repeats, 3)):
                    t0 = time.perf_counter()
                    subprocess.run([pkg.CLI4_PATH, "-i", "in.fa", "-t", "tree.txt", "-s"] + [str(x) for x in sc], cwd=td, check=True,
                                   stdout=subprocess.DEVNULL, timeout=1800)
                    cw.append((time.perf_counter() - t0) * 1e3)
                row["hw4_amd_wall_ms"] = stats(cw)
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
