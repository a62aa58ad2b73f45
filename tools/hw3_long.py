#!/usr/bin/env python3
"""hw3's all-pairs affine scores on few long sequences: device time of the score pass, wall time of pwa_scores_affine and of the
hw3-compatible CLI ("hw3 on few long sequences").

    python tools/hw3_long.py --shape 16x10000 [--shape 16x100000 ...] [--route -1|0|1] [--repeats 5] [--cli]

Sequences: NxL = the reference's 16 x 10 kb file for 16x10000 (tests/golden/hw4_input1610000.fasta, byte-identical to hw3's
input1610000.fasta), otherwise slices of the 16 x 100 kb file (sequence k = record k % 16, bases (k // 16) L .. (k // 16 + 1) L).
--route sets PWA_SCORES_ROUTE for the library context and the CLI (-1: leave the default, by estimated cost).  Device time:
events around the batch's kernels (pwa_batch_run_times) after one warm-up run; wall times by the host clock.  --cli also times
hw3_amd on the shape's FASTA, and its second phase on its own (the N-1 alignments against the center, pwa_align_affine_batch).
GCUPS counts real cells (sum of n * m).  Prints one JSON line per shape."""
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


def read_fasta(data):
    """hw3.cpp:137-167: '>' starts a record, whitespace inside sequence lines is dropped."""
    recs, name, seq = [], None, []
    for line in data.split(b"\n"):
        if not line:
            continue
        if line[:1] == b">":
            if name is not None:
                recs.append((name, b"".join(seq)))
            name, seq = line[1:], []
        else:
            seq.append(bytes(c for c in line if c not in b" \t\n\v\f\r"))
    if name is not None:
        recs.append((name, b"".join(seq)))
    return recs


def shape_records(n, length):
    if (n, length) == (16, 10000):
        return read_fasta(open(os.path.join(GOLDEN, "hw4_input1610000.fasta"), "rb").read())
    big = read_fasta(gzip.decompress(open(os.path.join(GOLDEN, "hw4_input16100000.fasta.gz"), "rb").read()))
    if (n, length) == (16, 100000):
        return big
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
    ap.add_argument("--scoring", default="5,-4,-16,-4")
    ap.add_argument("--cli", action="store_true", help="also time hw3_amd on the shape's FASTA")
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
        b = ctx.batch_affine(seqs, pa, pb, *sc)
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
            got = ctx.scores_affine_oneshot(seqs, pa, pb, *sc)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert got == first, "pwa_scores_affine and the batch disagree"
        row = dict(shape=shape, route=a.route, scoring=sc, kernel=info["kernel"], pairs=len(pa), cells=cells,
                   device_ms=stats(dev), pwa_scores_affine_wall_ms=stats(wall), gcups=cells / (min(dev) * 1e-3) / 1e9)
        if a.cli:
            with tempfile.TemporaryDirectory() as td:
                with open(os.path.join(td, "in.fa"), "wb") as f:
                    for h, s in recs:
                        f.write(b">" + h + b"\n" + s + b"\n")
                t0 = time.perf_counter()
                pr = subprocess.run([pkg.HW3_CLI_PATH, "-i", "in.fa", "-o", "out.phy", "-s", ":".join(str(x) for x in sc)], cwd=td,
                                    stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1800)
                row["hw3_amd_wall_ms"] = (time.perf_counter() - t0) * 1e3
                row["hw3_amd_rc"] = pr.returncode
                if pr.returncode:
                    row["hw3_amd_stderr"] = pr.stderr.decode("latin-1")[-400:]
            # hw3_amd's second phase on its own: the N-1 alignments against the center (pwa_align_affine_batch, untouched here)
            star = [0] * n   # hw3.cpp:232-251: star scores, the first strict maximum
            for i, j, v in zip(pa, pb, first):
                star[i] += v
                star[j] += v
            c = max(range(n), key=lambda k: (star[k], -k))
            others = [k for k in range(n) if k != c]
            t0 = time.perf_counter()
            try:
                ctx.align_affine_batch(seqs, [c] * len(others), others, *sc)
                row["align_phase_wall_ms"] = (time.perf_counter() - t0) * 1e3
            except Exception as e:   # (16 x 100 kb: the traceback codes of one wave task exceed free HBM)
                row["align_phase_error"] = str(e)[:300]
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
