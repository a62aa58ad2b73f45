#!/usr/bin/env python3
"""hw1_amd at scale: seeded genomes (tests/hw1_gen.py) of 1 / 16 / 100 Mb with 10k .. 1M reads; per input the wall time of
the whole CLI process (min of --repeat runs) and the PWA_DEBUG phase lines of the fastest run (library: SA rounds, device
build ms, occurrences call; CLI: read, text, context, suffix array, search, occurrences, write).  One JSON line per input.

    python3 tools/hw1_scale.py [--sizes 1,16,100] [--reads 10000,100000,1000000] [--repeat 3] [--out FILE.jsonl]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hw1_gen as G  # noqa: E402

CLI = os.path.join(ROOT, "bioinformatics-algorithms_amd", "host", "hw1_amd")
HBM_BPS = 8.0e12   # MI355X HBM3E peak (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,100", help="Mb of reference text")
    ap.add_argument("--reads", default="10000,100000,1000000")
    ap.add_argument("--refs", type=int, default=24)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    with tempfile.TemporaryDirectory() as td:
        for mb in [int(x) for x in a.sizes.split(",")]:
            n_refs = 1 if mb == 1 else a.refs
            refs = G.genome(16, mb * 1_000_000, n_refs)
            open(os.path.join(td, "ref.fa"), "wb").write(G.fasta(refs))
            for n_reads in [int(x) for x in a.reads.split(",")]:
                open(os.path.join(td, "pat.fa"), "wb").write(G.fasta(G.reads(17, refs, n_reads)))
                best = None
                for _ in range(a.repeat):
                    t0 = time.time()
                    pr = subprocess.run([CLI, "-r", "ref.fa", "-p", "pat.fa", "-o", "out"], cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                        timeout=a.timeout, env=dict(os.environ, PWA_DEBUG="1"))
                    wall = time.time() - t0
                    if pr.returncode != 0:
                        sys.exit("hw1_amd failed (%d): %s" % (pr.returncode, pr.stderr.decode()[-2000:]))
                    if best is None or wall < best[0]:
                        best = (wall, pr.stderr.decode())
                wall, err = best
                phases = {m.group(1): float(m.group(2)) for m in re.finditer(r"^\[hw1_amd\] ([A-Za-z .()+]+?) +([0-9.]+) ms$", err, re.M)}
                rec = dict(mb=mb, n_refs=n_refs, reads=n_reads, text_bytes=sum(len(s) + 1 for _, s in refs), wall_s=round(wall, 3),
                           phases_ms=phases)
                m = re.search(r"sa build: n=(\d+) sigma=(\d+) codes/key=(\d+) rounds=(\d+) passes=(\d+) device ([0-9.]+) ms", err)
                if m:
                    n, passes, ms = int(m.group(1)), int(m.group(5)), float(m.group(6))
                    # bytes a pass moves at least: read keys for the histogram, read + write (key, index) in the scatter = 32 B per element
                    rec.update(rounds=int(m.group(4)), passes=passes, sa_device_ms=ms, sa_bytes_per_s=n / (ms * 1e-3),
                               sort_traffic_frac_of_hbm=32.0 * n * passes / (ms * 1e-3) / HBM_BPS)
                m = re.search(r"sa occurrences: .*? ([0-9]+) hits kept, ([0-9.]+) ms", err)
                if m:
                    rec.update(hits=int(m.group(1)), occurrences_ms=float(m.group(2)))
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")


if __name__ == "__main__":
    main()
