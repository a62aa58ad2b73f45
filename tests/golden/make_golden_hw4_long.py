#!/usr/bin/env python3
"""Fixtures for hw4 on few long sequences (the stripe engine's distance kernel) from the UNMODIFIED hw4.cpp
(oracle/_ref).  Dev container only; the reference's matrices take ~500 MB per 10 kb pair and ~8 GB per 40 kb pair.

  hw4_input1610000.fasta      the reference's own 16 x 10 kb input (Multiple_Sequence_Alignment/input1610000.fasta)
  hw4_input16100000.fasta.gz  the reference's own 16 x 100 kb input, gzipped
  hw4_long.json               distances of all 120 pairs of the 10 kb file for two scorings, the tree bytes hw4 writes for
                              that file, and the distances of 40 000-base prefixes of a few pairs of the 100 kb file
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402

REF = "/root/reference/Multiple_Sequence_Alignment"
SCORINGS = [(1, -1, -1), (5, -4, -4)]
PREFIX = 40000
PREFIX_PAIRS = [(0, 1, (1, -1, -1)), (2, 9, (1, -1, -1)), (5, 15, (5, -4, -4)), (3, 4, (2, -3, -5))]


def read_fasta(data):
    """hw4.cpp:109-134: '>' starts a record, every other non-empty line (one trailing CR dropped) is appended."""
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


def main():
    assert O.have_ref4()
    shutil.copyfile(os.path.join(REF, "input1610000.fasta"), os.path.join(HERE, "hw4_input1610000.fasta"))
    with open(os.path.join(REF, "input16100000.fasta"), "rb") as f:
        open(os.path.join(HERE, "hw4_input16100000.fasta.gz"), "wb").write(gzip.compress(f.read(), 9, mtime=0))
    seqs = [s for _, s in read_fasta(open(os.path.join(REF, "input1610000.fasta"), "rb").read())]
    n = len(seqs)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]   # hw4.cpp:138-140: sequence1 = i, sequence2 = j
    out = {"file": "hw4_input1610000.fasta", "pairs": pairs, "dist": {}}
    with ThreadPoolExecutor(4) as ex:
        for sc in SCORINGS:
            out["dist"]["%d,%d,%d" % sc] = list(ex.map(lambda p: O.ref_nw_distance(seqs[p[0]], seqs[p[1]], *sc), pairs))
            print("10 kb", sc, "done", flush=True)
    with tempfile.TemporaryDirectory() as td:
        shutil.copyfile(os.path.join(REF, "input1610000.fasta"), os.path.join(td, "in.fa"))
        trees = {}
        for sc in SCORINGS:
            subprocess.run([O.REF4_CLI, "-i", "in.fa", "-t", "tree.txt", "-s"] + [str(x) for x in sc], cwd=td, check=True,
                           stdout=subprocess.DEVNULL)
            trees["%d,%d,%d" % sc] = open(os.path.join(td, "tree.txt"), "rb").read().decode("latin-1")
        out["tree"] = trees
    big = [s for _, s in read_fasta(open(os.path.join(REF, "input16100000.fasta"), "rb").read())]
    with ThreadPoolExecutor(2) as ex:
        dists = list(ex.map(lambda p: O.ref_nw_distance(big[p[0]][:PREFIX], big[p[1]][:PREFIX], *p[2]), PREFIX_PAIRS))
    out["prefix"] = {"file": "hw4_input16100000.fasta.gz", "length": PREFIX,
                     "pairs": [dict(a=a, b=b, scoring=list(sc), dist=d) for (a, b, sc), d in zip(PREFIX_PAIRS, dists)]}
    json.dump(out, open(os.path.join(HERE, "hw4_long.json"), "w"), indent=0)
    print("hw4_long.json", os.path.getsize(os.path.join(HERE, "hw4_long.json")))


if __name__ == "__main__":
    main()
