#!/usr/bin/env python3
"""Fixtures for hw3's score pass on few long sequences (the stripe engine's affine kernel) from the UNMODIFIED hw3.cpp
(oracle/_ref).  Dev container only.  Reuses the reference's own long inputs, committed for hw4 (byte-identical to
Multiple_Sequence_Alignment/input1610000.fasta and input16100000.fasta):

  hw3_long.json   affine scores of all 120 pairs of the 10 kb file for two scorings (and the center hw3 picks from them), the
                  output.phy bytes the reference writes for that file (~67 s, ~2.4 GB), the reference's scores of 20 000-base
                  prefixes of a few pairs of the 100 kb file (~9.6 GB of matrices each: one at a time), and the oracle's scores
                  (orc3_affine_score, O(m) memory, pinned to the reference on the inputs above) of 40 kb prefixes and full 100 kb
                  pairs, which the reference cannot hold.
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

SMALL = "hw4_input1610000.fasta"
BIG = "hw4_input16100000.fasta.gz"
SCORINGS = [(5, -4, -16, -4), (2, -3, -5, -2)]   # README's, and a second one
PREFIX = 20000
PREFIX_PAIRS = [(0, 1, SCORINGS[0]), (2, 9, SCORINGS[1]), (5, 15, SCORINGS[0]), (3, 4, SCORINGS[1]), (7, 12, (1, 3, 2, 1))]
ORACLE_PREFIX = 40000
ORACLE_PREFIX_PAIRS = [(0, 1, SCORINGS[0]), (6, 11, SCORINGS[1]), (13, 14, (1, 3, 2, 1))]
ORACLE_FULL_PAIRS = [(0, 1, SCORINGS[0]), (4, 10, SCORINGS[0]), (8, 15, SCORINGS[0])]   # the scoring of the 16 x 100 kb test


def key(sc):
    return "%d,%d,%d,%d" % sc


def main():
    assert O.have_ref3()
    small = [s for _, s in O.read_fasta_hw3(os.path.join(HERE, SMALL))]
    n = len(small)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]   # hw3.cpp:233-234: string1 = i, string2 = j
    out = {"file": SMALL, "pairs": pairs, "scores": {}, "center": {}}
    with ThreadPoolExecutor(4) as ex:   # ~2.4 GB of matrices per 10 kb pair
        for sc in SCORINGS:
            got = list(ex.map(lambda p: O.ref_affine_score(small[p[0]], small[p[1]], *sc), pairs))
            out["scores"][key(sc)] = got
            out["center"][key(sc)] = O.center(got, n)[0]
            print("10 kb", sc, "done", flush=True)
    with tempfile.TemporaryDirectory() as td:
        shutil.copyfile(os.path.join(HERE, SMALL), os.path.join(td, "in.fa"))
        sc = SCORINGS[0]
        subprocess.run([O.REF3_CLI, "-i", "in.fa", "-o", "output.phy", "-s", ":".join(str(x) for x in sc)], cwd=td, check=True,
                       stdout=subprocess.DEVNULL)
        out["phy"] = {"scoring": list(sc), "output": open(os.path.join(td, "output.phy"), "rb").read().decode("latin-1")}
    print("output.phy done", flush=True)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "big.fa")
        open(path, "wb").write(gzip.decompress(open(os.path.join(HERE, BIG), "rb").read()))
        big = [s for _, s in O.read_fasta_hw3(path)]
    recs = []
    for a, b, sc in PREFIX_PAIRS:   # one at a time: ~9.6 GB each
        v = O.ref_affine_score(big[a][:PREFIX], big[b][:PREFIX], *sc)
        assert v == O.affine_score(big[a][:PREFIX], big[b][:PREFIX], *sc), (a, b, sc)   # the oracle below is pinned here
        recs.append(dict(a=a, b=b, scoring=list(sc), score=v))
        print("prefix", a, b, "done", flush=True)
    out["prefix"] = {"file": BIG, "length": PREFIX, "pairs": recs}
    with ThreadPoolExecutor(3) as ex:
        op = list(ex.map(lambda p: O.affine_score(big[p[0]][:ORACLE_PREFIX], big[p[1]][:ORACLE_PREFIX], *p[2]), ORACLE_PREFIX_PAIRS))
        of = list(ex.map(lambda p: O.affine_score(big[p[0]], big[p[1]], *p[2]), ORACLE_FULL_PAIRS))
    out["oracle_prefix"] = {"file": BIG, "length": ORACLE_PREFIX,
                            "pairs": [dict(a=a, b=b, scoring=list(sc), score=v) for (a, b, sc), v in zip(ORACLE_PREFIX_PAIRS, op)]}
    out["oracle_full"] = {"file": BIG, "pairs": [dict(a=a, b=b, scoring=list(sc), score=v) for (a, b, sc), v in zip(ORACLE_FULL_PAIRS, of)]}
    json.dump(out, open(os.path.join(HERE, "hw3_long.json"), "w"), indent=0)
    print("hw3_long.json", os.path.getsize(os.path.join(HERE, "hw3_long.json")))


if __name__ == "__main__":
    main()
