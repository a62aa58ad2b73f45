#!/usr/bin/env python3
"""Fixtures for hw3's alignments of long pairs (the stripe engine's affine traceback fill and walk) from the UNMODIFIED hw3.cpp
(oracle/_ref).  Dev container only; one pair at a time (the reference holds six full matrices: ~2.4 GB at 10 kb, ~9.6 GB at 20 kb).

  hw3_align_long.json   per pair: score, number of alignment columns and the sha256 of the op list in traceback order
                        ('M' / 'D' / 'I', as pwa_align_affine_batch writes it), for
                        - the 15 alignments hw3 builds against the center of the 10 kb file with the README scoring
                          (hw3.cpp:261-283: string1 = the center, string2 = the other sequence);
                        - the 20 000-base prefix pairs of the 100 kb file that hw3_long.json scores (make_golden_hw3_long.py).
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracle_lib as O  # noqa: E402
from make_golden_hw3_long import BIG, PREFIX, PREFIX_PAIRS, SMALL, key  # noqa: E402

README = (5, -4, -16, -4)


def ops_of(a1, a2):
    """The reference's two aligned strings -> op list in traceback order."""
    out = bytearray()
    for x, y in zip(a1, a2):
        out.append(ord("D") if y == ord("-") else ord("I") if x == ord("-") else ord("M"))
    return bytes(reversed(out))


def record(s1, s2, sc):
    r = O.ref_affine_align(s1, s2, *sc)
    ops = ops_of(r["a1"], r["a2"])
    assert r["a1"].replace(b"-", b"") == s1 and r["a2"].replace(b"-", b"") == s2
    return dict(score=r["score"], n_ops=len(ops), sha256=hashlib.sha256(ops).hexdigest())


def main():
    assert O.have_ref3()
    small = [s for _, s in O.read_fasta_hw3(os.path.join(HERE, SMALL))]
    c = json.load(open(os.path.join(HERE, "hw3_long.json")))["center"][key(README)]
    center = []
    for j in range(len(small)):
        if j != c:
            center.append(dict(a=c, b=j, **record(small[c], small[j], README)))
            print("10 kb", c, j, "done", flush=True)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "big.fa")
        open(path, "wb").write(gzip.decompress(open(os.path.join(HERE, BIG), "rb").read()))
        big = [s for _, s in O.read_fasta_hw3(path)]
    prefix = []
    for a, b, sc in PREFIX_PAIRS:
        prefix.append(dict(a=a, b=b, scoring=list(sc), **record(big[a][:PREFIX], big[b][:PREFIX], sc)))
        print("prefix", a, b, "done", flush=True)
    out = {"center_pairs": {"file": SMALL, "scoring": list(README), "center": c, "pairs": center},
           "prefix": {"file": BIG, "length": PREFIX, "pairs": prefix}}
    json.dump(out, open(os.path.join(HERE, "hw3_align_long.json"), "w"), indent=0)
    print("hw3_align_long.json", os.path.getsize(os.path.join(HERE, "hw3_align_long.json")))


if __name__ == "__main__":
    main()
