#!/usr/bin/env python3
"""Fixtures for the differential oracle tests (tests/test_oracle.py, test_oracle_hw3.py, test_oracle_hw4.py): the same seeded
random inputs those tests draw, with what the UNMODIFIED hw2.cpp / hw3.cpp / hw4.cpp functions return for them (oracle/_ref,
built by `make -C oracle ref`).  Dev container only; the tests read differential.json.gz and need no compiled reference."""
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402

HW2_FIELDS = ("score", "aligned_pattern", "aligned_reference", "cigar", "mdz", "overlap")


def L(b):
    return b.decode("latin-1")


def hw2():
    rng = random.Random(2025)
    scorings = [(1, -1, -1), (2, -3, -5), (5, -4, -4), (1, -3, -1), (0, 0, 0), (1, 1, 1), (-1, 2, 1), (3, -1, 2)]
    out = []
    for it in range(1500):
        alpha = rng.choice([b"ACGT", b"AC", b"ACGTN"])
        p = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 60)))
        t = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 60)))
        sc = rng.choice(scorings)
        rec = dict(p=L(p), t=L(t), scoring=list(sc))
        for mode in ("nw", "sw"):
            r = O.ref_align(mode, p, t, *sc)
            rec[mode] = {k: (L(r[k]) if isinstance(r[k], bytes) else r[k]) for k in HW2_FIELDS}
        out.append(rec)
    return out


def hw3_scores():
    rng = random.Random(8)
    out = []
    for it in range(1500):
        a = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 50)))
        b = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 50)))
        sc = rng.choice([(5, -4, -16, -4), (1, -1, -2, -1), (1, 1, 1, 1), (0, 0, 0, 0), (4, -5, 2, -1), (2, -1, -3, 1)])
        out.append(dict(a=L(a), b=L(b), scoring=list(sc), score=O.ref_affine_score(a, b, *sc)))
    return out


def hw3_alignments():
    rng = random.Random(18)
    out = []
    for it in range(600):
        alpha = rng.choice([b"AC", b"ACGT", b"ACDEFGHIKLMNPQRSTVWY"])
        a = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 45)))
        b = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 45)))
        sc = rng.choice([(5, -4, -16, -4), (1, -1, -2, -1), (1, -1, 0, -1), (0, 0, 0, 0), (2, -1, -3, 1), (1, 1, 1, 1)])
        r = O.ref_affine_align(a, b, *sc)
        out.append(dict(a=L(a), b=L(b), scoring=list(sc), score=r["score"], a1=L(r["a1"]), a2=L(r["a2"])))
    return out


def hw4():
    rng = random.Random(44)
    out = []
    for it in range(1500):
        a = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 50)))
        b = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 50)))
        sc = rng.choice([(1, -1, -1), (2, -3, -5), (1, 1, 1), (0, 0, 0), (-1, 2, 1), (1, -1, 0)])
        out.append(dict(a=L(a), b=L(b), scoring=list(sc), dist=O.ref_nw_distance(a, b, *sc)))
    return out


def main():
    assert O.have_ref() and O.have_ref3() and O.have_ref4(), "run `make -C oracle ref` first (needs the reference source)"
    out = {"hw2": hw2(), "hw3_scores": hw3_scores(), "hw3_alignments": hw3_alignments(), "hw4": hw4()}
    path = os.path.join(HERE, "differential.json.gz")
    with open(path, "wb") as f:   # gzip without a timestamp: a rerun writes the same bytes
        f.write(gzip.compress(json.dumps(out, separators=(",", ":")).encode(), 9, mtime=0))
    print("differential.json.gz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
