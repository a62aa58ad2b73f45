"""Substitution-matrix batch alignments and scores next to the byte-compare gotoh calls on the same inputs.

The yardstick is pwa_align_gotoh_batch_cigar / the band-less gotoh scores at (1, -4, -6, -1); the matrix form gets the equivalent
4-code match / mismatch table, so both compute the same alignments.  Same process, the two forms alternated call by call; device ms
(pwa_align_subst_last_stats / pwa_align_gotoh_last_stats, pwa_batch_last_ms): median, min, max and spread = max / min over --reps
rounds after one warm-up round.
  g        4096 pairs 150 x 10k (tools/gotoh_batch.py's list): NW, SW, SG;
  reads    65 536 reads 150 x 400, SG;
  wide     1024 pairs 1000 x 10k (one pair per wave), NW;
  protein  the g shape over a random 20-symbol alphabet, NW: the matrix form under a random asymmetric matrix (the gather spreads over
           the table), the byte-compare form on the same bytes;
  pmc_subst | pmc_gotoh   one fill + walk of one form on g, NW, for a counter collection of its own around this process.
The scores rows run want_end = True, which puts the gotoh list on its band-less mini form too (pwa_gotoh_batch_create's rule).
One JSON line per (shape, mode, pass, form), appended to --out.

    python tools/subst_batch.py [--reps 5] [--shapes g,reads,wide,protein] [--out profiles/subst_batch.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as G  # noqa: E402
from gotoh_batch import mutate  # noqa: E402

GOTOH = (1, -4, -6, -1)
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"


def stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), spread=max(xs) / min(xs) if min(xs) > 0 else None, n=len(xs))


def gen(rng, n, alpha):
    return rng.choice(np.frombuffer(alpha, np.uint8), n)


def mutate_in(rng, s, rate, alpha):
    """gotoh_batch.mutate draws its new symbols from ACGT: map them onto `alpha`'s first four (the rates are what matters)"""
    out = np.frombuffer(mutate(rng, s, rate), np.uint8).copy()
    for k, v in enumerate(b"ACGT"):
        if v not in alpha:
            out[out == v] = alpha[k]
    return out.tobytes()


def g_list(rng, alpha=b"ACGT"):
    texts = [gen(rng, 10000, alpha) for _ in range(64)]
    pats = [mutate_in(rng, texts[k][at:at + 150], 0.03, alpha)[:150] for k, at in enumerate(rng.integers(0, 9850, 64))]
    return pats + [t.tobytes() for t in texts], [i % 64 for i in range(4096)], [64 + i // 64 for i in range(4096)]


def reads_list(rng):
    seqs, pa, pb = [], [], []
    for k in range(65536):
        region = gen(rng, 400, b"ACGT")
        at = int(rng.integers(0, 250))
        seqs += [mutate(rng, region[at:at + 150], 0.03)[:150], region.tobytes()]
        pa.append(2 * k)
        pb.append(2 * k + 1)
    return seqs, pa, pb


def wide_list(rng):
    seqs, pa, pb = [], [], []
    for k in range(1024):
        t = gen(rng, 10000, b"ACGT")
        at = int(rng.integers(0, 9000))
        seqs += [mutate(rng, t[at:at + 1000], 0.03)[:1000], t.tobytes()]
        pa.append(2 * k)
        pb.append(2 * k + 1)
    return seqs, pa, pb


def alternate(forms, reps):
    """forms: {name: callable -> dict of device ms}; one warm-up round, then `reps` rounds, the forms in turn"""
    ms = {k: {} for k in forms}
    for r in range(reps + 1):
        for k, f in forms.items():
            x = f()
            if r:
                for what, v in x.items():
                    ms[k].setdefault(what, []).append(v)
    return {k: {what: stat(v) for what, v in d.items()} for k, d in ms.items()}


def measure(pkg, ctx, emit, shape, mode, seqs, pa, pb, table, reps, scores=True):
    go, ge = GOTOH[2:]
    packed = pkg.pack_sequences(seqs)

    def subst_align():
        ctx.align_subst_batch_cigar(mode, packed, pa, pb, table, go, ge)
        st = ctx.align_subst_stats()
        return dict(fill=st["fill_ms"], walk=st["walk_ms"])

    def gotoh_align():
        ctx.align_gotoh_batch_cigar(mode, packed, pa, pb, *GOTOH)
        st = ctx.align_gotoh_stats()
        return dict(fill=st["fill_ms"], walk=st["walk_ms"])
    res = alternate({"subst": subst_align, "gotoh": gotoh_align}, reps)
    for what in ("fill", "walk"):
        s, g = res["subst"][what], res["gotoh"][what]
        emit(dict(shape=shape, mode=mode, **{"pass": what}, pairs=len(pa), n_sym=table[1], subst_ms=s, gotoh_ms=g, ratio=s["median"] / g["median"]))
    if not scores:
        return
    bs = ctx.batch_subst(mode, packed, pa, pb, table, go, ge, True)
    bg = ctx.batch_gotoh(mode, packed, pa, pb, *GOTOH, True)

    def run(b):
        def f():
            b.run()
            return dict(scores=b.last_ms())
        return f
    res = alternate({"subst": run(bs), "gotoh": run(bg)}, reps)
    s, g = res["subst"]["scores"], res["gotoh"]["scores"]
    emit(dict(shape=shape, mode=mode, **{"pass": "scores"}, pairs=len(pa), n_sym=table[1], subst_ms=s, gotoh_ms=g, ratio=s["median"] / g["median"],
              subst_kernel=bs.info()["kernel"], gotoh_kernel=bg.info()["kernel"], padded_cells=bs.info()["padded_cells"]))
    bs.close()
    bg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="g,reads,wide,protein")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subst_batch.jsonl"))
    a = ap.parse_args()
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    out = open(a.out, "a") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    dna = pkg.subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), GOTOH[0], GOTOH[1]))
    for shape in a.shapes.split(","):
        rng = np.random.default_rng(2026)
        if shape == "g":
            seqs, pa, pb = g_list(rng)
            for mode in ("nw", "sw", "sg"):
                measure(pkg, ctx, emit, shape, mode, seqs, pa, pb, dna, a.reps)
        elif shape == "reads":
            measure(pkg, ctx, emit, shape, "sg", *reads_list(rng), dna, a.reps)
        elif shape == "wide":
            measure(pkg, ctx, emit, shape, "nw", *wide_list(rng), dna, a.reps)
        elif shape == "protein":
            m = rng.integers(-9, 12, size=(20, 20))
            m[np.arange(20), np.arange(20)] = rng.integers(1, 12, size=20)
            measure(pkg, ctx, emit, shape, "nw", *g_list(rng, PROTEIN), pkg.subst_table(PROTEIN, m), a.reps)
        elif shape in ("pmc_subst", "pmc_gotoh"):
            seqs, pa, pb = g_list(rng)
            if shape == "pmc_subst":
                ctx.align_subst_batch_cigar("nw", seqs, pa, pb, dna, *GOTOH[2:])
                st = ctx.align_subst_stats()
            else:
                ctx.align_gotoh_batch_cigar("nw", seqs, pa, pb, *GOTOH)
                st = ctx.align_gotoh_stats()
            emit(dict(shape=shape, mode="nw", pairs=len(pa), padded_cells=4096 * 160 * 10000, **st))
    ctx.close()


if __name__ == "__main__":
    main()
