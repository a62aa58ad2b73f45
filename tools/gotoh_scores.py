"""Affine-gap (gotoh) score passes next to what they replace and to the closest kernels in the tree.

Tables (one process each, forms alternated run by run, device ms: pwa_batch_last_ms / pwa_align_gotoh_last_stats; median, min, max and
spread = max / min over --reps runs after one warm-up round):
  fill    scores pass against the FILL time of pwa_align_gotoh_batch_cigar on the same list, scoring (1, -4, -6, -1), NW, SW, SG:
          g (4096 pairs 150 x 10k, tools/gotoh_batch.py's list) and reads (65 536 reads 150 x 400, each against its own region);
  affine  NW, scoring (5, -4, -16, -4): the gotoh strips against pwa_affine_batch_create on bench.py's C3 shape (4096 patterns of 150
          x 256 texts of 10k) and its hw3 shape (all pairs of 1024 sequences of 1000);
  linear  SW on the C3 shape, scoring (1, -4, -6, -1) against the linear int32 strips (gap -1) of a PWA_CELL16=0 context;
  pmc     one run of each strip kernel of `affine` on the C3 shape, for a counter collection of its own around this process.
One JSON line per (table, shape, mode, form).

    python tools/gotoh_scores.py [--reps 5] [--tables fill,affine,linear] [--out profiles/gotoh_scores.jsonl]
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
from gotoh_batch import gen_dna, mutate  # noqa: E402

GOTOH = (1, -4, -6, -1)
HW3 = (5, -4, -16, -4)


def stat(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), spread=max(xs) / min(xs) if min(xs) > 0 else None, n=len(xs))


def g_list(rng):
    texts = [gen_dna(rng, 10000) for _ in range(64)]
    pats = [mutate(rng, texts[k][at:at + 150], 0.03)[:150] for k, at in enumerate(rng.integers(0, 9850, 64))]
    return pats + [t.tobytes() for t in texts], [i % 64 for i in range(4096)], [64 + i // 64 for i in range(4096)]


def reads_list(rng):
    seqs, pa, pb = [], [], []
    for k in range(65536):
        region = gen_dna(rng, 400)
        at = int(rng.integers(0, 250))
        seqs += [mutate(rng, region[at:at + 150], 0.03)[:150], region.tobytes()]
        pa.append(2 * k)
        pb.append(2 * k + 1)
    return seqs, pa, pb


def c3_list(rng):
    texts = [gen_dna(rng, 10000) for _ in range(256)]
    pats = [mutate(rng, texts[k % 256][at:at + 150], 0.03)[:150] for k, at in enumerate(rng.integers(0, 9850, 4096))]
    seqs = pats + [t.tobytes() for t in texts]
    pa = np.repeat(np.arange(4096, dtype=np.uint32), 256)
    pb = np.tile(np.arange(4096, 4096 + 256, dtype=np.uint32), 4096)
    return seqs, pa, pb


def hw3_list(rng):
    seqs = [gen_dna(rng, 1000).tobytes() for _ in range(1024)]
    ia, ib = np.triu_indices(1024, 1)
    return seqs, ia.astype(np.uint32), ib.astype(np.uint32)


def alternate(forms, reps):
    """forms: {name: callable -> device ms}; one warm-up round, then `reps` rounds, the forms in turn"""
    ms = {k: [] for k in forms}
    for r in range(reps + 1):
        for k, f in forms.items():
            x = f()
            if r:
                ms[k].append(x)
    return {k: stat(v) for k, v in ms.items()}


def batch_form(b):
    def run():
        b.run()
        return b.last_ms()
    return run


def table_fill(ctx, emit, reps, rng):
    for shape, (seqs, pa, pb) in (("g", g_list(rng)), ("reads", reads_list(rng))):
        for mode in ("nw", "sw", "sg"):
            b = ctx.batch_gotoh(mode, seqs, pa, pb, *GOTOH)

            def fill():
                ctx.align_gotoh_batch_cigar(mode, seqs, pa, pb, *GOTOH)
                return ctx.align_gotoh_stats()["fill_ms"]
            res = alternate({"scores": batch_form(b), "align_fill": fill}, reps)
            info = b.info()
            b.close()
            for form, st in res.items():
                emit(dict(table="fill", shape=shape, mode=mode, form=form, scoring=GOTOH, pairs=len(pa), ms=st,
                          kernel=info["kernel"] if form == "scores" else "gotoh_fill_kernel", cells=info["cells"]))


def table_affine(ctx, emit, reps, rng, pmc=False):
    for shape, (seqs, pa, pb) in (("c3", c3_list(rng)),) + (() if pmc else (("hw3", hw3_list(rng)),)):
        bg = ctx.batch_gotoh("nw", seqs, pa, pb, *HW3)
        ba = ctx.batch_affine(seqs, pa, pb, *HW3)
        res = alternate({"gotoh_strips": batch_form(bg), "affine_strips": batch_form(ba)}, 1 if pmc else reps)
        for form, b in (("gotoh_strips", bg), ("affine_strips", ba)):
            info = b.info()
            emit(dict(table="pmc" if pmc else "affine", shape=shape, mode="nw", form=form, scoring=HW3, pairs=len(pa), ms=res[form],
                      kernel=info["kernel"], cells=info["cells"], padded_cells=info["padded_cells"]))
            b.close()


def table_linear(pkg, ctx, emit, reps, rng):
    seqs, pa, pb = c3_list(rng)
    os.environ["PWA_CELL16"] = "0"
    lin_ctx = pkg.Context(0)
    del os.environ["PWA_CELL16"]
    bg = ctx.batch_gotoh("sw", seqs, pa, pb, *GOTOH)
    bl = lin_ctx.batch("sw", seqs, pa, pb, 1, -4, -1)
    res = alternate({"gotoh_strips": batch_form(bg), "linear_int32_strips": batch_form(bl)}, reps)
    for form, b in (("gotoh_strips", bg), ("linear_int32_strips", bl)):
        info = b.info()
        emit(dict(table="linear", shape="c3", mode="sw", form=form, scoring=GOTOH if form == "gotoh_strips" else (1, -4, -1), pairs=len(pa),
                  ms=res[form], kernel=info["kernel"], cells=info["cells"], padded_cells=info["padded_cells"]))
        b.close()
    lin_ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tables", default="fill,affine,linear")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gotoh_scores.jsonl"))
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
    for t in a.tables.split(","):
        rng = np.random.default_rng(2026)
        if t == "fill":
            table_fill(ctx, emit, a.reps, rng)
        elif t == "affine":
            table_affine(ctx, emit, a.reps, rng)
        elif t == "pmc":
            table_affine(ctx, emit, a.reps, rng, pmc=True)
        elif t == "linear":
            table_linear(pkg, ctx, emit, a.reps, rng)
    ctx.close()


if __name__ == "__main__":
    main()
