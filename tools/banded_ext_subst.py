"""Banded X-drop extension under a substitution matrix (pwa_scores_extend_banded_subst, pwa_extend_banded_subst_batch_cigar),
DESIGN.md §3.17.  The table is ACGT with match 1 / mismatch -4 plus a neutral N (row and column 0); gaps (-6, -1).

Shapes: tools/banded_ext.py's three, generated the same way.
  stop    4096 pairs 10 000 x 10 000 at half-width 128; text rows 1..2000 are a copy of the pattern at ~3 % divergence, the rest is
          unrelated random DNA; xdrop = 100.  The sweep ends in stripe 9 of 40 (256-row stripes).
  nostop  the same shape with the whole text related, xdrop = -1: the cost of the table cell with nothing saved.
  seeded  65 536 reads 1500 x 4000 (64 shared texts), as extension from a seed at (0, 0) of the region cut out at the read's diagonal:
          band +- 100, xdrop = 100.
Yardsticks, on the same pairs and bands, in the same child: the byte-compare EXT calls (scores_extend_banded for the score pass,
extend_banded_batch_cigar for the fill and the walk) -- the ratio table / byte-compare is the cost of the policy swap --, and the SW
table calls (scores_banded_subst("sw"), align_banded_subst_batch_cigar("sw")).  Per form: device ms (median of --reps after one
warm-up call) of the score pass, the fill and the walk, the ratios, the mean `rows` and the share of pairs with a pattern end.

Checked in every shape: the scores call equals the alignment call on score, end, rows and pend; and, the sequences holding no N, the
table calls equal the byte-compare calls on score, end and rows.
Condition (shape `stop`): the table EXT score pass takes at most 0.5 x the SW table score pass, and the table EXT fill at most 0.5 x
the SW table fill; the child -- and the tool -- end with status 3 if a check or the condition fails.

One GPU process at a time: the parent never touches the GPU; it runs every shape in a child of its own under a time limit, one after
the other, stops at the first that fails, and appends the children's JSON lines to profiles/banded_ext_subst.jsonl.

    python tools/banded_ext_subst.py [--reps 3] [--shapes stop,nostop,seeded] [--limit 420]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from banded_batch import fit, gen_dna, mutate  # noqa: E402
from banded_ext import SC, timed  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "banded_ext_subst.jsonl")


def run_shape(shape, reps):
    import __graft_entry__ as G
    pkg = G.load_pkg()
    ctx = pkg.Context(0)
    m = np.where(np.eye(5, dtype=bool), SC[0], SC[1])
    m[4, :] = m[:, 4] = 0
    table, go, ge = pkg.subst_table(b"ACGTN", m, unknown=4), SC[2], SC[3]
    rng = np.random.default_rng(2027)
    if shape in ("stop", "nostop"):
        n, count, w, xdrop = 10000, 4096, 128, (100 if shape == "stop" else -1)
        seqs = []
        for k in range(count):
            p = gen_dna(rng, n)
            t = fit(rng, mutate(rng, p, 0.03), n) if shape == "nostop" else fit(rng, mutate(rng, p[:2000], 0.03)[:2000], n)
            seqs += [p.tobytes(), t]
        pa, pb = list(range(0, 2 * count, 2)), list(range(1, 2 * count, 2))
        bands = [(-w, w)] * count
    else:
        xdrop = 100
        texts = [gen_dna(rng, 6400) for _ in range(64)]
        seqs, pa, pb = [], [], []
        for k in range(65536):
            d = int(rng.integers(0, 2400))
            seqs += [fit(rng, mutate(rng, texts[k % 64][d:d + 1500], 0.03), 1500), texts[k % 64][d:d + 4000].tobytes()]   # the region from the seed on
            pa.append(2 * k)
            pb.append(2 * k + 1)
        bands = [(-100, 100)] * 65536
    seqs = pkg.pack_sequences(seqs)
    sw_s, t_sw_s = timed(reps, lambda: ctx.scores_banded_subst("sw", seqs, pa, pb, table, go, ge, bands, want_end=True), ctx.scores_banded_stats)
    by_s, t_by_s = timed(reps, lambda: ctx.scores_extend_banded(seqs, pa, pb, *SC, bands, xdrop, want_end=True), ctx.extend_banded_stats)
    ex_s, t_ex_s = timed(reps, lambda: ctx.scores_extend_banded_subst(seqs, pa, pb, table, go, ge, bands, xdrop, want_end=True), ctx.extend_banded_stats)
    sw_a, t_sw_a = timed(reps, lambda: ctx.align_banded_subst_batch_cigar("sw", seqs, pa, pb, table, go, ge, bands), ctx.align_banded_stats)
    by_a, t_by_a = timed(reps, lambda: ctx.extend_banded_batch_cigar(seqs, pa, pb, *SC, bands, xdrop), ctx.extend_banded_stats)
    ex_a, t_ex_a = timed(reps, lambda: ctx.extend_banded_subst_batch_cigar(seqs, pa, pb, table, go, ge, bands, xdrop), ctx.extend_banded_stats)
    ctx.close()
    equal = [(x["score"], x["end"], x["rows"], x["pend"]) for x in ex_a] == list(zip(ex_s[0], zip(ex_s[1], ex_s[2]), ex_s[3], ex_s[4]))
    same = tuple(ex_s[:4]) == tuple(by_s) and [(x["score"], x["end"], x["rows"], x["cigar"], x["mdz"]) for x in ex_a] == \
        [(x["score"], x["end"], x["rows"], x["cigar"], x["mdz"]) for x in by_a]
    row = dict(shape=shape, scoring=SC, table="ACGT match / mismatch + neutral N", pairs=len(pa), xdrop=xdrop, half_width=bands[0][1],
               mean_rows=float(np.mean(ex_s[3])), pattern_end_share=float(np.mean([x is not None for x in ex_s[4]])),
               mean_score_ext=float(np.mean(ex_s[0])), mean_score_sw=float(np.mean(sw_s[0])),
               sw_subst_scores_ms=t_sw_s["fill_ms"], ext_scores_ms=t_by_s["fill_ms"], ext_subst_scores_ms=t_ex_s["fill_ms"],
               scores_ratio_table_over_bytes=t_ex_s["fill_ms"] / t_by_s["fill_ms"], scores_ratio_ext_over_sw=t_ex_s["fill_ms"] / t_sw_s["fill_ms"],
               sw_subst_fill_ms=t_sw_a["fill_ms"], ext_fill_ms=t_by_a["fill_ms"], ext_subst_fill_ms=t_ex_a["fill_ms"],
               fill_ratio_table_over_bytes=t_ex_a["fill_ms"] / t_by_a["fill_ms"], fill_ratio_ext_over_sw=t_ex_a["fill_ms"] / t_sw_a["fill_ms"],
               sw_subst_walk_ms=t_sw_a["walk_ms"], ext_walk_ms=t_by_a["walk_ms"], ext_subst_walk_ms=t_ex_a["walk_ms"],
               scores_equal_alignments=equal, table_equals_byte_compare=same, reps=reps)
    print(json.dumps(row), flush=True)
    ok = equal and same
    if shape == "stop":
        holds = row["scores_ratio_ext_over_sw"] <= 0.5 and row["fill_ratio_ext_over_sw"] <= 0.5
        print(json.dumps(dict(shape=shape, verdict="table EXT score pass <= 0.5 x SW table score pass and table EXT fill <= 0.5 x SW table fill (device ms)",
                              holds=holds, scores_ratio=row["scores_ratio_ext_over_sw"], fill_ratio=row["fill_ratio_ext_over_sw"],
                              mean_rows=row["mean_rows"])), flush=True)
        ok = ok and holds
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="stop,nostop,seeded")
    ap.add_argument("--limit", type=int, default=420, help="seconds per shape")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_shape(a.child, a.reps)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        with open(OUT, "a") as f:
            for x in r.stdout.splitlines():
                if x.startswith("{"):
                    f.write(x + "\n")
                    print(x, flush=True)
        if r.returncode != 0:
            print("shape %s ended with status %d: stopping" % (shape, r.returncode), file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
