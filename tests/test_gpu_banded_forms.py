"""The banded forms against each other on one context: the twelve banded calls -- op lists, strings and scores, each over byte
compares, under a table, as an extension and as an extension under a table -- share one launcher and its per-kernel dynamic-LDS
attribute.  One list of three pairs holds both stripe heights; every call is made twice, the second time in reverse order and with
the wide pair in front, and has to return what it returned the first time, which is what the numpy oracles say."""
import random

import pytest

import banded_ext_oracle as XO
import banded_oracle as BO
from test_gpu_banded_ext import SC, _seqs
from test_gpu_banded_subst import _table
from test_gpu_cigar import fmt
from test_gpu_gotoh import _mutate, _rand

pytestmark = pytest.mark.gpu

XDROP = 20
SHAPES = [(300, 310), (70, 65), (600, 580)]    # two 256-row stripes; a single stripe; a band of 1041 diagonals: the 512-row class
BANDS = [(-4, 4), (-4, 4), (-520, 520)]        # lo <= 0 <= hi everywhere: the same list serves the extension calls
FORMS = ["byte", "table", "ext", "ext_table"]
OUTS = ["ops", "strings", "scores"]


def _pairs():
    rng = random.Random(20250)
    pairs = []
    for n, m in SHAPES:
        p = _rand(rng, n, b"ACGT")
        pairs.append((p, (_mutate(rng, p, b"ACGT", rate=0.05) + _rand(rng, m, b"ACGT"))[:m]))
    return pairs


def _call(c, form, out, pairs, bands):
    """one of the twelve calls -> one tuple per pair: the call's own values, in the order _want lists them"""
    table, go, ge, _alpha = _table("dna")   # five symbols
    seqs, pa, pb = _seqs(pairs)
    ext, tab = form.startswith("ext"), form.endswith("table")
    scoring = (table, go, ge) if tab else SC
    head = (seqs, pa, pb, *scoring, bands, XDROP) if ext else ("sw", seqs, pa, pb, *scoring, bands)
    stem = "banded_subst" if tab else "banded"
    if out == "scores":
        return list(zip(*getattr(c, ("scores_extend_" if ext else "scores_") + stem)(*head, want_end=True)))
    fn = getattr(c, ("extend_" if ext else "align_") + stem + ("_batch" if out == "ops" else "_batch_cigar"))
    extra = {"byte": (), "table": (), "ext": ("rows",), "ext_table": ("rows", "pend")}[form]
    own = ("ops",) if out == "ops" else ("cigar", "mdz")
    return [tuple(r[k] for k in ("score", "end", "start") + own + extra) for r in fn(*head)]


def _want(form, out, pairs, bands):
    table, go, ge, _alpha = _table("dna")
    res = {"byte": lambda: BO.align_many(pairs, bands, "sw", SC[:2], *SC[2:]), "table": lambda: BO.align_many(pairs, bands, "sw", table, go, ge),
           "ext": lambda: XO.extend_many(pairs, bands, SC[:2], *SC[2:], XDROP), "ext_table": lambda: XO.extend_many(pairs, bands, table, go, ge, XDROP)}[form]()
    extra = {"byte": (), "table": (), "ext": ("rows",), "ext_table": ("rows", "pend")}[form]
    want = {}
    for o in out:
        rows = []
        for (p, t), w in zip(pairs, res):
            end, start, tail = tuple(w["end"]), tuple(w["start"]), tuple(w[k] for k in extra)
            if o == "scores":
                rows.append((w["score"],) + end + tail)
            else:
                rows.append((w["score"], end, start) + ((w["ops"],) if o == "ops" else fmt(p, t, w["ops"], start)) + tail)
        want[o] = rows
    return want


def test_forms_interleaved_on_one_context(ctx):
    pairs = _pairs()
    calls = [(f, o) for f in FORMS for o in OUTS]
    want = {f: _want(f, OUTS, pairs, BANDS) for f in FORMS}
    first = {}
    for f, o in calls:
        first[f, o] = _call(ctx, f, o, pairs, BANDS)
        assert first[f, o] == want[f][o], (f, o)
    # the same calls backwards with the wide pair in front: every launch follows one of another kernel, stripe height and row_cap
    order = [2, 0, 1]
    for f, o in reversed(calls):
        again = _call(ctx, f, o, [pairs[k] for k in order], [BANDS[k] for k in order])
        assert [again[order.index(k)] for k in range(len(pairs))] == first[f, o], (f, o)
