"""Every form of the stripe and mini-stripe ("pair") engine, reached by name.  A launch of that engine is one PairForm value (family,
mode, band, walk, cells, rl, w | ln; pwalign.h, pwa_pair_form_table), and which one a call builds is decided by the planners
(TbPlan::class_of, choose_geom, mini_eligible, choose_cell_form).  Here every form has a RECIPE -- the environment, the call, the
alphabet, the pattern lengths and the scorings that pin each of its fields -- and a case that resets the context's record, makes the
call, wants ctx.pair_forms() == [the form's name] and every result equal to the oracle, field for field.

tests/test_pair_forms.py (no GPU) holds the other half: the names with a recipe here are exactly the names pwa_pair_form_table lists.
RECIPES is built from this file's own loops, not from the library's listing, so a form added to either side alone fails there.

What pins which field -- existing switches only, read once per context (conftest.switched_context):
  family, engine   the call (align_batch, overlaps, matrices, a batch with end cells, the gotoh / subst / hw3 / hw4 calls);
                   PWA_FORCE_RL + PWA_FORCE_W keep every pair on the stripe engine at that geometry (mini_eligible refuses the mini
                   classes under them), PWA_TB_ENGINE=2 gives 257 .. 1024 rows one pair per wave; PWA_SCORES_ROUTE=1 (+ PWA_NO_PACKED_DIST)
                   and PWA_AFFINE_TB_ROUTE=1 move hw4's, hw3's score and hw3's alignment lists to the stripe engine
  rl, ln           mini classes: the pattern length alone (mini_rl_for, wide_rl_for; gotoh: <= 256, <= 512, <= 1024 rows)
  w (hw3 align)    the longest pattern: <= 256 rows one compute wave, four beyond
  band             none: a batch with end cells; tb: an alignment call; tb+scores: the same with set_score_band(True), or matrices
  walk             ops: align_batch; overlap: overlaps; none: matrices / a batch
  cells            coded: ACGT; keyed: twenty letters (no code table); plain: PWA_NO_KEYED_TB with a band, twenty letters without one
                   (the band-less fills have no keyed form on raw bytes); gap0: global, ACGT, a scoring inside gap0_ok, no score band;
                   coded in NW with a band: PWA_NO_GAP_SHIFT; coded in NW without one: a scoring whose shifted match constant
                   (match - 2 gap) * 4 + 1 leaves the byte table while (match - gap) * 4 + 2 stays inside (the band-less mini fills
                   take the gap shift from the scoring alone)

Shapes.  Stripe classes at w = 1: 64 rl - 3 rows, one stripe with a short last row block (the band-less coded and gap0 fills see
patterns of more than 256 rows only -- shorter ones go to the mini fills -- so there: the first 64 rl k - 3 above 256); at w = 4:
5 * 64 rl + 3 rows, more stripes than compute waves, so a workgroup takes a second round and reads hand-off rows.  Mini classes: the
class's upper edge 16 rl and the first length above the class below; one pair per wave: both edges of the class.  Texts: a mutated
copy of (at most 300 symbols of) the pattern between short random flanks, 37 columns, 150 unrelated columns, and one empty text.
hw3's alignment class W follows the longest pattern, so its lists hold one length."""
import collections
import random

import numpy as np
import pytest

import gotoh_oracle as GO
import oracle_lib as O
import sg_oracle as SG
from conftest import load_pkg, switched_context

pytestmark = pytest.mark.gpu

MINI_RL = (4, 6, 8, 10, 12, 16)                                              # kernel_table.h, kMiniRL: 16 lanes per pair
WIDE = {6: (257, 384), 8: (385, 512), 12: (513, 768), 16: (769, 1024)}       # wide_rl_for: one pair per wave, (first, last) length
GOTOH_WIDE = {8: (257, 512), 16: (513, 1024)}                                # TbPlan::class_of / setup_gotoh_mini
STRIPE = ((2, 1), (2, 4), (4, 1), (4, 4))
MODES = ("NW", "SW", "SG")
DNA, TWENTY = b"ACGT", b"ACDEFGHIKLMNPQRSTVWY"
LINEAR = ((1, -1, -1), (2, -3, -5))
NO_SHIFT = ((5, -4, -20), (3, -2, -16))     # diag_keys_fit, not gap0_ok: (5 + 40) * 4 + 1 and (3 + 32) * 4 + 1 leave a signed byte
GOTOH = ((1, -4, -6, -1), (2, -3, -5, -2))
GAPS = ((-6, -1), (-11, -2))                # with the two tables of subst_tables()
HW = ((3, -4, -7, -2), (1, -1, -2, -1))     # hw3: match, mismatch, gap opening, gap extension
DIST = ((1, -1, -1), (3, -4, -2))           # hw4

Recipe = collections.namedtuple("Recipe", "name env call mode alpha lens scorings score_band")


def stripe_env(rl, w, **more):
    env = dict(PWA_FORCE_RL=rl, PWA_FORCE_W=w, PWA_SCORES_ROUTE=1, PWA_NO_PACKED_DIST=1, PWA_AFFINE_TB_ROUTE=1, **more)
    return tuple(sorted((k, str(v)) for k, v in env.items()))


def mini_env(**more):
    return tuple(sorted((k, str(v)) for k, v in dict(PWA_TB_ENGINE=2, **more).items()))


def stripe_rows(rl, w, above_mini=False):
    if w == 4:
        return (5 * 64 * rl + 3,)
    k = 1
    while above_mini and 64 * rl * k - 3 <= 256:
        k += 1
    return (64 * rl * k - 3,)


def mini_rows(rl, ln):
    if ln == 64:
        return WIDE[rl]
    below = [r for r in MINI_RL if r < rl]
    return (16 * below[-1] + 1 if below else 1, 16 * rl)


def gotoh_rows(rl, ln):
    return GOTOH_WIDE[rl] if ln == 64 else mini_rows(rl, 16)


def _recipes():
    out = {}

    def add(family, mode, band, walk, cells, rl, w, env, call, alpha, lens, scorings, score_band=False):
        name = "%s/%s/%s/%s/%s/rl%d/%s%d" % (family, mode, band, walk, cells, rl, "ln" if family.startswith("mini") else "w", w)
        assert name not in out, name
        out[name] = Recipe(name, env, call, mode.lower(), alpha, tuple(lens), tuple(scorings), score_band)
    mini = [(rl, 16) for rl in MINI_RL] + [(rl, 64) for rl in WIDE]
    gotoh = [(rl, 16) for rl in MINI_RL] + [(rl, 64) for rl in GOTOH_WIDE]
    for mode in MODES:
        nw = mode == "NW"
        # ---- batches with end cells: no band, the end-cell pick
        for rl, w in STRIPE:
            add("stripe_fill", mode, "none", "none", "plain", rl, w, stripe_env(rl, w), "batch", TWENTY, stripe_rows(rl, w), LINEAR)
            add("stripe_fill", mode, "none", "none", "coded", rl, w, stripe_env(rl, w), "batch", DNA, stripe_rows(rl, w, True), NO_SHIFT if nw else LINEAR)
            if nw:
                add("stripe_fill", mode, "none", "none", "gap0", rl, w, stripe_env(rl, w), "batch", DNA, stripe_rows(rl, w, True), LINEAR)
        for rl in MINI_RL:
            add("mini_fill", mode, "none", "none", "coded", rl, 16, mini_env(), "batch", DNA, mini_rows(rl, 16), NO_SHIFT if nw else LINEAR)
            if nw:
                add("mini_fill", mode, "none", "none", "gap0", rl, 16, mini_env(), "batch", DNA, mini_rows(rl, 16), LINEAR)
        # ---- alignment calls: a band, op lists or overlaps; with the score band beside it
        for band in ("tb", "tb+scores"):
            sb = band == "tb+scores"
            shift = nw and not sb                                    # where the planner would take the gap shift
            for walk in ("ops", "overlap"):
                if walk == "overlap" and mode == "SG":
                    continue
                call = "align" if walk == "ops" else "overlaps"
                for rl, w in STRIPE:
                    rows = stripe_rows(rl, w)
                    if rl == 4:
                        add("stripe_fill", mode, band, walk, "plain", rl, w, stripe_env(rl, w, PWA_NO_KEYED_TB=1), call, DNA, rows, LINEAR, sb)
                    add("stripe_fill", mode, band, walk, "keyed", rl, w, stripe_env(rl, w), call, TWENTY, rows, LINEAR, sb)
                    add("stripe_fill", mode, band, walk, "coded", rl, w, stripe_env(rl, w, PWA_NO_GAP_SHIFT=1) if shift else stripe_env(rl, w), call, DNA, rows, LINEAR, sb)
                    if shift:
                        add("stripe_fill", mode, band, walk, "gap0", rl, w, stripe_env(rl, w), call, DNA, rows, LINEAR, sb)
                for rl, ln in mini:
                    add("mini_fill", mode, band, walk, "coded", rl, ln, mini_env(PWA_NO_GAP_SHIFT=1) if shift else mini_env(), call, DNA, mini_rows(rl, ln), LINEAR, sb)
                    if shift:
                        add("mini_fill", mode, band, walk, "gap0", rl, ln, mini_env(), call, DNA, mini_rows(rl, ln), LINEAR, sb)
        # ---- matrices: both bands, no walk
        for rl, w in STRIPE:
            if rl == 4:
                add("stripe_fill", mode, "tb+scores", "none", "plain", rl, w, stripe_env(rl, w, PWA_NO_KEYED_TB=1), "matrices", DNA, stripe_rows(rl, w), LINEAR)
            add("stripe_fill", mode, "tb+scores", "none", "keyed", rl, w, stripe_env(rl, w), "matrices", DNA, stripe_rows(rl, w), LINEAR)
        for rl, ln in mini:
            add("mini_fill", mode, "tb+scores", "none", "coded", rl, ln, mini_env(), "matrices", DNA, mini_rows(rl, ln), LINEAR)
        # ---- the affine-gap families
        for rl, ln in gotoh:
            add("mini_gotoh", mode, "none", "none", "keyed", rl, ln, mini_env(), "gotoh_batch", DNA, gotoh_rows(rl, ln), GOTOH)
            add("mini_gotoh", mode, "tb", "ops", "keyed", rl, ln, mini_env(), "gotoh_align", DNA, gotoh_rows(rl, ln), GOTOH)
            add("mini_subst", mode, "none", "none", "keyed", rl, ln, mini_env(), "subst_batch", DNA, gotoh_rows(rl, ln), GAPS)
            add("mini_subst", mode, "tb", "ops", "keyed", rl, ln, mini_env(), "subst_align", DNA, gotoh_rows(rl, ln), GAPS)
    # ---- hw4's distances, hw3's scores and alignments on the stripe engine
    for rl, w in STRIPE:
        add("stripe_dist", "NW", "none", "none", "plain", rl, w, stripe_env(rl, w), "dist", DNA, stripe_rows(rl, w), DIST)
        add("stripe_affine", "NW", "none", "none", "plain", rl, w, stripe_env(rl, w), "affine", DNA, stripe_rows(rl, w), HW)
        if rl == 4:
            add("stripe_affine_tb", "NW", "tb", "ops", "plain", rl, w, stripe_env(rl, w), "affine_tb", DNA, stripe_rows(rl, w), HW)
    return out


RECIPES = _recipes()
RAN = set()   # the names whose case found exactly its form in the record: test_every_listed_form_ran


# ------------------------------------------------------------------ lists
def rand_seq(rng, n, alpha):
    return bytes(rng.choice(alpha) for _ in range(n))


def mutated(rng, s, alpha):
    """s with one symbol in eight replaced, dropped or doubled: matches, mismatches and both gaps"""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < 0.04:
            continue
        out.append(rng.choice(alpha) if r < 0.09 else c)
        if r > 0.96:
            out.append(rng.choice(alpha))
    return bytes(out)


_PAIRS = {}


def pairs_of(lens, alpha):
    """[(pattern, text)]: the longest pattern against a mutated copy, 37 columns and nothing; the shortest (the same one when the
    class has one length) against 150 unrelated columns and a mutated copy of its own"""
    key = (lens, alpha)
    if key not in _PAIRS:
        rng = random.Random("%s %s" % (lens, alpha))
        pats = [rand_seq(rng, n, alpha) for n in lens]

        def near(p):
            a = rng.randrange(0, max(1, len(p) - 300))
            return rand_seq(rng, 11, alpha) + mutated(rng, p[a:a + 300], alpha) + rand_seq(rng, 17, alpha)
        hi, lo = pats[-1], pats[0]
        out = [(hi, near(hi)), (hi, rand_seq(rng, 37, alpha)), (lo, rand_seq(rng, 150, alpha)), (hi, b"")]
        if len(lens) > 1:
            out.insert(3, (lo, near(lo)))
        _PAIRS[key] = out
    return _PAIRS[key]


_TABLES = []


def subst_tables():
    if not _TABLES:
        _TABLES.extend(GO.random_table(seed, DNA) for seed in (5, 6))
    return _TABLES


# ------------------------------------------------------------------ oracles, once per (call, mode, list, scoring)
_WANT = {}


def want(r, sc, which):
    kind = {"batch": "linear", "align": "linear", "overlaps": "linear", "gotoh_batch": "gotoh", "gotoh_align": "gotoh", "subst_batch": "subst",
            "subst_align": "subst"}.get(r.call, r.call)
    key = (kind, r.mode, r.lens, r.alpha, sc, which)
    if key in _WANT:
        return _WANT[key]
    pairs = pairs_of(r.lens, r.alpha)
    if kind == "linear":
        w = [SG.align(p, t, *sc) if r.mode == "sg" else O.align(r.mode, p, t, *sc) for p, t in pairs]
    elif kind == "matrices":
        w = []
        for p, t in pairs:
            if r.mode == "sg":
                m = SG.align(p, t, *sc, mats=True)
                w.append((m["dp"], m["tb"]))
            else:
                w.append(O.matrices(r.mode, p, t, *sc))
    elif kind == "gotoh":
        w = GO.align_many(pairs, r.mode, sc[:2], *sc[2:])
    elif kind == "subst":
        w = GO.align_many(pairs, r.mode, subst_tables()[which], *sc)
    elif kind == "dist":
        w = [O.nw_distance(p, t, *sc)[0] for p, t in pairs]
    elif kind == "affine":
        w = [O.affine_score(p, t, *sc) for p, t in pairs]
    else:
        w = [O.affine_align(p, t, *sc) for p, t in pairs]
    _WANT[key] = w
    return w


def full(rows):
    return [(x["score"], tuple(x["end"]), tuple(x["start"]), x["ops"]) for x in rows]


def ends(rows):
    return [x["score"] for x in rows], [x["end"][0] for x in rows], [x["end"][1] for x in rows]


def fetched(b):
    try:
        b.run()
        return b.fetch()
    finally:
        b.close()


def call(c, r, sc, which):
    """-> (what the library returned, what the oracle says), in one comparable shape"""
    pairs = pairs_of(r.lens, r.alpha)
    seqs = [x for pt in pairs for x in pt]
    pa, pb = list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))
    w = want(r, sc, which)
    if r.call == "batch":
        return tuple(fetched(c.batch(r.mode, seqs, pa, pb, *sc, want_end=True))), ends(w)
    if r.call == "align":
        return full(c.align_batch(r.mode, seqs, pa, pb, *sc)), full(w)
    if r.call == "overlaps":
        return c.overlaps(r.mode, seqs, pa, pb, *sc), ([x["score"] for x in w], [x["overlap"] for x in w])
    if r.call == "gotoh_batch":
        return tuple(fetched(c.batch_gotoh(r.mode, seqs, pa, pb, *sc, want_end=True))), ends(w)
    if r.call == "gotoh_align":
        return full(c.align_gotoh_batch(r.mode, seqs, pa, pb, *sc)), full(w)
    if r.call == "subst_batch":
        return tuple(fetched(c.batch_subst(r.mode, seqs, pa, pb, subst_tables()[which], *sc, want_end=True))), ends(w)
    if r.call == "subst_align":
        return full(c.align_subst_batch(r.mode, seqs, pa, pb, subst_tables()[which], *sc)), full(w)
    if r.call == "dist":
        return c.distances(seqs, pa, pb, *sc), w
    if r.call == "affine":
        return c.scores_affine(seqs, pa, pb, *sc), w
    assert r.call == "affine_tb", r.call
    return [(x["score"], x["ops"]) for x in c.align_affine_batch(seqs, pa, pb, *sc)], [(x["score"], x["ops"]) for x in w]


# ------------------------------------------------------------------ the cases, environment by environment
CASES = sorted(RECIPES.values(), key=lambda r: (r.env, r.name))


@pytest.fixture(scope="module")
def context_for():
    """one context per environment: the cases are sorted by it, so a context is created when the environment changes and closed then"""
    held = {}

    def get(env):
        if held.get("env") != env:
            if "cm" in held:
                held.pop("cm").__exit__(None, None, None)
            held["env"] = env
            held["cm"] = switched_context(**dict(env))
            held["ctx"] = held["cm"].__enter__()
        return held["ctx"]
    yield get
    if "cm" in held:
        held.pop("cm").__exit__(None, None, None)


@pytest.mark.parametrize("recipe", CASES, ids=lambda r: r.name)
def test_pair_form(context_for, recipe):
    r = recipe
    c = context_for(r.env)
    c.set_score_band(r.score_band)
    try:
        for which, sc in enumerate(r.scorings):
            if r.call == "matrices":   # one pair per call: the record is read after each
                for k, (p, t) in enumerate(pairs_of(r.lens, r.alpha)):
                    if not t:
                        continue
                    c.reset_pair_forms()
                    dp, tb = c.matrices(r.mode, p, t, *sc)
                    assert c.pair_forms() == [r.name], (c.pair_forms(), sc, len(p), len(t))
                    RAN.add(r.name)
                    wdp, wtb = want(r, sc, which)[k]
                    assert np.array_equal(dp, wdp) and np.array_equal(tb, wtb), (r.name, sc, len(p), len(t))
                continue
            c.reset_pair_forms()
            got, wanted = call(c, r, sc, which)
            assert c.pair_forms() == [r.name], (c.pair_forms(), sc)
            RAN.add(r.name)
            assert got == wanted, (r.name, sc, [(len(p), len(t)) for p, t in pairs_of(r.lens, r.alpha)])
    finally:
        c.set_score_band(False)


def test_every_listed_form_ran():
    """the guard against vacuity (runs last): the forms whose cases found exactly their name in the record are the whole listing"""
    listed = set(load_pkg().pair_form_table())
    assert RAN == listed, (sorted(listed - RAN)[:12], sorted(RAN - listed)[:12])
