"""Every instantiated register-strip kernel, reached by name.  The strip table (strip_kernels_{sw,nw,aff,gotoh}.hip) holds one entry
per (R, cell form, score path), and an entry up to six kernels (kernel_table.h: multi-strip, single strip, LANES and CELL16 forms of
both).  Which of them a list runs is the scheduler's choice (choose_cell_form, plan_strip_tasks, choose_strip_height, cell16_admitted in
pwalign.hip), so here every (entry, variant) has a RECIPE: the environment that pins the height, the scoring that picks the cell
form, the alphabet that picks the score path and the list shape that picks the variant.  A case builds its list, asserts the kernel
name the batch reports (and cell_bits() for the packed f16 forms), runs it and wants every result equal to the oracle.

tests/test_strip_table.py (no GPU) holds the other half: every (entry, variant) that pwa_strip_table lists has a recipe here, under
the name the library reports, except the profile forms named in PROFILE_FORMS.

What steers the choice -- existing switches only, read once per context (conftest.switched_context):
  PWA_SCORES_ROUTE=0    every pair stays on the strips (no work-aware split)
  PWA_FORCE_R           the strip height
  PWA_FORCE_MODE=0 | 6  plain against saturating SW (both serve every SW list; the cost model prefers the saturating form)
  PWA_CELL16=0 | 1      int32 cells against packed f16 cells where the latter are admitted
  PWA_FORCE_LANES=0     a text-grouped list this small counts as underfilled and would get every lane its own text
  PWA_NO_PACKED_DIST    hw4's two-value distance form for lists inside the packed key's bounds
The scoring does the rest: small scores give the shifted / gap-shifted forms, a gap-open term of 2^25 / (max_n + max_m + 4) and more
the plain affine and gotoh forms, 100 / -90 / -70 plain BM_NW; four letters give SC_PERM, twenty-six SC_CMP.

Shapes are sized for the height under test.  Multi-strip variants: pattern lengths 1, R-1, R, R+1, 2R-1, 2R, 2R+1, 3R+2 mixed in
one wave task (pad rows, lanes that finish strips early); single-strip variants: 1, R/2, R-1, R and nothing longer (max_strips == 1
selects them).  Text-grouped lists: 70 patterns (130 for the 128-slot packed tasks) against a 70-column text -- a full task and a
partly empty one, hand-off rows with a tail block -- and one pattern of every length against texts of 1, 2, 3, 5, 8, 18, 31 and 69
columns: every residue mod 4, and texts without a single 4-column block.  Index-paired lists: 70 pairs, every text used once, the
same two length sets.  Every other pattern is a mutated copy of its text, the rest are unrelated to it."""
import collections
import random

import pytest

import gotoh_oracle as GO
import oracle_lib as O
from conftest import switched_context

pytestmark = pytest.mark.gpu

BM_SW, BM_NW, BM_NWG, BM_AFF, BM_AFFS, BM_DIST, BM_SWS, BM_DISTP, BM_GNW, BM_GNWS, BM_GSW = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10   # kernel_table.h
MODE_NAME = {BM_SW: "BM_SW", BM_NW: "BM_NW", BM_NWG: "BM_NWG", BM_AFF: "BM_AFF", BM_AFFS: "BM_AFFS", BM_SWS: "BM_SWS", BM_GNW: "BM_GNW",
             BM_GNWS: "BM_GNWS", BM_GSW: "BM_GSW"}
SC_PERM, SC_CMP = 0, 1
SC_NAME = {SC_PERM: "SC_PERM", SC_CMP: "SC_CMP"}
BASE = "multi"   # the variant every entry has: its multi-strip kernel (fn, afn or dfn of BatchKernelEntry)
# the variants without a recipe here, and where they are tested instead: the profile forms of the packed f16 cells, one instantiation
# each, hung on both CELL16 entries (tests/test_gpu_scores_profile*.py, by pwa_batch_profile_form / _profile_int)
PROFILE_FORMS = {(R, BM_SWS, SC_PERM, v) for R in (52, 76) for v in ("prof16", "prof16_int")}

ALPHA = {SC_PERM: b"ACGT", SC_CMP: bytes(range(65, 91))}
TEXT_LENGTHS = (70, 1, 2, 3, 5, 8, 18, 31, 69)   # the first takes the full tasks

Recipe = collections.namedtuple("Recipe", "R mode score variant name call scoring env")


def _name(R, mode, score):
    if mode in (BM_DIST, BM_DISTP):
        return "batch_nwdist_kernel<R=%d,%s>" % (R, "PACKED" if mode == BM_DISTP else SC_NAME[score])
    head = "batch_affine_kernel" if mode in (BM_AFF, BM_AFFS) else "batch_gotoh_kernel" if mode in (BM_GNW, BM_GNWS, BM_GSW) else "batch_scores_kernel"
    return "%s<R=%d,%s,%s>" % (head, R, MODE_NAME[mode], SC_NAME[score])


# call, scoring: "big" stands for the gap-open term that takes the list out of the shifted form (big_gap_open)
FORMS = {BM_SW: ("sw", (5, -4, -7)), BM_SWS: ("sw", (5, -4, -7)), BM_NW: ("nw", (100, -90, -70)), BM_NWG: ("nw", (2, -3, -4)),
         BM_AFFS: ("affine", (3, -4, -7, -2)), BM_AFF: ("affine", (3, -4, "big", -2)), BM_DIST: ("nwdist", (3, -4, -2)), BM_DISTP: ("nwdist", (3, -4, -2)),
         BM_GNWS: ("gotoh nw", (3, -4, -7, -2)), BM_GNW: ("gotoh nw", (3, -4, "big", -2)), BM_GSW: ("gotoh sw", (3, -4, -7, -2))}


def _recipes():
    out = {}

    def add(heights, mode, paths, variants):
        for R in heights:
            for score in paths:
                for v in variants:
                    env = {"PWA_SCORES_ROUTE": "0", "PWA_FORCE_R": str(R), "PWA_CELL16": "1" if v.startswith("cell16") else "0"}
                    if not v.startswith("lanes"):
                        env["PWA_FORCE_LANES"] = "0"
                    if mode in (BM_SW, BM_SWS):
                        env["PWA_FORCE_MODE"] = str(mode)
                    if mode == BM_DIST:
                        env["PWA_NO_PACKED_DIST"] = "1"
                    assert (R, mode, score, v) not in out
                    out[(R, mode, score, v)] = Recipe(R, mode, score, v, _name(R, mode, score), FORMS[mode][0], FORMS[mode][1], tuple(sorted(env.items())))
    both, singles, lanes = (SC_PERM, SC_CMP), (BASE, "single"), ("lanes", "lanes_single")
    add((64, 76, 104, 128, 152), BM_SW, (SC_PERM,), singles)
    add((64, 128, 152), BM_SW, (SC_CMP,), singles)
    add((40, 52, 76, 96), BM_SWS, both, singles + lanes)
    add((52, 76), BM_SWS, (SC_PERM,), ("cell16", "cell16_single"))
    add((64, 128, 152), BM_NW, both, singles)
    add((64, 128, 152), BM_NWG, both, singles)
    add((64, 128, 152), BM_NWG, (SC_PERM,), lanes)
    add((32, 52), BM_AFFS, both, (BASE,))
    add((32, 52), BM_AFF, both, (BASE,))
    add((32, 64), BM_DIST, both, (BASE,))
    add((64, 128), BM_DISTP, both, (BASE,))
    for mode in (BM_GNWS, BM_GNW, BM_GSW):
        add((32, 52), mode, both, (BASE,))
    return out


RECIPES = _recipes()


# ------------------------------------------------------------------ lists
def rand_seq(rng, n, alpha):
    return bytes(rng.choice(alpha) for _ in range(n))


def related(rng, text, n, alpha):
    """n symbols over alpha: the text (continued at random where it is shorter) with one symbol in ten replaced, dropped or doubled,
    and with every symbol of the text that alpha does not hold replaced"""
    base = bytearray((text + rand_seq(rng, n, alpha))[:n + 8])
    out = bytearray()
    for c in base:
        r = rng.random()
        if r < 0.03:
            continue
        out.append(rng.choice(alpha) if r < 0.07 or c not in alpha else c)
        if r > 0.97:
            out.append(rng.choice(alpha))
    return bytes((out + rand_seq(rng, n, alpha))[:n])


def pattern_lengths(R, single):
    return (1, R // 2, R - 1, R) if single else (1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R + 2)


def strip_list(R, variant, score):
    """-> (seqs, pair_a, pair_b) for one (height, variant, score path); seeded by them, so the same list every time"""
    rng = random.Random("%d %s %d" % (R, variant, score))
    single = variant.endswith("single")
    plens = pattern_lengths(R, single)
    alpha = ALPHA[score]
    # the packed f16 cells take patterns over four codes; a fifth symbol in the texts alone keeps the list out of their profile form
    talpha = alpha + b"N" if variant.startswith("cell16") else alpha
    seqs, pa, pb = [], [], []

    def pattern(text, n, k):
        return related(rng, text, n, alpha) if k % 2 == 0 else rand_seq(rng, n, alpha)
    if variant.startswith("lanes"):   # index-paired: every text once, more tasks than a text-grouped list would fill
        for k in range(70):
            t = rand_seq(rng, TEXT_LENGTHS[k % len(TEXT_LENGTHS)], talpha)
            seqs += [pattern(t, plens[(k // 2) % len(plens)], k), t]
            pa.append(len(seqs) - 2)
            pb.append(len(seqs) - 1)
        # (the LANES form of global alignment wants every pattern symbol among the texts')
        assert score == SC_CMP or set(b"".join(seqs[1::2])) >= set(b"".join(seqs[0::2]))
    else:
        full = 130 if variant.startswith("cell16") else 70
        for j, m in enumerate(TEXT_LENGTHS):
            t = rand_seq(rng, m, talpha)
            seqs.append(t)
            ti = len(seqs) - 1
            for k in range(full if j == 0 else len(plens)):
                seqs.append(pattern(t, plens[k % len(plens)], k + j))
                pa.append(len(seqs) - 1)
                pb.append(ti)
    longest = max(len(seqs[a]) for a in pa)
    assert all(set(seqs[a]) <= set(alpha) for a in pa)
    assert longest ==(R if single else 3 * R + 2) and len(pa) <= 200 and {len(seqs[b]) % 4 for b in pb} == {0, 1, 2, 3}
    return seqs, pa, pb


def big_gap_open(seqs, pa, pb):
    """the smallest |gap_open| at which (max_n + max_m + 4) * 4 * |gap_open| reaches 2^27: outside the shifted affine and gotoh forms"""
    span = max(len(seqs[a]) for a in pa) + max(len(seqs[b]) for b in pb) + 4
    a = -((1 << 25) // -span)
    assert span * (a - 1) * 4 < 1 << 27 <= span * a * 4 and (span + 2) * (a + 2) < 1 << 28   # ... and far inside the gotoh calls' own range
    return -a


def make_batch(c, call, seqs, pa, pb, scoring):
    if call in ("sw", "nw"):
        return c.batch(call, seqs, pa, pb, *scoring)
    if call == "affine":
        return c.batch_affine(seqs, pa, pb, *scoring)
    if call == "nwdist":
        return c.batch_distances(seqs, pa, pb, *scoring)
    return c.batch_gotoh(call.split()[1], seqs, pa, pb, *scoring)


def oracle_results(call, seqs, pa, pb, scoring):
    pairs = [(seqs[a], seqs[b]) for a, b in zip(pa, pb)]
    if call in ("sw", "nw"):
        return [O.score(call, p, t, *scoring)[0] for p, t in pairs]
    if call == "affine":
        return [O.affine_score(p, t, *scoring) for p, t in pairs]
    if call == "nwdist":
        return [O.nw_distance(p, t, *scoring)[0] for p, t in pairs]
    return [w["score"] for w in GO.align_many(pairs, call.split()[1], scoring[:2], *scoring[2:], want_ops=False)]


def run_named(c, call, seqs, pa, pb, scoring):
    """-> (kernel name, cell bits, profile form, results) of one prepared batch"""
    b = make_batch(c, call, seqs, pa, pb, scoring)
    try:
        b.run()
        return b.info()["kernel"], b.cell_bits(), b.profile_form(), b.fetch()
    finally:
        b.close()


def mismatches(got, want, seqs, pa, pb):
    return [(k, len(seqs[pa[k]]), len(seqs[pb[k]]), g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:8]


# ------------------------------------------------------------------ the cases, environment by environment
CASES = sorted(RECIPES.values(), key=lambda r: (r.env, r.mode, r.score, r.variant))


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


@pytest.mark.parametrize("recipe", CASES, ids=lambda r: "%s-%s" % (r.name, r.variant))
def test_strip_kernel(context_for, recipe):
    seqs, pa, pb = strip_list(recipe.R, recipe.variant, recipe.score)
    scoring = tuple(big_gap_open(seqs, pa, pb) if s == "big" else s for s in recipe.scoring)
    name, bits, profile, got = run_named(context_for(recipe.env), recipe.call, seqs, pa, pb, scoring)
    want_name = recipe.name[:-1] + ",LANES>" if recipe.variant.startswith("lanes") else recipe.name
    assert name == want_name, (name, want_name)                        # the strips alone: no " + " part of another engine
    assert bits == (16 if recipe.variant.startswith("cell16") else 32) and profile == 0, (bits, profile)
    want = oracle_results(recipe.call, seqs, pa, pb, scoring)
    assert got == want, (recipe.name, recipe.variant, scoring, mismatches(got, want, seqs, pa, pb))
