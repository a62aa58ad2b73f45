"""Wavefront (WFA) global affine-gap alignments on the GPU (pwa_scores_wfa, pwa_align_wfa_batch(_cigar), pwa_wfa_last_stats) against
wfa_oracle.py: scores, penalties, op lists byte for byte, the strings, the stats' cells, the bound and the not-found sentinel, at the
smallest shapes at which each mechanism of the kernels can go wrong; long pairs against the banded score pass."""
import ctypes as C
import functools
import random

import pytest

import gotoh_oracle as GO
import wfa_oracle as WO
from conftest import load_pkg, switched_context

pytestmark = pytest.mark.gpu

SC = (1, -4, -6, -1)   # x, o, e = 10, 12, 3
INVALID, CAPACITY = -1, -5


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet=b"ACGT"):
    """substitutions, insertions and deletions, each at rate / 3 per symbol"""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice(alphabet))
            out.append(c)
        elif r < rate:
            out.append(rng.choice([a for a in alphabet if a != c]))
        else:
            out.append(c)
    return bytes(out)


def strings_of(p, t, ops):
    """CIGAR and MD:Z of an op list in traceback order from (n, m) to (0, 0), as pwa_format_alignment writes them (NUL bytes kept)"""
    cg, md = bytearray(), bytearray()
    i = j = matches = 0
    fwd = ops[::-1]
    c = 0
    while c < len(fwd):
        run = 1
        while c + run < len(fwd) and fwd[c + run] == fwd[c]:
            run += 1
        cg += b"%d%c" % (run, fwd[c])
        if fwd[c] == 77:
            for _ in range(run):
                if p[i] == t[j]:
                    matches += 1
                else:
                    md += b"%d" % matches + bytes([t[j]])
                    matches = 0
                i, j = i + 1, j + 1
        elif fwd[c] == 68:
            md += b"%d^" % matches + p[i:i + run]
            matches = 0
            i += run
        else:
            j += run
        c += run
    md += b"%d" % matches
    return bytes(cg), bytes(md)


def flatten(pairs, front=()):
    seqs = list(front)
    pa, pb = [], []
    for p, t in pairs:
        pa.append(len(seqs))
        pb.append(len(seqs) + 1)
        seqs += [p, t]
    return seqs, pa, pb


def oracle(pairs, sc, bounds=None):
    return [WO.align(p, t, *sc, min_score=None if bounds is None else bounds[k]) for k, (p, t) in enumerate(pairs)]


def check(c, pairs, sc, bounds=None, want=None, front=()):
    """every call on one list against the oracle's results `want`"""
    pkg = load_pkg()
    want = want or oracle(pairs, sc, bounds)
    seqs, pa, pb = flatten(pairs, front)
    cells = sum(w["cells"] for w in want)
    scores, pens = c.scores_wfa(seqs, pa, pb, *sc, min_score=bounds, want_penalty=True)
    assert scores == [w["score"] for w in want]
    assert pens == [w["penalty"] for w in want]
    assert c.align_wfa_stats()["cells"] == cells
    al = c.align_wfa_batch(seqs, pa, pb, *sc, min_score=bounds)
    st = c.align_wfa_stats()
    assert st["cells"] == cells
    cg = c.align_wfa_batch_cigar(seqs, pa, pb, *sc, min_score=bounds)
    assert c.align_wfa_stats()["cells"] == cells
    for k, ((p, t), w) in enumerate(zip(pairs, want)):
        assert al[k]["score"] == w["score"] and cg[k]["score"] == w["score"], k
        assert al[k]["ops"] == w["ops"], (k, p, t)
        assert al[k]["end"] == (len(p), len(t)) and al[k]["start"] == (0, 0)
        if w["score"] is None:
            assert (cg[k]["cigar"], cg[k]["mdz"]) == (b"", b""), k
            continue
        assert (cg[k]["cigar"], cg[k]["mdz"]) == strings_of(p, t, w["ops"]), k
        if 0 not in p and 0 not in t:
            f = pkg.format_alignment(p, t, w["ops"], (len(p), len(t)))
            assert (cg[k]["cigar"], cg[k]["mdz"]) == (f["cigar"], f["mdz"]), k
    return al, st


# ------------------------------------------------------------------ empty and trivial
def test_empty_and_trivial_pairs(ctx):
    pairs = [(b"", b""), (b"ACGTA", b""), (b"", b"ACG"), (b"ACGTACGTAC", b"ACGTACGTAC"), (b"ACGTACGTAC", b"ACGTTCGTAC"),
             (b"ACGTACGTAC", b"ACGTCGTAC"), (b"ACGTCGTAC", b"ACGTACGTAC"), (b"A", b"C"), (b"A", b"A"), (b"A", b""), (b"", b"T")]
    al, _ = check(ctx, pairs, SC)
    assert [a["ops"] for a in al[:4]] == [b"", b"DDDDD", b"III", b"M" * 10]
    assert [a["score"] for a in al[:5]] == [0, -11, -9, 10, 5]
    assert ctx.scores_wfa([b"A"], [], [], *SC) == [] and ctx.align_wfa_batch([b"A"], [], [], *SC) == []
    assert ctx.align_wfa_batch_cigar([b"A"], [], [], *SC) == []


# ------------------------------------------------------------------ lane-chunk edges: the wavefront passes 64 and 128 diagonals
def test_gap_runs_across_the_lane_chunks(ctx):
    rng = random.Random(5)
    p = rand_seq(rng, 300)
    pairs = []
    for run in (31, 32, 33, 63, 64, 65, 130):
        at = rng.randint(40, 120)
        pairs.append((p, p[:at] + rand_seq(rng, run) + p[at:]))      # an inserted run: the wavefront grows upwards
        pairs.append((p, p[:at] + p[at + run:]))                     # a deleted run: downwards
    al, _ = check(ctx, pairs, SC)
    for k, run in enumerate((31, 32, 33, 63, 64, 65, 130)):
        assert al[2 * k]["score"] >= 300 - 6 - run and al[2 * k + 1]["score"] == 300 - run - 6 - run


# ------------------------------------------------------------------ extend: 8 bytes per step, ended by the clamp
def test_extend_match_runs_of_every_length(ctx):
    rng = random.Random(6)
    p, t = bytearray(), bytearray()
    for run in list(range(21)) + list(range(20, -1, -1)):
        s = rand_seq(rng, run, b"GT")
        p += s + b"A"
        t += s + b"C"
    pairs = [(bytes(p), bytes(t)), (bytes(p[:-1]), bytes(t[:-1])), (bytes(p[3:]), bytes(t[3:]))]
    check(ctx, pairs, (1, -1, -3, -2))


def test_extend_at_every_blob_offset_and_at_the_blob_end(ctx):
    rng = random.Random(7)
    p = rand_seq(rng, 37)
    t = mutate(rng, p, 0.1) + rand_seq(rng, 4)
    seqs = []
    for d in range(8):
        seqs += [b"x" * d, p, t]
    off, at = set(), 0
    for s in seqs:
        if s in (p, t):
            off.add(at % 8)
        at += len(s)
    assert off == set(range(8))
    pa, pb = [3 * d + 1 for d in range(8)], [3 * d + 2 for d in range(8)]
    want = WO.align(p, t, *SC)
    assert ctx.scores_wfa(seqs, pa, pb, *SC) == [want["score"]] * 8
    assert [a["ops"] for a in ctx.align_wfa_batch(seqs, pa, pb, *SC)] == [want["ops"]] * 8
    # the last pair ends on the blob's last byte; its text is a run that goes on to that byte
    long_run = rand_seq(rng, 61)
    check(ctx, [(long_run[:29], long_run), (long_run, long_run[:29]), (long_run[5:], long_run)], SC, front=[b"xyz"])


def test_extend_stops_at_the_length_not_at_the_neighbour(ctx):
    rng = random.Random(8)
    s = rand_seq(rng, 45)
    seqs = [s, s, s]   # back to back: an extend that ignores the length runs on into the copy
    pa, pb = [0, 1, 0, 2, 1], [1, 2, 2, 0, 1]
    assert ctx.scores_wfa(seqs, pa, pb, *SC, want_penalty=True) == ([45] * 5, [0] * 5)
    assert [a["ops"] for a in ctx.align_wfa_batch(seqs, pa, pb, *SC)] == [b"M" * 45] * 5
    # prefixes of the same sequence next to it: the run reaches the pattern's end while the text goes on, and the reverse
    check(ctx, [(s[:16], s), (s, s[:16]), (s[:8], s[:9]), (s[:24], s[:17])], SC)


def test_bytes_nul_dash_and_ff(ctx):
    rng = random.Random(9)
    alphabet = b"\x00-\xffA"
    pairs = []
    for n in (1, 7, 8, 9, 60, 150):
        p = rand_seq(rng, n, alphabet)
        pairs += [(p, mutate(rng, p, 0.15, alphabet)), (p, rand_seq(rng, n + 3, alphabet)), (b"\x00" * n, b"\x00" * (n + 1))]
    check(ctx, pairs, SC)


# ------------------------------------------------------------------ long pairs: the point of the feature
def test_long_pairs_against_the_banded_scores(ctx, pkg):
    rng = random.Random(10)
    seqs = []
    for _ in range(16):
        p = rand_seq(rng, 5000)
        seqs += [p, mutate(rng, p, 0.01)]
    pa, pb = list(range(0, 32, 2)), list(range(1, 32, 2))
    bands = [pkg.band_around(len(seqs[a]), len(seqs[b]), 512) for a, b in zip(pa, pb)]
    banded = ctx.scores_banded("nw", seqs, pa, pb, *SC, bands)
    scores, pens = ctx.scores_wfa(seqs, pa, pb, *SC, want_penalty=True)
    assert scores == banded
    x, o, e, g = WO.penalties(*SC)
    assert [WO.score_of(pens[k], len(seqs[pa[k]]), len(seqs[pb[k]]), SC[0], g) for k in range(16)] == scores
    al = ctx.align_wfa_batch(seqs, pa, pb, *SC, min_score=[s - 150 for s in scores])   # a bound keeps the plan near the penalty
    for k in range(16):
        p, t, ops = seqs[pa[k]], seqs[pb[k]], al[k]["ops"]
        assert al[k]["score"] == scores[k]
        assert (ops.count(b"M") + ops.count(b"D"), ops.count(b"M") + ops.count(b"I")) == (len(p), len(t))
        assert GO.op_score(p, t, ops, (0, 0), SC[:2], SC[2], SC[3]) == scores[k]


# ------------------------------------------------------------------ the bound; ranges; junk in the buffers
@functools.lru_cache(maxsize=None)
def mixed():
    """found pairs, pairs not found on the host (both cases) and by the sweep, empty-sided pairs -> pairs, bounds, the oracle's results"""
    rng = random.Random(11)
    pairs, bounds = [], []
    for n in (40, 90, 200, 330):
        p = rand_seq(rng, n)
        for t in (mutate(rng, p, 0.08), p[:n // 3] + rand_seq(rng, 9) + p[n // 3:], p):
            best = WO.align(p, t, *SC, want_ops=False)["score"]
            for b in (best, best + 1, -(1 << 20), None, best - 7):
                pairs.append((p, t))
                bounds.append(b)
    pairs += [(b"", b""), (b"", b""), (b"ACGT", b""), (b"ACGT", b""), (b"", b"AC"), (b"", b"AC"), (b"ACGTAC", b"ACG"), (b"ACGTAC", b"ACG")]
    bounds += [0, 1, -10, -9, -8, -7, -6, -5]
    bounds = [-(1 << 30) if b is None else b for b in bounds]   # one list of ints: "no bound" as a bound far below
    want = oracle(pairs, SC, bounds)
    kinds = {(w["score"] is None, w["cells"] > 0) for w in want}
    assert kinds == {(False, True), (True, False), (True, True)}   # found; not found on the host; not found by the sweep
    return pairs, bounds, want


def test_bound_at_above_and_below_the_optimum(ctx):
    pairs, bounds, want = mixed()
    check(ctx, pairs, SC, bounds, want)
    free = oracle(pairs[:12], SC)
    check(ctx, pairs[:12], SC, None, free)                       # None: no bound
    best = [w["score"] for w in free]
    check(ctx, pairs[:12], SC, best)                             # every pair at its optimum
    al, _ = check(ctx, pairs[:12], SC, [b + 1 for b in best])    # ... and one above: nothing is found
    assert all(a["score"] is None and a["ops"] == b"" for a in al)
    assert ctx.scores_wfa(*flatten(pairs[:12]), *SC, min_score=-(1 << 20)) == best   # one int for every pair


def split(sizes, budget):
    """ranges of consecutive pairs as the library cuts them: at least one pair, then while the next still fits"""
    out, k = [], 0
    while k < len(sizes):
        tot, k0 = sizes[k], k
        k += 1
        while k < len(sizes) and tot + sizes[k] <= budget:
            tot += sizes[k]
            k += 1
        out.append((k0, k))
    return out


def test_ranges_and_poisoned_buffers_change_nothing(ctx, pkg):
    pairs, bounds, want = mixed()
    plan = pkg.wfa_plan(*SC, [(len(p), len(t)) for p, t in pairs], bounds)
    sizes = [12 * c + len(p) + len(t) for c, (p, t) in zip(plan["cells"], pairs)]
    budget = max(4096, sum(sizes) // 5)
    assert len(split(sizes, budget)) >= 3
    plain, st = check(ctx, pairs, SC, bounds, want)
    with switched_context(PWA_RANGE_BYTES=budget) as c:
        cut, st_cut = check(c, pairs, SC, bounds, want)
        assert cut == plain and st_cut["cells"] == st["cells"] and st_cut["workspace_bytes"] < st["workspace_bytes"]
    for byte in ("0xA5", "0"):
        with switched_context(PWA_POISON=byte) as c:
            got, _ = check(c, pairs, SC, bounds, want)
            assert got == plain
            assert c.poison_stats()["buffers"] > 0
        with switched_context(PWA_POISON=byte, PWA_RANGE_BYTES=budget) as c:
            assert check(c, pairs, SC, bounds, want)[0] == plain


def test_workspace_is_twelve_bytes_per_planned_cell(ctx, pkg):
    pairs, bounds, want = mixed()
    seqs, pa, pb = flatten(pairs)
    plan = pkg.wfa_plan(*SC, [(len(p), len(t)) for p, t in pairs], bounds)
    ctx.align_wfa_batch(seqs, pa, pb, *SC, min_score=bounds)
    assert ctx.align_wfa_stats()["workspace_bytes"] == 12 * sum(plan["cells"])


# ------------------------------------------------------------------ scorings: linear, a wide ring, g = 4
@functools.lru_cache(maxsize=None)
def scoring_list():
    rng = random.Random(12)
    pairs = []
    for k in range(200):   # 150 pairs of 50 .. 150 symbols, 50 that climb to 400; every divergence step at every length class
        n = 50 + (7 * k * k) % 101 if k < 150 else 155 + 5 * (k - 150)
        p = rand_seq(rng, n)
        pairs.append((p, mutate(rng, p, 0.15 * (k % 16) / 15)))
    assert min(len(p) for p, _ in pairs) == 50 and max(len(p) for p, _ in pairs) == 400
    return pairs


@pytest.mark.parametrize("sc", [(1, -1, 0, -1), (5, -4, -16, -4), (0, -4, -6, -2)])
def test_scorings_on_a_ragged_list(ctx, sc):
    pairs = scoring_list()
    want = oracle(pairs, sc)
    if sc == (0, -4, -6, -2):
        assert WO.penalties(*sc) == (2, 3, 1, 4)   # g = 4: the reduction
    check(ctx, pairs, sc, None, want)
    dp = GO.align_many(pairs[::20], "nw", sc[:2], sc[2], sc[3], want_ops=False)
    assert [w["score"] for w in want[::20]] == [d["score"] for d in dp]


def test_a_ring_deeper_than_64_scores_reads_the_markers(ctx):
    """1/-40/-6/-1: x, o, e = 82, 12, 3, so the sweep looks 82 scores back: beyond the 64 whose emptiness it keeps in a register, it
    reads the markers of the skipped wavefronts instead -- in the ring of the score form and in the stored wavefronts alike"""
    sc = (1, -40, -6, -1)
    assert WO.penalties(*sc) == (82, 12, 3, 1)
    pairs = scoring_list()[3:200:5]
    want = oracle(pairs, sc)
    assert max(w["penalty"] for w in want) > 3 * 82
    check(ctx, pairs, sc, None, want)
    best = [w["score"] for w in want]
    check(ctx, pairs[:12], sc, [b + (k % 2) for k, b in enumerate(best[:12])])   # every second pair one above its optimum: not found


# ------------------------------------------------------------------ errors
def test_invalid_scorings_and_indices(ctx, pkg):
    seqs = [b"ACGT", b"ACGA"]
    for bad in [(1, 1, -1, -1), (0, -1, -1, 0), (1, 0, 1, -1), (1, 0, -1, 1)]:
        for call in (ctx.scores_wfa, ctx.align_wfa_batch, ctx.align_wfa_batch_cigar):
            with pytest.raises(pkg.PwaError):
                call(seqs, [0], [1], *bad)
    ctx.scores_wfa(seqs, [0], [1], *SC)
    before = ctx.align_wfa_stats()
    for pa, pb in [([2], [0]), ([0], [7]), ([0, 0], [1, 2])]:
        for call in (ctx.scores_wfa, ctx.align_wfa_batch, ctx.align_wfa_batch_cigar):
            with pytest.raises(pkg.PwaError):
                call(seqs, pa, pb, *SC)
    assert ctx.align_wfa_stats() == before   # a call that fails validation leaves the stats alone


def test_string_capacity_protocol(ctx, pkg):
    L = pkg.lib()
    rng = random.Random(13)
    pairs = [(p, mutate(rng, p, 0.1)) for p in (rand_seq(rng, 80) for _ in range(6))]
    seqs, pa, pb = flatten(pairs)
    full = ctx.align_wfa_batch_cigar(seqs, pa, pb, *SC)
    need_c, need_m = sum(len(r["cigar"]) for r in full), sum(len(r["mdz"]) for r in full)
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa)
    a, b = (C.c_uint32 * n)(*pa), (C.c_uint32 * n)(*pb)
    sc = (C.c_int32 * n)()
    co, mo, need = (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))(), (C.c_uint64 * 2)()
    for cap_c, cap_m, rc in [(need_c - 1, need_m, CAPACITY), (need_c, need_m - 1, CAPACITY), (0, 0, CAPACITY), (need_c, need_m, 0)]:
        cg, md = C.create_string_buffer(max(cap_c, 1)), C.create_string_buffer(max(cap_m, 1))
        need[0] = need[1] = 0
        got = L.pwa_align_wfa_batch_cigar(ctx._h, *SC, blob, off, len(seqs), a, b, n, sc, cg, cap_c, co, md, cap_m, mo, need, None)
        assert got == rc and (need[0], need[1]) == (need_c, need_m)
    assert cg.raw[:need_c] == b"".join(r["cigar"] for r in full) and md.raw[:need_m] == b"".join(r["mdz"] for r in full)
    assert L.pwa_align_wfa_batch_cigar(ctx._h, *SC, blob, off, len(seqs), a, b, n, sc, None, 8, co, md, need_m, mo, need, None) == INVALID
