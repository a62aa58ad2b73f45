"""Semi-global wavefront alignments on the GPU (pwa_scores_wfa_sg, pwa_align_wfa_sg_batch(_cigar), pwa_wfa_last_stats) against
wfa_sg_oracle.py: scores, penalties, end and start cells, op lists byte for byte, the strings, the stats' cells, the bound and the
not-found sentinel, at the smallest shapes at which each mechanism of the SG form of the kernels can go wrong; scores and end cells
against the DP oracle (gotoh_oracle, mode sg) as well, and reads above the DP calls' 1024 rows against the banded score pass."""
import ctypes as C
import functools
import random

import pytest

import gotoh_oracle as GO
import test_gpu_wfa as TW
import wfa_sg_oracle as SO
from conftest import load_pkg, switched_context

pytestmark = pytest.mark.gpu

SC = (1, -4, -6, -1)    # x, o, eI, eD = 5, 6, 1, 2
SC0 = (0, -4, -6, -2)   # match = 0: x, o, eI, eD = 2, 3, 1, 1 with g = 2
INVALID, CAPACITY = -1, -5
rand_seq, mutate, flatten, strings_of = TW.rand_seq, TW.mutate, TW.flatten, TW.strings_of


def oracle(pairs, sc, bounds=None):
    return [SO.align(p, t, *sc, min_score=None if bounds is None else bounds[k]) for k, (p, t) in enumerate(pairs)]


def check(c, pairs, sc, bounds=None, want=None, front=()):
    """every call on one list against the oracle's results `want` -> (alignments, stats of the alignment call)"""
    pkg = load_pkg()
    want = want or oracle(pairs, sc, bounds)
    seqs, pa, pb = flatten(pairs, front)
    cells = sum(w["cells"] for w in want)
    scores, pens, ends = c.scores_wfa_sg(seqs, pa, pb, *sc, min_score=bounds, want_penalty=True, want_end=True)
    assert scores == [w["score"] for w in want]
    assert pens == [w["penalty"] for w in want]
    assert ends == [w["end"] for w in want]
    assert c.align_wfa_stats()["cells"] == cells
    al = c.align_wfa_sg_batch(seqs, pa, pb, *sc, min_score=bounds)
    st = c.align_wfa_stats()
    assert st["cells"] == cells
    cg = c.align_wfa_sg_batch_cigar(seqs, pa, pb, *sc, min_score=bounds)
    assert c.align_wfa_stats()["cells"] == cells
    for k, ((p, t), w) in enumerate(zip(pairs, want)):
        assert al[k] == dict(score=w["score"], ops=w["ops"], end=w["end"], start=w["start"]), (k, p, t)
        assert (cg[k]["score"], cg[k]["end"], cg[k]["start"]) == (w["score"], w["end"], w["start"]), k
        if w["score"] is None:
            assert (cg[k]["cigar"], cg[k]["mdz"]) == (b"", b""), k
            continue
        assert (cg[k]["cigar"], cg[k]["mdz"]) == strings_of(p, t[w["start"][1]:], w["ops"]), k
        if 0 not in p and 0 not in t:
            f = pkg.format_alignment(p, t, w["ops"], w["end"])
            assert (cg[k]["cigar"], cg[k]["mdz"]) == (f["cigar"], f["mdz"]), k
    return al, st


def against_the_dp(pairs, sc, want):
    dp = GO.align_many(pairs, "sg", sc[:2], sc[2], sc[3], want_ops=False)
    assert [(w["score"], w["end"]) for w in want] == [(d["score"], d["end"]) for d in dp]


# ------------------------------------------------------------------ empty and trivial
def test_empty_and_trivial_pairs(ctx):
    pairs = [(b"", b""), (b"", b"ACG"), (b"ACGTA", b""), (b"A", b"A"), (b"A", b"C"), (b"A", b""), (b"ACGTACGTAC", b"ACGTAC"), (b"ACGTACGTAC", b"ACGTACGTAC"),
             (b"ACGTACGTAC", b"TTACGTACGTACTT"), (b"ACGTACGTAC", b"ACGTTCGTAC"), (b"GGGG", b"ACGGTGGAC")]
    want = oracle(pairs, SC)
    al, _ = check(ctx, pairs, SC, want=want)
    against_the_dp(pairs, SC, want)
    assert [a["ops"] for a in al[:4]] == [b"", b"", b"DDDDD", b"M"]
    assert [a["score"] for a in al[:8]] == [0, 0, -11, 1, -4, -7, -4, 10]
    assert [(a["end"], a["start"]) for a in al[:4]] == [((0, 0), (0, 0)), ((0, 0), (0, 0)), ((5, 0), (0, 0)), ((1, 1), (0, 0))]
    assert b"D" in al[6]["ops"] and al[6]["end"][0] == 10            # n > m needs deletions
    assert (al[7]["ops"], al[7]["end"], al[7]["start"]) == (b"M" * 10, (10, 10), (0, 0))
    assert (al[8]["ops"], al[8]["end"], al[8]["start"]) == (b"M" * 10, (10, 12), (0, 2))
    assert ctx.scores_wfa_sg([b"A"], [], [], *SC) == [] and ctx.align_wfa_sg_batch([b"A"], [], [], *SC) == []
    assert ctx.align_wfa_sg_batch_cigar([b"A"], [], [], *SC) == []
    check(ctx, [(b"", b"")], SC)                               # both sides empty, alone in its launch
    check(ctx, [(b"", b""), (b"A", b"A")], SC, bounds=[1, 2])   # nothing for the device to do at all


# ------------------------------------------------------------------ the end diagonal in every lane chunk and on every chunk edge
def planted(rng, m, read, at):
    t = bytearray(rand_seq(rng, m, b"AC"))   # the read is over GT: it occurs nowhere else
    for a in at:
        t[a:a + len(read)] = read
    return bytes(t)


def test_an_exact_occurrence_at_every_chunk_edge(ctx):
    rng = random.Random(31)
    read = rand_seq(rng, 20, b"GT")
    at = [0, 1, 62, 63, 64, 65, 127, 128, 180]
    pairs = [(read, planted(rng, 200, read, [a])) for a in at]
    al, _ = check(ctx, pairs, SC)
    assert [(a["score"], a["ops"], a["start"], a["end"]) for a in al] == [(20, b"M" * 20, (0, a), (20, a + 20)) for a in at]


def test_of_two_occurrences_the_lower_end_wins(ctx):
    rng = random.Random(32)
    read = rand_seq(rng, 20, b"GT")
    twice = [(3, 30), (5, 70), (60, 130), (63, 64 + 20), (0, 180), (100, 150)]   # in one chunk, in two, on the edges
    pairs = [(read, planted(rng, 200, read, at)) for at in twice]
    want = oracle(pairs, SC)
    al, _ = check(ctx, pairs, SC, want=want)
    against_the_dp(pairs, SC, want)
    assert [(a["start"], a["end"]) for a in al] == [((0, lo), (20, lo + 20)) for lo, _ in twice]


# ------------------------------------------------------------------ mismatches, 'I' runs and 'D' runs of 1 .. 5
@functools.lru_cache(maxsize=None)
def edited():
    rng = random.Random(33)
    t = rand_seq(rng, 150)
    pairs = []
    for L in range(1, 6):
        sub = bytes(b"ACGT"[(b"ACGT".index(c) + 1) % 4] for c in t[70:70 + L])
        pairs.append((t[40:70] + sub + t[70 + L:100], t))                  # L mismatches
        pairs.append((t[40:70] + t[70 + L:100 + L], t))                    # an 'I' run: L text symbols against a gap
        pairs.append((t[40:70] + rand_seq(rng, L, b"N") + t[70:100], t))   # a 'D' run: L pattern symbols against a gap
    pairs.append((b"NNN" + t[:50], t))             # starts with 'D': the span grows to the left of diagonal 0
    pairs.append((t[100:] + b"NNNN", t))           # hangs over the text's end: diagonals above m - n, and back by 'D'
    pairs.append((b"NN" + t + b"NNN", t))          # both at once, n > m
    return pairs


@pytest.mark.parametrize("sc", [SC, SC0])
def test_planted_edits_of_every_kind(ctx, sc):
    pairs = edited()
    want = oracle(pairs, sc)
    al, _ = check(ctx, pairs, sc, want=want)
    against_the_dp(pairs, sc, want)
    for L in range(1, 6):
        mis, ins, dele = al[3 * L - 3:3 * L]
        assert (mis["start"], mis["end"]) == ((0, 40), (60, 100))
        assert mis["ops"] == b"M" * 60 or L == 5   # (five mismatches in a row tie with a pair of gaps around chance matches)
        assert ins["ops"].count(b"I") == L and dele["ops"].count(b"D") == L, L
    assert al[15]["ops"].endswith(b"DDD") and al[15]["start"] == (0, 0)
    assert al[16]["ops"].startswith(b"DDDD") and al[16]["end"] == (54, 150)
    assert al[17]["ops"] == b"DDD" + b"M" * 150 + b"DD"
    if sc == SC:
        assert SO.penalties(*sc)[2:4] == (1, 2)   # eI != eD
    else:
        assert SO.penalties(*sc)[2:4] == (1, 1)


def test_gap_runs_across_the_lane_chunks(ctx):
    rng = random.Random(34)
    p = rand_seq(rng, 300)
    pairs = []
    for run in (31, 32, 33, 63, 64, 65, 127, 128, 129, 130):
        pairs.append((p, rand_seq(rng, 7) + p[:150] + rand_seq(rng, run, b"N") + p[150:] + rand_seq(rng, 9)))
        pairs.append((p[:150] + rand_seq(rng, run, b"N") + p[150:], rand_seq(rng, 70) + p))
    want = oracle(pairs, SC)
    al, _ = check(ctx, pairs, SC, want=want)
    against_the_dp(pairs[::3], SC, want[::3])
    assert all(b"I" * 31 in a["ops"] for a in al[::2]) and all(b"D" * 31 in a["ops"] for a in al[1::2])


# ------------------------------------------------------------------ the extend: every byte alignment, the blob's last byte, any byte value
def test_match_runs_at_every_blob_offset_and_the_last_byte(ctx):
    rng = random.Random(35)
    p, t = bytearray(), bytearray()
    for run in list(range(21)) + list(range(20, -1, -1)):
        s = rand_seq(rng, run, b"GT")
        p += s + b"A"
        t += s + b"C"
    p, t = bytes(p), b"AC" + bytes(t) + b"CAC"
    sc = (1, -1, -3, -2)
    want = SO.align(p, t, *sc)
    assert want["ops"] == b"M" * len(p) and want["start"] == (0, 2)
    seqs, at, offsets = [], 0, set()
    for d in range(8):   # the pattern at offset d mod 8
        seqs += [b"x" * ((d - sum(len(s) for s in seqs)) % 8), p, t]
    for s in seqs:
        if s in (p, t):
            offsets.add(at % 8)
        at += len(s)
    assert offsets == set(range(8))
    pa, pb = [3 * d + 1 for d in range(8)], [3 * d + 2 for d in range(8)]
    assert ctx.align_wfa_sg_batch(seqs, pa, pb, *sc) == [dict(score=want["score"], ops=want["ops"], end=want["end"], start=want["start"])] * 8
    long_run = rand_seq(rng, 61)   # runs ended by the clamp, the text the last sequence of the blob
    ends = [(long_run[:29], long_run), (long_run, long_run[:29]), (long_run[5:], long_run), (long_run[30:] + b"ACGT", long_run)]
    check(ctx, ends, SC, front=[b"xyz"])
    s = rand_seq(rng, 45)   # back to back copies: an extend that ignores the lengths runs on into the neighbour
    assert [a["ops"] for a in ctx.align_wfa_sg_batch([s, s, s], [0, 1, 0, 2, 1], [1, 2, 2, 0, 1], *SC)] == [b"M" * 45] * 5


def test_match_runs_across_the_replay_step(ctx):
    """pass B extends 512 symbols per step of the 64 lanes: runs of 511 .. 1300 matches from a start cell inside the text, ended by the
    pattern's end, by the text's end and by a mismatch"""
    rng = random.Random(36)
    big = rand_seq(rng, 1300)
    pairs = [(big[:L], b"TTG" + big[:L] + b"CA") for L in (511, 512, 513, 1023, 1024, 1025, 1300)]
    pairs += [(big, big), (big[:700] + b"A" + big[701:], b"GG" + big[:700] + b"C" + big[701:]), (big[:513] + b"NN", b"ACGT" * 3 + big[:513])]
    bounds = [len(p) - 40 for p, _ in pairs]
    al, _ = check(ctx, pairs, SC, bounds)
    assert [a["ops"] for a in al[:8]] == [b"M" * len(p) for p, _ in pairs[:8]]
    assert al[9]["ops"] == b"DD" + b"M" * 513


def test_bytes_nul_dash_and_ff(ctx):
    rng = random.Random(37)
    alphabet = b"\x00-\xffA"
    pairs = []
    for n in (1, 7, 8, 9, 60, 150):
        p = rand_seq(rng, n, alphabet)
        t = rand_seq(rng, 11, alphabet) + mutate(rng, p, 0.15, alphabet) + rand_seq(rng, 5, alphabet)
        pairs += [(p, t), (p, rand_seq(rng, n + 3, alphabet)), (b"\x00" * n, b"\x00" * (n + 1)), (b"\xff" * n, b"-" + b"\xff" * n)]
    want = oracle(pairs, SC)
    check(ctx, pairs, SC, want=want)
    against_the_dp(pairs, SC, want)


# ------------------------------------------------------------------ the ring: the register history, the markers, g > 1
@functools.lru_cache(maxsize=None)
def ragged():
    """200 reads of 30 .. 300 symbols in regions of 1 .. 3 times their length, 0 .. 20 % mutated"""
    rng = random.Random(38)
    pairs = []
    for k in range(200):
        n = 30 + (270 * k) // 199
        m = n * (1 + k % 3) + (k % 7 if k % 3 else 0)
        t = rand_seq(rng, m)
        at = rng.randint(0, m - n) if k % 3 else 0
        pairs.append((mutate(rng, t[at:at + n], 0.2 * (k % 11) / 10), t))
    assert min(len(p) for p, _ in pairs) <= 31 and max(len(p) for p, _ in pairs) >= 280
    return pairs


@pytest.mark.parametrize("sc", [SC, (5, -4, -16, -4), (3, -3, -9, -3)])
def test_scorings_on_a_ragged_list(ctx, sc):
    pairs = ragged()
    want = oracle(pairs, sc)
    x, o, ei, ed, g = SO.penalties(*sc)
    assert max(x, o + ei, o + ed) + 1 <= 64                     # the emptiness of the sources comes from the register history
    if sc == (3, -3, -9, -3):
        assert (x, o, ei, ed, g) == (2, 3, 1, 2, 3)             # g > 1: the reduction
    check(ctx, pairs, sc, None, want)
    against_the_dp(pairs, sc, want)


@pytest.mark.parametrize("sc", [(1, -40, -6, -1), (1, -70, -6, -1)])
def test_a_deep_ring(ctx, sc):
    """1/-40/-6/-1 looks 41 scores back, 1/-70/-6/-1 71: beyond the 64 whose emptiness the sweep keeps in a register, so it reads the
    markers of the skipped wavefronts in the ring; between two filled wavefronts lie skipped ones whose codes are never written"""
    x, o, ei, ed, g = SO.penalties(*sc)
    assert (x > 63) == (sc[1] == -70)
    pairs = ragged()[3:200:5]
    want = oracle(pairs, sc)
    assert max(w["penalty"] for w in want) > 2 * x
    check(ctx, pairs, sc, None, want)
    against_the_dp(pairs[::4], sc, want[::4])
    best = [w["score"] for w in want]
    check(ctx, pairs[:12], sc, [b + (k % 2) for k, b in enumerate(best[:12])])   # every second pair one above its optimum: not found


# ------------------------------------------------------------------ the bound; ranges; junk in the buffers
@functools.lru_cache(maxsize=None)
def mixed():
    """found pairs, pairs not found on the host (both cases) and by the sweep, empty-sided pairs -> pairs, bounds, the oracle's results"""
    rng = random.Random(39)
    pairs, bounds = [], []
    for n in (40, 90, 200, 330):
        t = rand_seq(rng, n + 57)
        r = t[20:20 + n]
        for p in (mutate(rng, r, 0.08), r[:n // 3] + rand_seq(rng, 9, b"N") + r[n // 3:], r):
            best = SO.align(p, t, *SC, want_ops=False)["score"]
            for b in (best, best + 1, -(1 << 20), None, best - 7):
                pairs.append((p, t))
                bounds.append(b)
    pairs += [(b"", b""), (b"", b""), (b"ACGT", b""), (b"ACGT", b""), (b"", b"AC"), (b"", b"AC"), (b"ACGTAC", b"ACG"), (b"ACGTAC", b"ACG"), (b"ACGTAC", b"ACG")]
    bounds += [0, 1, -10, -9, 0, 1, -6, -5, 7]
    bounds = [-(1 << 30) if b is None else b for b in bounds]   # one list of ints: "no bound" as a bound far below
    want = oracle(pairs, SC, bounds)
    kinds = {(w["score"] is None, w["cells"] > 0) for w in want}
    assert kinds == {(False, True), (True, False), (True, True)}   # found; not found on the host; not found by the sweep
    plan = load_pkg().wfa_sg_plan(*SC, [(len(p), len(t)) for p, t in pairs[-3:]], bounds[-3:])
    assert plan["p_max"][1:] == [None, None]                       # n > m under the forced gap's penalty; a bound above match n
    return pairs, bounds, want


def test_bound_at_above_and_below_the_optimum(ctx):
    pairs, bounds, want = mixed()
    check(ctx, pairs, SC, bounds, want)
    free = oracle(pairs[:15], SC)
    check(ctx, pairs[:15], SC, None, free)                       # None: no bound
    best = [w["score"] for w in free]
    check(ctx, pairs[:15], SC, best)                             # every pair at its optimum
    check(ctx, pairs[:15], SC, [b - 1 for b in best])            # ... one below
    al, _ = check(ctx, pairs[:15], SC, [b + 1 for b in best])    # ... and one above: nothing is found
    assert all(a == dict(score=None, ops=b"", end=(0, 0), start=(0, 0)) for a in al)
    assert ctx.scores_wfa_sg(*flatten(pairs[:15]), *SC, min_score=-(1 << 20)) == best   # one int for every pair


def sizes_of(pkg, pairs, sc, bounds):
    """per pair: (ring bytes, cells) as the header states them; (0, 0) for a pair decided on the host"""
    x, o, ei, ed, g = SO.penalties(*sc)
    plan = pkg.wfa_sg_plan(*sc, [(len(p), len(t)) for p, t in pairs], bounds)
    out = []
    for (p, t), p_max, cells in zip(pairs, plan["p_max"], plan["cells"]):
        out.append((0, 0) if p_max is None else (12 * min(max(x, o + ei, o + ed) + 1, p_max + 1) * SO.width(p_max, len(p), len(t), o, ed), cells))
    return out


def test_ranges_and_poisoned_buffers_change_nothing(ctx, pkg):
    pairs, bounds, want = mixed()
    sizes = [ring + cells + (len(p) + len(t) if ring else 0) for (ring, cells), (p, t) in zip(sizes_of(pkg, pairs, SC, bounds), pairs)]
    budget = max(4096, sum(sizes) // 5)
    assert len(TW.split(sizes, budget)) >= 3 and len(TW.split([s + 16 for s in sizes], budget)) >= 3
    plain, st = check(ctx, pairs, SC, bounds, want)
    with switched_context(PWA_RANGE_BYTES=budget) as c:
        cut, st_cut = check(c, pairs, SC, bounds, want)
        assert cut == plain and st_cut["cells"] == st["cells"] and st_cut["workspace_bytes"] < st["workspace_bytes"]
    for byte in ("0xFF", "0"):
        with switched_context(PWA_POISON=byte) as c:
            assert check(c, pairs, SC, bounds, want)[0] == plain
            assert c.poison_stats()["buffers"] > 0
        with switched_context(PWA_POISON=byte, PWA_RANGE_BYTES=budget) as c:
            assert check(c, pairs, SC, bounds, want)[0] == plain


def test_workspace_is_a_ring_and_one_byte_per_planned_cell(ctx, pkg):
    pairs, bounds, want = mixed()
    sizes = sizes_of(pkg, pairs, SC, bounds)
    seqs, pa, pb = flatten(pairs)
    ctx.align_wfa_sg_batch(seqs, pa, pb, *SC, min_score=bounds)
    got = ctx.align_wfa_stats()["workspace_bytes"]
    low, high = sum(ring + cells for ring, cells in sizes), sum(ring + cells + 16 for ring, cells in sizes if ring)
    print("sg codes workspace %d B in [%d, %d]" % (got, low, high))
    assert low <= got <= high
    ctx.scores_wfa_sg(seqs, pa, pb, *SC, min_score=bounds)
    assert ctx.align_wfa_stats()["workspace_bytes"] == sum(ring for ring, _ in sizes)


# ------------------------------------------------------------------ reads above the DP calls' 1024 rows
def test_eight_reads_of_two_thousand_symbols(ctx, pkg):
    """no oracle DP at this size: scores and end cells against the banded score pass on the band [-600, m - n + 600].  That band holds
    every start 0 .. m - n of the region with 600 diagonals to spare on each side; an alignment that leaves it has gap runs of more
    than 600 symbols net, which scores below -600 while the planted read scores above 1500, so the banded optimum is the exact one."""
    rng = random.Random(40)
    pairs = []
    for k in range(8):
        t = rand_seq(rng, 2600 + 3 * k)
        at = rng.randint(0, 600)
        pairs.append((mutate(rng, t[at:at + 2000], 0.02), t))
    seqs, pa, pb = flatten(pairs)
    bands = [(-600, len(t) - len(p) + 600) for p, t in pairs]
    banded, end_i, end_j = ctx.scores_banded("sg", seqs, pa, pb, *SC, bands, want_end=True)
    assert min(banded) > 1500
    bounds = [s - 60 for s in banded]
    scores, ends = ctx.scores_wfa_sg(seqs, pa, pb, *SC, min_score=bounds, want_end=True)
    assert scores == list(banded) and ends == list(zip(end_i, end_j))
    al = ctx.align_wfa_sg_batch(seqs, pa, pb, *SC, min_score=bounds)
    for k, ((p, t), a) in enumerate(zip(pairs, al)):
        assert (a["score"], a["end"]) == (scores[k], ends[k])
        (i0, j0), (i1, j1) = a["start"], a["end"]
        assert i0 == 0 and i1 == len(p)
        assert (a["ops"].count(b"M") + a["ops"].count(b"D"), a["ops"].count(b"M") + a["ops"].count(b"I")) == (len(p), j1 - j0)
        assert GO.op_score(p, t, a["ops"], a["start"], SC[:2], SC[2], SC[3]) == scores[k]
    with pytest.raises(pkg.PwaError, match="(?i)capacity|rows|1024"):
        ctx.align_gotoh_batch("sg", seqs, pa, pb, *SC)


# ------------------------------------------------------------------ errors and the strings' protocol
def raw_call(pkg, ctx, name, seqs, pa, pb, sc):
    L = pkg.lib()
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa)
    a, b = (C.c_uint32 * max(n, 1))(*pa), (C.c_uint32 * max(n, 1))(*pb)
    score = (C.c_int32 * max(n, 1))()
    cells = [(C.c_uint64 * max(2 * n, 1))(), (C.c_uint64 * max(2 * n, 1))()] if "_sg_" in name else []
    if name.endswith("_cigar"):
        cg, md, co, mo = C.create_string_buffer(4096), C.create_string_buffer(4096), (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))()
        return getattr(L, name)(ctx._h, *sc, blob, off, len(seqs), a, b, n, score, cg, 4096, co, md, 4096, mo, *cells, None, None)
    ops, ooff, nops = C.create_string_buffer(4096), (C.c_uint64 * max(n, 1))(), (C.c_uint64 * max(n, 1))()
    return getattr(L, name)(ctx._h, *sc, blob, off, len(seqs), a, b, n, score, ops, ooff, nops, *cells, None)


def test_validation_results_and_order_are_the_global_codes_calls(ctx, pkg):
    seqs = [b"ACGT", b"ACGA", b"A" * 300]
    wide = (1, -(1 << 20), -6, -1)   # the range rule: (n + m + 2) 2^20 < 2^28 holds for the short pairs only
    cases = [(seqs, [0], [1], SC, 0), (seqs, [0], [1], (1, 1, -1, -1), INVALID), (seqs, [3], [1], (1, 1, -1, -1), INVALID), (seqs, [3], [1], SC, INVALID),
             (seqs, [0], [9], SC, INVALID), (seqs, [0], [1], wide, 0), (seqs, [0], [2], wide, CAPACITY), (seqs, [0, 0], [2, 7], wide, CAPACITY),
             (seqs, [0, 0], [7, 2], wide, INVALID), (seqs, [], [], SC, 0)]
    ctx.scores_wfa_sg(seqs, [0], [1], *SC)
    for old, new in [("pwa_align_wfa_codes_batch", "pwa_align_wfa_sg_batch"), ("pwa_align_wfa_codes_batch_cigar", "pwa_align_wfa_sg_batch_cigar")]:
        for s, pa, pb, sc, rc in cases:
            if rc:
                before = ctx.align_wfa_stats()
            assert raw_call(pkg, ctx, new, s, pa, pb, sc) == raw_call(pkg, ctx, old, s, pa, pb, sc) == rc, (new, pa, pb, sc)
            if rc:
                assert ctx.align_wfa_stats() == before   # a call that fails validation leaves the stats alone
    for bad in [(1, 1, -1, -1), (1, -1, -1, 0), (-1, -3, 0, -1), (1, 0, 1, -1)]:
        for call in (ctx.scores_wfa_sg, ctx.align_wfa_sg_batch, ctx.align_wfa_sg_batch_cigar):
            with pytest.raises(pkg.PwaError):
                call(seqs, [0], [1], *bad)


def test_string_capacity_protocol(ctx, pkg):
    L = pkg.lib()
    rng = random.Random(41)
    pairs = [(mutate(rng, t[9:89], 0.1), t) for t in (rand_seq(rng, 120) for _ in range(6))]
    seqs, pa, pb = flatten(pairs)
    full = ctx.align_wfa_sg_batch_cigar(seqs, pa, pb, *SC)
    ops = ctx.align_wfa_sg_batch(seqs, pa, pb, *SC)
    for (p, t), r, a in zip(pairs, full, ops):
        f = pkg.format_alignment(p, t, a["ops"], a["end"])
        assert (r["cigar"], r["mdz"], r["end"], r["start"]) == (f["cigar"], f["mdz"], a["end"], a["start"])
    need_c, need_m = sum(len(r["cigar"]) for r in full), sum(len(r["mdz"]) for r in full)
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa)
    a, b = (C.c_uint32 * n)(*pa), (C.c_uint32 * n)(*pb)
    sc = (C.c_int32 * n)()
    co, mo, need = (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))(), (C.c_uint64 * 2)()
    for cap_c, cap_m, rc in [(need_c - 1, need_m, CAPACITY), (need_c, need_m - 1, CAPACITY), (0, 0, CAPACITY), (need_c, need_m, 0)]:
        cg, md = C.create_string_buffer(max(cap_c, 1)), C.create_string_buffer(max(cap_m, 1))
        need[0] = need[1] = 0
        got = L.pwa_align_wfa_sg_batch_cigar(ctx._h, *SC, blob, off, len(seqs), a, b, n, sc, cg, cap_c, co, md, cap_m, mo, None, None, need, None)
        assert got == rc and (need[0], need[1]) == (need_c, need_m)
    assert cg.raw[:need_c] == b"".join(r["cigar"] for r in full) and md.raw[:need_m] == b"".join(r["mdz"] for r in full)
    assert L.pwa_align_wfa_sg_batch_cigar(ctx._h, *SC, blob, off, len(seqs), a, b, n, sc, None, 8, co, md, need_m, mo, None, None, need, None) == INVALID
