"""The codes form of the wavefront alignments on the GPU (pwa_align_wfa_codes_batch(_cigar): a ring sweep plus one code byte per planned
cell, a two-pass walk) against the offsets form (pwa_align_wfa_batch(_cigar)), which it must equal byte for byte -- op lists, scores,
op counts, CIGAR and MD:Z -- and against wfa_oracle.py where that is cheap; the workspace it reports against the plan."""
import ctypes as C
import random

import pytest

import test_gpu_wfa as TW
import wfa_oracle as WO
from conftest import switched_context

pytestmark = pytest.mark.gpu

SC = TW.SC
INVALID, CAPACITY = -1, -5
rand_seq, mutate, flatten = TW.rand_seq, TW.mutate, TW.flatten


def both(c, pairs, sc, bounds=None, want=None, front=()):
    """the two forms of both calls on one list: equal in everything, and equal to the oracle's results `want` where given
    -> (alignments, stats of the codes call, stats of the offsets call)"""
    seqs, pa, pb = flatten(pairs, front)
    off = c.align_wfa_batch(seqs, pa, pb, *sc, min_score=bounds)
    st_off = c.align_wfa_stats()
    cod = c.align_wfa_batch(seqs, pa, pb, *sc, min_score=bounds, form="codes")
    st_cod = c.align_wfa_stats()
    assert len(cod) == len(pairs)
    for k, (a, b) in enumerate(zip(cod, off)):
        assert a == b, (k, pairs[k])
    assert st_cod["cells"] == st_off["cells"]
    cg_off = c.align_wfa_batch_cigar(seqs, pa, pb, *sc, min_score=bounds)
    cg_cod = c.align_wfa_batch_cigar(seqs, pa, pb, *sc, min_score=bounds, form="codes")
    assert c.align_wfa_stats()["cells"] == st_off["cells"]
    for k, (a, b) in enumerate(zip(cg_cod, cg_off)):
        assert a == b, (k, pairs[k])
    for k, a in enumerate(cod):
        if a["score"] is None:
            assert (a["ops"], cg_cod[k]["cigar"], cg_cod[k]["mdz"]) == (b"", b"", b""), k
    if want is not None:
        assert [(a["score"], a["ops"]) for a in cod] == [(w["score"], w["ops"]) for w in want]
        assert st_cod["cells"] == sum(w["cells"] for w in want)
    return cod, st_cod, st_off


def test_the_form_argument(ctx):
    seqs = [b"ACGTACGT", b"ACGAACGT"]
    for call in (ctx.align_wfa_batch, ctx.align_wfa_batch_cigar):
        assert call(seqs, [0], [1], *SC, form="codes") == call(seqs, [0], [1], *SC, form="offsets") == call(seqs, [0], [1], *SC)
        for bad in ("code", "", None):
            with pytest.raises(ValueError):
                call(seqs, [0], [1], *SC, form=bad)


def test_empty_and_trivial_pairs(ctx):
    pairs = [(b"", b""), (b"ACGTA", b""), (b"", b"ACG"), (b"ACGTACGTAC", b"ACGTACGTAC"), (b"ACGTACGTAC", b"ACGTTCGTAC"),
             (b"ACGTACGTAC", b"ACGTCGTAC"), (b"ACGTCGTAC", b"ACGTACGTAC"), (b"A", b"C"), (b"A", b"A"), (b"A", b""), (b"", b"T")]
    al, _, _ = both(ctx, pairs, SC, want=TW.oracle(pairs, SC))
    assert [a["ops"] for a in al[:4]] == [b"", b"DDDDD", b"III", b"M" * 10]
    assert ctx.align_wfa_batch([b"A"], [], [], *SC, form="codes") == [] and ctx.align_wfa_batch_cigar([b"A"], [], [], *SC, form="codes") == []
    both(ctx, [(b"", b"")], SC, want=TW.oracle([(b"", b"")], SC))          # both sides empty, alone in its launch
    both(ctx, [(b"", b""), (b"", b"")], SC, bounds=[1, 1])                   # nothing for the device to do at all


def test_gap_runs_across_the_lane_chunks(ctx):
    rng = random.Random(21)
    p = rand_seq(rng, 300)
    pairs = []
    for run in (31, 32, 33, 63, 64, 65, 127, 128, 129, 130):
        at = rng.randint(40, 120)
        pairs.append((p, p[:at] + rand_seq(rng, run) + p[at:]))
        pairs.append((p, p[:at] + p[at + run:]))
    al, _, _ = both(ctx, pairs, SC)
    want = TW.oracle(pairs[::5], SC)
    assert [(a["score"], a["ops"]) for a in al[::5]] == [(w["score"], w["ops"]) for w in want]


def test_match_runs_of_every_length_at_every_blob_offset(ctx):
    """pass B's extend: runs of 0 .. 20 matches between mismatches, the pair at every offset mod 8 of the blob, so every run starts at
    every byte alignment of the 8-byte compare; then runs that are ended by the clamp, on the blob's last byte"""
    rng = random.Random(22)
    p, t = bytearray(), bytearray()
    for run in list(range(21)) + list(range(20, -1, -1)):
        s = rand_seq(rng, run, b"GT")
        p += s + b"A"
        t += s + b"C"
    p, t = bytes(p), bytes(t)
    sc = (1, -1, -3, -2)
    want = WO.align(p, t, *sc)
    assert want["ops"] == b"M" * len(p)
    seqs, at, offsets = [], 0, set()
    for d in range(8):   # the pattern at offset d mod 8
        seqs += [b"x" * ((d - sum(len(s) for s in seqs)) % 8), p, t]
    for s in seqs:
        if s in (p, t):
            offsets.add(at % 8)
        at += len(s)
    assert offsets == set(range(8))
    pa, pb = [3 * d + 1 for d in range(8)], [3 * d + 2 for d in range(8)]
    for form in ("offsets", "codes"):
        assert [a["ops"] for a in ctx.align_wfa_batch(seqs, pa, pb, *sc, form=form)] == [want["ops"]] * 8
    trimmed = [(p[:-1], t[:-1]), (p[3:], t[3:]), (p[5:], t[2:])]
    both(ctx, trimmed, sc, want=TW.oracle(trimmed, sc))
    long_run = rand_seq(rng, 61)
    ends = [(long_run[:29], long_run), (long_run, long_run[:29]), (long_run[5:], long_run)]
    both(ctx, ends, SC, want=TW.oracle(ends, SC), front=[b"xyz"])
    s = rand_seq(rng, 45)   # back to back copies: an extend that ignores the lengths runs on into the neighbour
    seqs = [s, s, s]
    for form in ("offsets", "codes"):
        assert [a["ops"] for a in ctx.align_wfa_batch(seqs, [0, 1, 0, 2, 1], [1, 2, 2, 0, 1], *SC, form=form)] == [b"M" * 45] * 5
    # a run longer than one step of the 64 lanes (512 symbols), ended by a mismatch, by the clamp, and at exactly 512 and 1024
    big = rand_seq(rng, 1300)
    runs = [(big, big), (big[:512], big[:512]), (big[:1024], big[:1024] + b"A"), (big[:700] + b"A" + big[701:], big[:700] + b"C" + big[701:]),
            (big[:511], big[:513]), (big[:513], big[:511])]
    both(ctx, runs, SC, want=TW.oracle(runs, SC))


def test_bytes_nul_dash_and_ff(ctx):
    rng = random.Random(23)
    alphabet = b"\x00-\xffA"
    pairs = []
    for n in (1, 7, 8, 9, 60, 150):
        p = rand_seq(rng, n, alphabet)
        pairs += [(p, mutate(rng, p, 0.15, alphabet)), (p, rand_seq(rng, n + 3, alphabet)), (b"\x00" * n, b"\x00" * (n + 1))]
    both(ctx, pairs, SC, want=TW.oracle(pairs, SC))


def test_crafted_ties(ctx):
    """what test_wfa_codes_oracle.py proves for the restatement, on the kernels: all three sources of M tied, an I run next to a D
    run, a gap next to a mismatch, a gap whose open and extend tie"""
    rng = random.Random(24)
    left, right = rand_seq(rng, 30, b"AC"), rand_seq(rng, 25, b"AC")
    homo = [(b"A" * n, b"A" * m) for n, m in [(10, 13), (13, 9), (1, 6), (6, 1), (40, 41), (7, 7), (70, 140)]]
    for sc in [SC, (1, -1, 0, -1), (5, -4, -16, -4), (0, -4, -6, -2), (1, -40, -6, -1)]:
        both(ctx, homo, sc, want=TW.oracle(homo, sc))
    blocks = [(left + a + right, left + b + right) for a, b in [(b"TTT", b"GG"), (b"GG", b"TTT"), (b"T", b"G"), (b"TTTTT", b"GGGGG")]]
    al, _, _ = both(ctx, blocks, (1, -40, -6, -1), want=TW.oracle(blocks, (1, -40, -6, -1)))
    assert any(b"ID" in a["ops"] or b"DI" in a["ops"] for a in al)
    beside = [(left + b"T" + right, left + b"GGGG" + right), (left + b"TGGG" + right, left + b"C" + right), (left + b"TT" + right, left + b"G" + right),
              (b"T" + right, b"GGG" + right), (left + b"T", left + b"GGG")]
    beside += [(t, p) for p, t in beside]
    for sc in [SC, (5, -4, -16, -4), (1, -1, 0, -1)]:
        both(ctx, beside, sc, want=TW.oracle(beside, sc))
    ties = [((1, -1, 0, -1), left + right, left + b"GGGG" + right), ((1, -1, 0, -1), left + b"TTTTT" + right, left + right),
            ((1, -1, 0, -1), b"ACACACACAC", b"ACACACACACACAC"), (SC, b"ACACACACACACACAC" * 2, b"ACACACACAC" * 2), (SC, b"AAAA", b"CCCCCCCCC"),
            ((5, -4, -16, -4), b"ACAA", b"CCGGCGCCC"), ((1, -40, -6, -1), b"ACAA", b"CCGGCGCCC"), ((0, -4, -6, -2), b"GTGTGTGTGTGTGTGTGT", b"GTGTGTGTGT")]
    for sc, p, t in ties:
        both(ctx, [(p, t), (t, p)], sc, want=TW.oracle([(p, t), (t, p)], sc))


def test_bound_at_above_and_below_the_optimum(ctx):
    pairs, bounds, want = TW.mixed()
    both(ctx, pairs, SC, bounds, want)
    free = TW.oracle(pairs[:12], SC)
    both(ctx, pairs[:12], SC, None, free)
    best = [w["score"] for w in free]
    both(ctx, pairs[:12], SC, best)
    al, _, _ = both(ctx, pairs[:12], SC, [b + 1 for b in best])
    assert all(a["score"] is None and a["ops"] == b"" for a in al)


@pytest.mark.parametrize("sc", [(1, -1, 0, -1), (5, -4, -16, -4), (0, -4, -6, -2)])
def test_scorings_on_a_ragged_list(ctx, sc):
    pairs = TW.scoring_list()
    al, _, _ = both(ctx, pairs, sc)
    want = TW.oracle(pairs[::8], sc)
    assert [(a["score"], a["ops"]) for a in al[::8]] == [(w["score"], w["ops"]) for w in want]


def test_a_ring_deeper_than_64_scores(ctx):
    """1/-40/-6/-1: x, o, e = 82, 12, 3, a ring of 83 wavefronts: the sweep reads the markers in the ring, and between two filled
    wavefronts lie skipped ones whose code bytes are never written and never read"""
    sc = (1, -40, -6, -1)
    pairs = TW.scoring_list()[3:200:5]
    al, _, _ = both(ctx, pairs, sc)
    want = TW.oracle(pairs[::4], sc)
    assert [(a["score"], a["ops"]) for a in al[::4]] == [(w["score"], w["ops"]) for w in want]
    assert max(w["penalty"] for w in want) > 3 * 82
    best = [a["score"] for a in al[:12]]
    cut, _, _ = both(ctx, pairs[:12], sc, [b + (k % 2) for k, b in enumerate(best)])
    assert [a["score"] is None for a in cut] == [bool(k % 2) for k in range(12)]


def codes_sizes(pkg, pairs, sc, bounds):
    """per pair: (ring bytes, cells) as the header states them; (0, 0) for a pair decided on the host"""
    x, o, e, g = WO.penalties(*sc)
    plan = pkg.wfa_plan(*sc, [(len(p), len(t)) for p, t in pairs], bounds)
    out = []
    for (p, t), p_max, cells in zip(pairs, plan["p_max"], plan["cells"]):
        if p_max is None:
            out.append((0, 0))
            continue
        out.append((12 * min(max(x, o + e) + 1, p_max + 1) * WO.width(p_max, len(p), len(t), o, e), cells))
    return out


def test_ranges_and_poisoned_buffers_change_nothing(ctx, pkg):
    pairs, bounds, want = TW.mixed()
    sizes = [ring + cells + (len(p) + len(t) if ring else 0) for (ring, cells), (p, t) in zip(codes_sizes(pkg, pairs, SC, bounds), pairs)]
    budget = max(4096, sum(sizes) // 5)
    assert len(TW.split(sizes, budget)) >= 3 and len(TW.split([s + 16 for s in sizes], budget)) >= 3
    plain, st, _ = both(ctx, pairs, SC, bounds, want)
    with switched_context(PWA_RANGE_BYTES=budget) as c:
        cut, st_cut, _ = both(c, pairs, SC, bounds, want)
        assert cut == plain and st_cut["cells"] == st["cells"] and st_cut["workspace_bytes"] < st["workspace_bytes"]
    for byte in ("0xFF", "0"):
        with switched_context(PWA_POISON=byte) as c:
            assert both(c, pairs, SC, bounds, want)[0] == plain
            assert c.poison_stats()["buffers"] > 0
        with switched_context(PWA_POISON=byte, PWA_RANGE_BYTES=budget) as c:
            assert both(c, pairs, SC, bounds, want)[0] == plain


def test_ranges_without_a_live_pair_change_nothing(ctx, pkg):
    """the first pair and a run of four in the middle carry a bound above any score, so the host rules them out; under a budget of
    about two pairs' op bytes they form ranges of their own in the alignment forms -- the first range among them --, which launch
    nothing, and every result and the cell count stay the uncut call's"""
    rng = random.Random(27)
    dead = {0, 5, 6, 7, 8}
    pairs = []
    for k in range(12):
        p = rand_seq(rng, 60 + 5 * k)
        t = mutate(rng, p, 0.05 + 0.005 * k)
        pairs.append((p, t + rand_seq(rng, max(0, len(p) - len(t)))))   # m >= n: the bound below is above the semi-global scores too
    bounds = [SC[0] * (len(p) + len(t)) // 2 + 1 if k in dead else -(1 << 30) for k, (p, t) in enumerate(pairs)]
    nm = [len(p) + len(t) for p, t in pairs]
    budget = 2 * max(nm)
    # the ranges, on the CPU: a live pair alone exceeds the budget in every form, a pair ruled out weighs its op bytes
    cells = pkg.wfa_plan(*SC, [(len(p), len(t)) for p, t in pairs], bounds)["cells"]
    sg_cells = pkg.wfa_sg_plan(*SC, [(len(p), len(t)) for p, t in pairs], bounds)["cells"]
    by_form = dict(offsets=[12 * c + s for c, s in zip(cells, nm)],
                   codes=[ring + (c + 3) // 4 * 4 + s for (ring, c), s in zip(codes_sizes(pkg, pairs, SC, bounds), nm)],
                   sg=[c + s for c, s in zip(sg_cells, nm)])   # (a lower bound: the ring comes on top)
    for form, sizes in by_form.items():
        assert all((sizes[k] == nm[k]) == (k in dead) for k in range(12)) and min(sizes[k] for k in range(12) if k not in dead) > budget, form
        ranges = TW.split(sizes, budget)
        assert ranges[0] == (0, 1) and sum(all(k in dead for k in range(k0, k1)) for k0, k1 in ranges) >= 3, (form, ranges)
    seqs, pa, pb = flatten(pairs)

    def everything(c):
        out = []
        for call in (lambda: c.align_wfa_batch(seqs, pa, pb, *SC, min_score=bounds), lambda: c.align_wfa_batch(seqs, pa, pb, *SC, min_score=bounds, form="codes"),
                     lambda: c.align_wfa_batch_cigar(seqs, pa, pb, *SC, min_score=bounds), lambda: c.align_wfa_batch_cigar(seqs, pa, pb, *SC, min_score=bounds, form="codes"),
                     lambda: c.align_wfa_sg_batch(seqs, pa, pb, *SC, min_score=bounds), lambda: c.align_wfa_sg_batch_cigar(seqs, pa, pb, *SC, min_score=bounds),
                     lambda: c.scores_wfa(seqs, pa, pb, *SC, min_score=bounds, want_penalty=True),
                     lambda: c.scores_wfa_sg(seqs, pa, pb, *SC, min_score=bounds, want_penalty=True, want_end=True)):
            out.append((call(), c.align_wfa_stats()["cells"]))
        return out

    plain = everything(ctx)
    for res, n_cells in plain[:6]:
        assert [a["score"] is None for a in res] == [k in dead for k in range(12)] and n_cells > 0
    assert plain[1] == plain[0] and [(a["score"], a["ops"]) for a in plain[0][0]] == [(w["score"], w["ops"]) for w in TW.oracle(pairs, SC, bounds)]
    with switched_context(PWA_RANGE_BYTES=budget) as c:
        assert everything(c) == plain


def test_workspace_is_a_ring_and_one_byte_per_planned_cell(ctx, pkg):
    pairs, bounds, want = TW.mixed()
    sizes = codes_sizes(pkg, pairs, SC, bounds)
    _, st_cod, st_off = both(ctx, pairs, SC, bounds, want)
    low = sum(ring + cells for ring, cells in sizes)
    high = sum(ring + cells + 16 for ring, cells in sizes if ring)
    print("codes workspace %d B in [%d, %d]; offsets workspace %d B" % (st_cod["workspace_bytes"], low, high, st_off["workspace_bytes"]))
    assert low <= st_cod["workspace_bytes"] <= high
    assert st_off["workspace_bytes"] == 12 * sum(cells for _, cells in sizes)
    assert st_cod["workspace_bytes"] < st_off["workspace_bytes"]


def raw_calls(pkg, ctx, name, seqs, pa, pb, sc):
    L = pkg.lib()
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa)
    a, b = (C.c_uint32 * max(n, 1))(*pa), (C.c_uint32 * max(n, 1))(*pb)
    score = (C.c_int32 * max(n, 1))()
    if name.endswith("_cigar"):
        cg, md, co, mo = C.create_string_buffer(4096), C.create_string_buffer(4096), (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))()
        return getattr(L, name)(ctx._h, *sc, blob, off, len(seqs), a, b, n, score, cg, 4096, co, md, 4096, mo, None, None)
    ops, ooff, nops = C.create_string_buffer(4096), (C.c_uint64 * max(n, 1))(), (C.c_uint64 * max(n, 1))()
    return getattr(L, name)(ctx._h, *sc, blob, off, len(seqs), a, b, n, score, ops, ooff, nops, None)


def test_validation_results_and_order_are_the_offsets_calls(ctx, pkg):
    seqs = [b"ACGT", b"ACGA", b"A" * 300]
    wide = (1, -(1 << 20), -6, -1)   # the range rule: (n + m + 2) 2^20 < 2^28 holds for the short pairs only
    cases = [(seqs, [0], [1], SC, 0), (seqs, [0], [1], (1, 1, -1, -1), INVALID), (seqs, [3], [1], (1, 1, -1, -1), INVALID), (seqs, [3], [1], SC, INVALID),
             (seqs, [0], [9], SC, INVALID), (seqs, [0], [1], wide, 0), (seqs, [0], [2], wide, CAPACITY), (seqs, [0, 0], [2, 7], wide, CAPACITY),
             (seqs, [0, 0], [7, 2], wide, INVALID), (seqs, [], [], SC, 0)]
    ctx.scores_wfa(seqs, [0], [1], *SC)
    for old in ("pwa_align_wfa_batch", "pwa_align_wfa_batch_cigar"):
        new = old.replace("wfa_", "wfa_codes_")
        for s, pa, pb, sc, rc in cases:
            if rc:
                before = ctx.align_wfa_stats()
            assert raw_calls(pkg, ctx, new, s, pa, pb, sc) == raw_calls(pkg, ctx, old, s, pa, pb, sc) == rc, (new, pa, pb, sc)
            if rc:
                assert ctx.align_wfa_stats() == before
    for call in (ctx.align_wfa_batch, ctx.align_wfa_batch_cigar):
        with pytest.raises(pkg.PwaError):
            call(seqs, [0], [1], 1, 1, -1, -1, form="codes")


def test_string_capacity_protocol(ctx, pkg):
    L = pkg.lib()
    rng = random.Random(25)
    pairs = [(p, mutate(rng, p, 0.1)) for p in (rand_seq(rng, 80) for _ in range(6))]
    seqs, pa, pb = flatten(pairs)
    full = ctx.align_wfa_batch_cigar(seqs, pa, pb, *SC, form="codes")
    assert full == ctx.align_wfa_batch_cigar(seqs, pa, pb, *SC)
    need_c, need_m = sum(len(r["cigar"]) for r in full), sum(len(r["mdz"]) for r in full)
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa)
    a, b = (C.c_uint32 * n)(*pa), (C.c_uint32 * n)(*pb)
    sc = (C.c_int32 * n)()
    co, mo, need = (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))(), (C.c_uint64 * 2)()
    for cap_c, cap_m, rc in [(need_c - 1, need_m, CAPACITY), (need_c, need_m - 1, CAPACITY), (0, 0, CAPACITY), (need_c, need_m, 0)]:
        cg, md = C.create_string_buffer(max(cap_c, 1)), C.create_string_buffer(max(cap_m, 1))
        need[0] = need[1] = 0
        got = L.pwa_align_wfa_codes_batch_cigar(ctx._h, *SC, blob, off, len(seqs), a, b, n, sc, cg, cap_c, co, md, cap_m, mo, need, None)
        assert got == rc and (need[0], need[1]) == (need_c, need_m)
    assert cg.raw[:need_c] == b"".join(r["cigar"] for r in full) and md.raw[:need_m] == b"".join(r["mdz"] for r in full)
    assert L.pwa_align_wfa_codes_batch_cigar(ctx._h, *SC, blob, off, len(seqs), a, b, n, sc, None, 8, co, md, need_m, mo, need, None) == INVALID


def test_eight_pairs_of_two_thousand_symbols(ctx):
    rng = random.Random(26)
    pairs = []
    for _ in range(8):
        p = rand_seq(rng, 2000)
        pairs.append((p, mutate(rng, p, 0.02)))
    seqs, pa, pb = flatten(pairs)
    scores = ctx.scores_wfa(seqs, pa, pb, *SC)
    bounds = [s - 100 for s in scores]
    al, st_cod, st_off = both(ctx, pairs, SC, bounds)
    assert [a["score"] for a in al] == scores
    for (p, t), a in zip(pairs, al):
        assert (a["ops"].count(b"M") + a["ops"].count(b"D"), a["ops"].count(b"M") + a["ops"].count(b"I")) == (len(p), len(t))
    assert 4 * st_cod["workspace_bytes"] < st_off["workspace_bytes"]
