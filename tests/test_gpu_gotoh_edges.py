"""Affine-gap (gotoh) batch alignments at the edges of the device code (gotoh_fill.hip.h, include/pwalign.h): every pattern class on
both sides of its row bounds, texts on both sides of the fill's chunk and lane ramp, the walk's LDS windows and op stores, tasks
whose four pairs end far apart or are padded with dummies, the edge scorings, the key-range limit, the three kinds of tie, and the
op-region / string-buffer forms of the C ABI.  Every device result is compared field for field with the numpy oracle
gotoh_oracle.py (itself tied to a scalar three-matrix DP by test_gotoh_oracle.py), not only re-scored."""
import ctypes as C
import random

import numpy as np
import pytest

import gotoh_oracle as GO
from conftest import switched_context
from test_gotoh_oracle import EDGE_SCORINGS
from test_gpu_cigar import fmt

pytestmark = pytest.mark.gpu

MODES = ["nw", "sw", "sg"]
PWA_E_CAPACITY = -5
# every gotoh class, pwalign.h: 16 lanes x RL rows for RL = 4, 6, 8, 10, 12, 16 (n <= 16 RL), then one pair per wave, 64 lanes x 8 | 16
PAT_LENS = [1, 15, 16, 17, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512,
            513, 767, 768, 769, 1023, 1024]
# both sides of the 16-step chunk, the 15- (16 lanes) and 63-step (64 lanes) lane ramps, the walk's LDS windows (32 steps for 16 lanes,
# 16 for 64) and its 64-op stores
TEXT_LENS = [0, 1, 2, 14, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 62, 63, 64, 65, 66, 79, 80, 81, 95, 96, 97, 127, 128, 129, 255, 256,
             257, 511, 512, 513, 1023, 1024, 1025]
LONG_TEXT = 10007
LONG_FOR = {1, 16, 17, 64, 96, 128, 160, 192, 256, 257, 512, 1024}   # the patterns that also get the long text
CLASS_REPS = [40, 80, 112, 150, 180, 230, 400, 900]                  # one pattern length per class
NORMAL = [(1, -4, -6, -1), (2, -3, -5, -2)]
POS_MISMATCH = (2, 1, -3, -1)   # rows past n (never-equal pad symbol) then grow past the real rows


def gotoh_class(n):
    """(lanes per pair, rows per lane) of the class a pattern of n symbols runs in (pwalign_align.hip: class_of for gotoh)"""
    if n <= 256:
        return 16, next(rl for rl in (4, 6, 8, 10, 12, 16) if n <= 16 * rl)
    return 64, 8 if n <= 512 else 16


ALL_CLASSES = {(16, rl) for rl in (4, 6, 8, 10, 12, 16)} | {(64, 8), (64, 16)}


def max_admitted(n, m):
    """pwalign.h: every result is exact while (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|) < 2^28"""
    return ((1 << 28) - 1) // (n + m + 2)


def _rand(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def _mutate(rng, s, alpha=b"ACGT", rate=0.08):
    out = bytearray()
    for x in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out += _rand(rng, rng.randint(1, 4), alpha)
        out.append(rng.choice(alpha) if rate / 3 * 2 <= r < rate else x)
    return bytes(out)


def _text_for(rng, p, length, alpha=b"ACGT"):
    """a random text holding a mutated copy of p near its start"""
    t = bytearray(_rand(rng, length, alpha))
    core = _mutate(rng, p, alpha)
    off = rng.randint(0, 40)
    t[off:off + len(core)] = core
    return bytes(t[:length])


def run_groups(c, mode, groups, sc, cigar=True, shuffle=None):
    """groups: [(p, t, ms)] -> the pairs (p, t[:m]) in one call (in a shuffled order when shuffle is a seed); each pattern's oracle
    results come from ONE fill of (p, t[:max(ms)]).  Compares score, end, start and ops (and the CIGAR / MD:Z call) with the oracle."""
    match, mismatch, go, ge = sc
    pairs, want = [], []
    for p, t, ms in groups:
        want += GO.prefixes(p, t[:max(ms)], ms, mode, (match, mismatch), go, ge)
        pairs += [(p, t[:m]) for m in ms]
    order = list(range(len(pairs)))
    if shuffle is not None:
        random.Random(shuffle).shuffle(order)
    seqs, pa, pb = [], [], []
    for k in order:
        seqs += list(pairs[k])
        pa.append(len(seqs) - 2)
        pb.append(len(seqs) - 1)
    got = c.align_gotoh_batch(mode, seqs, pa, pb, match, mismatch, go, ge)
    gc = c.align_gotoh_batch_cigar(mode, seqs, pa, pb, match, mismatch, go, ge) if cigar else None
    for x, k in enumerate(order):
        p, t = pairs[k]
        g, w = got[x], want[k]
        key = (mode, sc, len(p), len(t))
        assert (g["score"], g["end"], g["start"]) == (w["score"], w["end"], w["start"]), key
        assert g["ops"] == w["ops"], key
        if cigar:
            assert (gc[x]["score"], gc[x]["end"], gc[x]["start"]) == (w["score"], w["end"], w["start"]), key
            assert (gc[x]["cigar"], gc[x]["mdz"]) == fmt(p, t, w["ops"], w["start"]), key
    return got


def test_the_grids_reach_every_class_and_boundary():
    assert {gotoh_class(n) for n in PAT_LENS} == ALL_CLASSES
    assert {gotoh_class(n) for n in CLASS_REPS} == ALL_CLASSES
    for lo, hi in [(0, 64), (64, 96), (96, 128), (128, 160), (160, 192), (192, 256), (256, 512), (512, 768), (768, 1024)]:
        assert hi in PAT_LENS and (hi + 1 in PAT_LENS or hi == 1024) and hi - 1 in PAT_LENS, hi   # both sides of every class edge
    for b in (16, 32, 48, 64, 80, 96, 128, 256, 512, 1024):   # chunks, ramps (15, 63), windows (32, 16 steps), 64-op stores
        assert {b - 1, b, b + 1} <= set(TEXT_LENS), b
    assert {14, 15, 16, 62, 63, 64} <= set(TEXT_LENS)


def _grid(seed, alpha=b"ACGT"):
    rng = random.Random(seed)
    groups = []
    for n in PAT_LENS:
        p = _rand(rng, n, alpha)
        ms = TEXT_LENS + ([LONG_TEXT] if n in LONG_FOR else [])
        groups.append((p, _text_for(rng, p, max(ms), alpha), ms))
    return groups


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sc", NORMAL + [POS_MISMATCH, (1, -4, -6, 0)])
def test_class_and_text_boundaries(ctx, mode, sc):
    """B: every pattern length of PAT_LENS against every text length of TEXT_LENS (and a ~10 000-symbol text for a pattern of each
    class): op lists, cells, scores, CIGAR and MD:Z against the oracle"""
    run_groups(ctx, mode, _grid(101), sc)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sc", [NORMAL[1], POS_MISMATCH])
def test_tasks_whose_pairs_end_far_apart(ctx, mode, sc):
    """C: exactly four pairs of each class, texts of 0, 17, 1000 and ~10 000 symbols: one 16-lane task whose lanes freeze one after
    another (GUARD chunks long past the shortest text), in a shuffled caller order"""
    rng = random.Random(202)
    groups = []
    for n in CLASS_REPS:
        p = _rand(rng, n)
        groups.append((p, _text_for(rng, p, LONG_TEXT), [0, 17, 1000, LONG_TEXT]))
    run_groups(ctx, mode, groups, sc, shuffle=len(mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", [1, 2, 3])
def test_tasks_padded_with_dummies(ctx, mode, count):
    """C: 1, 2 or 3 pairs of each class: the last 16-lane task of every class is padded with empty dummy patterns"""
    rng = random.Random(303 + count)
    groups = []
    for n in CLASS_REPS:
        p = _rand(rng, n)
        groups.append((p, _text_for(rng, p, LONG_TEXT), [LONG_TEXT, 17, 1000][:count]))
    for sc in (NORMAL[0], POS_MISMATCH):
        run_groups(ctx, mode, groups, sc, shuffle=count)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sc", EDGE_SCORINGS + [POS_MISMATCH, (0, 0, -2, -1), (3, 3, -4, -1)])
def test_edge_scorings_at_every_class(ctx, mode, sc):
    """D: gap_extend = 0, a gap open too dear to pay off, match <= mismatch, negative match, positive mismatch, match = 0 with gaps,
    match = mismatch: one pattern per class against a few texts on a three-letter alphabet (more ties)"""
    rng = random.Random(404)
    groups = []
    for n in CLASS_REPS:
        p = _rand(rng, n, b"ACG")
        groups.append((p, _text_for(rng, p, 1100, b"ACG"), [0, 1, 17, 63, 64, 65, 300, 1100]))
    run_groups(ctx, mode, groups, sc)


# ------------------------------------------------------------------ E. the key-range limit
def _raw_gotoh(pkg, c, mode, sc, seqs, pa, pb, ops_off=None):
    """pwa_align_gotoh_batch through ctypes -> (rc, scores, ops buffer, ops_off, n_ops, end cells, start cells)"""
    L = pkg.lib()
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa)
    if ops_off is None:
        ops_off, tot = [], 0
        for k in range(n):
            ops_off.append(tot)
            tot += len(seqs[pa[k]]) + len(seqs[pb[k]])
    tot = max([ops_off[k] + len(seqs[pa[k]]) + len(seqs[pb[k]]) for k in range(n)] + [1])
    ooff = (C.c_uint64 * max(n, 1))(*ops_off)
    ops = C.create_string_buffer(tot)
    sc_out = (C.c_int32 * max(n, 1))()
    nops = (C.c_uint64 * max(n, 1))()
    endc, startc = (C.c_uint64 * (2 * max(n, 1)))(), (C.c_uint64 * (2 * max(n, 1)))()
    rc = L.pwa_align_gotoh_batch(c._h, pkg.MODE[mode], *sc, blob, off, len(seqs), (C.c_uint32 * max(n, 1))(*pa),
                                 (C.c_uint32 * max(n, 1))(*pb), n, sc_out, ops, ooff, nops, endc, startc)
    return rc, list(sc_out)[:n], ops.raw, list(ops_off), list(nops)[:n], list(endc)[:2 * n], list(startc)[:2 * n]


def _batch(pairs):
    """[(p, t)] -> seqs, pair_a, pair_b"""
    seqs = [x for pr in pairs for x in pr]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1024, 256, 1])
def test_largest_admitted_scores_are_exact(ctx, mode, n):
    """E: identical n x n pairs at the largest admitted match (1024: 64 lanes, SW's first-maximum key H * 16 only 2^21 below 2^31;
    256: 16 lanes; 1 x 1), with mismatch and gap_open + gap_extend at the bound as well, and a mutated pair at the same scoring"""
    mx = max_admitted(n, n)
    assert (n + n + 2) * mx < 1 << 28 <= (n + n + 2) * (mx + 1)
    sc = (mx, -mx, -(mx // 3), -(mx - mx // 3))
    rng = random.Random(n)
    p = _rand(rng, n)
    q = _mutate(rng, p, rate=0.1)[:n]
    q += _rand(rng, n - len(q))
    pairs = [(p, p), (q, p), (p, q)] if n > 1 else [(b"A", b"A"), (b"A", b"C"), (b"\x00", b"\x00")]
    got = ctx.align_gotoh_batch(mode, *_batch(pairs), *sc)
    assert got[0]["score"] == n * mx and got[0]["ops"] == b"M" * n, mode
    for (a, b), g in zip(pairs, got):
        w = GO.align(a, b, mode, sc[:2], *sc[2:])
        assert (g["score"], g["end"], g["start"], g["ops"]) == (w["score"], w["end"], w["start"], w["ops"]), (mode, len(a), len(b))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [256, 1024])
def test_most_negative_keys_are_exact(ctx, mode, n):
    """E: pattern and text without a common symbol, a ~10 000-symbol text, mismatch and |gap_open| + |gap_extend| at the bound: NW's
    score comes within a few percent of -2^28 (keys V * 8 near -2^31)"""
    m = LONG_TEXT
    mx = max_admitted(n, m)
    sc = (1, -mx, -1, -(mx - 1))
    rng = random.Random(n + 1)
    pairs = [(b"A" * n, b"C" * m), (_rand(rng, n, b"AC"), _rand(rng, m, b"GT"))]
    got = ctx.align_gotoh_batch(mode, *_batch(pairs), *sc)
    if mode == "nw":
        assert got[0]["score"] < -(1 << 28) * 0.85
    for (a, b), g in zip(pairs, got):
        w = GO.align(a, b, mode, sc[:2], *sc[2:])
        assert (g["score"], g["end"], g["start"], g["ops"]) == (w["score"], w["end"], w["start"], w["ops"]), (mode, n)


@pytest.mark.parametrize("mode", MODES)
def test_one_step_over_the_bound_is_refused(pkg, ctx, mode):
    """E: one step over the bound, through each of its three terms, is PWA_E_CAPACITY -- alone and inside a batch of smaller pairs
    -- and the context stays usable; at the bound the call succeeds"""
    rng = random.Random(7)
    for n, m in [(1024, 1024), (256, 256), (1, 1), (100, 5000)]:
        mx = max_admitted(n, m)
        p, t = _rand(rng, n), _rand(rng, m)
        pairs = [(p, t), (p[:n // 2], t[:m // 2]), (b"", t[:1])]
        seqs, pa, pb = _batch(pairs)
        half = mx // 2
        for at, over in [((mx, -1, -1, -1), (mx + 1, -1, -1, -1)), ((-mx, -1, -1, -1), (-mx - 1, -1, -1, -1)),
                         ((1, -mx, -1, -1), (1, -mx - 1, -1, -1)), ((1, -1, -half, half - mx), (1, -1, -half, half - mx - 1)),
                         ((1, -1, 0, -mx), (1, -1, 0, -mx - 1)), ((1, -1, -mx, 0), (1, -1, -mx - 1, 0))]:
            assert max(abs(at[0]), abs(at[1]), -at[2] - at[3]) == mx
            assert _raw_gotoh(pkg, ctx, mode, at, seqs, pa, pb)[0] == 0, (n, m, at)
            assert _raw_gotoh(pkg, ctx, mode, over, seqs, pa, pb)[0] == PWA_E_CAPACITY, (n, m, over)
            assert _raw_gotoh(pkg, ctx, mode, over, seqs, [0], [1])[0] == PWA_E_CAPACITY, (n, m, over)
    with pytest.raises(pkg.PwaError, match="range"):
        ctx.align_gotoh_batch(mode, [b"A" * 1024, b"A" * 1024], [0], [1], max_admitted(1024, 1024) + 1, -1, -1, -1)
    run_groups(ctx, mode, [(b"ACGTACGTTTGA" * 9, b"ACGTACTTGA" * 30, [0, 5, 100, 300])], NORMAL[0])


# ------------------------------------------------------------------ F. ties
def _homopolymer_reads(rng, n, count):
    """reads of about n symbols made of homopolymer runs; each read has one to three bases planted in or cut out of a run"""
    out = []
    for k in range(count):
        runs = []
        while sum(len(r) for r in runs) < n + 20:
            runs.append(bytes([rng.choice(b"ACGT")]) * rng.randint(1, 9))
        ref = b"".join(runs)
        read = bytearray(ref[:n + 20])
        r = rng.randrange(len(runs) - 2)
        at = sum(len(x) for x in runs[:r]) + rng.randint(0, len(runs[r]))
        L = rng.randint(1, 3)
        if k % 2:
            read[at:at] = runs[r][:1] * L   # the run grows
        else:
            del read[at:at + min(L, len(runs[r]) - 1)]   # the run shrinks, but stays
        out.append((bytes(read[:n]), ref))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [100, 600])
def test_homopolymer_indels_land_where_the_oracle_puts_them(ctx, mode, n):
    """F: a planted indel inside a homopolymer run can sit anywhere in the run; the gap placement equals the oracle's (both lane
    widths), with gap_extend < 0 and = 0"""
    rng = random.Random(n)
    pairs = _homopolymer_reads(rng, n, 48 if n <= 256 else 16)
    for sc in [(1, -4, -6, -1), (2, -3, -5, 0)]:
        seqs, pa, pb = _batch(pairs)
        got = ctx.align_gotoh_batch(mode, seqs, pa, pb, *sc)
        for (p, t), g in zip(pairs, got):
            w = GO.align(p, t, mode, sc[:2], *sc[2:])
            assert (g["score"], g["end"], g["start"], g["ops"]) == (w["score"], w["end"], w["start"], w["ops"]), (mode, sc, p, t)


@pytest.mark.parametrize("mode", MODES)
def test_gap_extend_zero_open_and_extend_tie(ctx, mode):
    """F: gap_extend = 0: every choice between opening and extending a gap ties (a tie opens); reads with long indels of every class"""
    rng = random.Random(55)
    groups = []
    for n in CLASS_REPS:
        p = _rand(rng, n)
        t = bytearray(_mutate(rng, p, rate=0.15))
        a = rng.randrange(len(t))
        t[a:a] = _rand(rng, rng.randint(5, 40))
        del t[len(t) // 2:len(t) // 2 + rng.randint(3, 20)]
        groups.append((p, bytes(t) + _rand(rng, 200), [len(t) // 2, len(t), len(t) + 200]))
    for sc in [(1, -4, -6, 0), (2, -3, -3, 0), (1, -1, -2, 0)]:
        run_groups(ctx, mode, groups, sc)


def _copies(rng, p, k, junk=(3, 30), alpha=b"ACGT"):
    t = bytearray(_rand(rng, rng.randint(*junk), alpha))
    for _ in range(k):
        t += p + _rand(rng, rng.randint(*junk), alpha)
    return bytes(t)


@pytest.mark.parametrize("n", [16, 40, 100, 200, 256, 600, 1024])
def test_sw_keeps_the_first_row_major_maximum(ctx, n):
    """F: equal maxima in several columns (texts of repeated copies of the pattern) and in several rows (a pattern X + X against a
    text with separate copies of X): the end cell is the first row-major maximum, as the oracle's"""
    rng = random.Random(n + 9)
    x = _rand(rng, n // 2)
    p = _rand(rng, n)
    pairs = [(p, _copies(rng, p, 4)), (p, p * 3), (x + x, _copies(rng, x, 3)), (x + _rand(rng, n - 2 * len(x)) + x, _copies(rng, x, 2)),
             (p, _copies(rng, p[: n // 2], 2) + _copies(rng, p[n // 2:], 2))]
    for sc in [(1, -4, -6, -1), (2, -3, -5, 0), POS_MISMATCH]:
        seqs, pa, pb = _batch(pairs)
        got = ctx.align_gotoh_batch("sw", seqs, pa, pb, *sc)
        for (a, b), g in zip(pairs, got):
            w = GO.align(a, b, "sw", sc[:2], *sc[2:])
            assert (g["score"], g["end"], g["start"], g["ops"]) == (w["score"], w["end"], w["start"], w["ops"]), (n, sc, len(a), len(b))


@pytest.mark.parametrize("n", [16, 40, 100, 200, 256, 600, 1024])
def test_sg_keeps_the_smallest_end_column(ctx, n):
    """F: the pattern at several offsets of the text (exact copies, and copies with one substitution each at the same score): the
    end column is the smallest j with maximal H[n][j], as the oracle's"""
    rng = random.Random(n + 19)
    p = _rand(rng, n)

    def sub(s, i):
        return s[:i] + bytes([b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]]) + s[i + 1:]
    pairs = [(p, _copies(rng, p, 4)), (p, p * 3), (p, _copies(rng, sub(p, 0), 1) + _copies(rng, sub(p, n - 1), 2)),
             (p, _rand(rng, 50) + p + p[: n // 2] + p)]
    for sc in [(1, -4, -6, -1), (2, -3, -5, 0), POS_MISMATCH]:
        seqs, pa, pb = _batch(pairs)
        got = ctx.align_gotoh_batch("sg", seqs, pa, pb, *sc)
        for (a, b), g in zip(pairs, got):
            w = GO.align(a, b, "sg", sc[:2], *sc[2:])
            assert (g["score"], g["end"], g["start"], g["ops"]) == (w["score"], w["end"], w["start"], w["ops"]), (n, sc, len(a), len(b))


# ------------------------------------------------------------------ G. op-region layout and string buffers
def _mixed(seed, count):
    rng = random.Random(seed)
    pairs = []
    for k in range(count):
        n = rng.choice(CLASS_REPS + [0, 1, 17, 256, 257, 1024])
        p = _rand(rng, n)
        m = rng.choice([0, 1, 16, 63, 200, 1030])
        pairs.append((p, _text_for(rng, p, m) if m else b""))
    return pairs


@pytest.mark.parametrize("mode", MODES)
def test_op_region_layouts_are_byte_identical(pkg, ctx, mode):
    """G: gapped ops_off (the staging copy) and PWA_NO_TILED_OPS give the tiled call's scores, cells and op bytes; the tiled call
    itself against the oracle on a sample"""
    sc = NORMAL[1]
    pairs = _mixed(66, 160)
    seqs, pa, pb = _batch(pairs)
    rc, s0, raw0, off0, nops0, e0, st0 = _raw_gotoh(pkg, ctx, mode, sc, seqs, pa, pb)
    assert rc == 0
    ops0 = [raw0[off0[k]:off0[k] + nops0[k]] for k in range(len(pairs))]
    gapped, tot = [], 0
    for k, (p, t) in enumerate(pairs):
        tot += 7 + 64 * (k % 3)
        gapped.append(tot)
        tot += len(p) + len(t)
    rc, s1, raw1, off1, nops1, e1, st1 = _raw_gotoh(pkg, ctx, mode, sc, seqs, pa, pb, gapped)
    assert rc == 0
    assert (s1, nops1, e1, st1) == (s0, nops0, e0, st0)
    assert [raw1[off1[k]:off1[k] + nops1[k]] for k in range(len(pairs))] == ops0
    with switched_context(PWA_NO_TILED_OPS="1") as c:
        rc, s2, raw2, off2, nops2, e2, st2 = _raw_gotoh(pkg, c, mode, sc, seqs, pa, pb)
        assert rc == 0
        assert (s2, nops2, e2, st2) == (s0, nops0, e0, st0)
        assert [raw2[off2[k]:off2[k] + nops2[k]] for k in range(len(pairs))] == ops0
    for k in range(0, len(pairs), 11):
        w = GO.align(*pairs[k], mode, sc[:2], *sc[2:])
        assert (s0[k], ops0[k], tuple(e0[2 * k:2 * k + 2]), tuple(st0[2 * k:2 * k + 2])) == (w["score"], w["ops"], w["end"], w["start"]), k


@pytest.mark.parametrize("mode", MODES)
def test_cigar_capacity(pkg, ctx, mode):
    """G: too small a cigar_cap or mdz_cap is PWA_E_CAPACITY with the exact totals in needed[]; a retry at exactly needed gives the
    strings of the roomy call"""
    L = pkg.lib()
    sc = NORMAL[0]
    pairs = _mixed(77, 60)
    seqs, pa_l, pb_l = _batch(pairs)
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa_l)
    pa, pb = (C.c_uint32 * n)(*pa_l), (C.c_uint32 * n)(*pb_l)
    u64p = C.POINTER(C.c_uint64)

    def call(cap_c, cap_m):
        cg, md = np.zeros(max(cap_c, 1), np.uint8), np.zeros(max(cap_m, 1), np.uint8)
        co, mo = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        need = (C.c_uint64 * 2)()
        rc = L.pwa_align_gotoh_batch_cigar(ctx._h, pkg.MODE[mode], *sc, blob, off, len(seqs), pa, pb, n, (C.c_int32 * n)(),
                                           cg.ctypes.data_as(C.c_void_p), cap_c, co.ctypes.data_as(u64p), md.ctypes.data_as(C.c_void_p),
                                           cap_m, mo.ctypes.data_as(u64p), None, None, need)
        strs = [(cg[int(co[k]):int(co[k + 1])].tobytes(), md[int(mo[k]):int(mo[k + 1])].tobytes()) for k in range(n)] if rc == 0 else None
        return rc, (need[0], need[1]), strs

    want = [(g["cigar"], g["mdz"]) for g in ctx.align_gotoh_batch_cigar(mode, seqs, pa_l, pb_l, *sc)]
    rc, need, strs = call(1 << 20, 1 << 20)
    assert rc == 0 and strs == want
    assert need == (sum(len(c) for c, _ in want), sum(len(m) for _, m in want))
    assert call(need[0] - 1, need[1])[:2] == (PWA_E_CAPACITY, need)
    assert call(need[0], need[1] - 1)[:2] == (PWA_E_CAPACITY, need)
    assert call(0, 0)[:2] == (PWA_E_CAPACITY, need)
    assert call(need[0], need[1]) == (0, need, want)
