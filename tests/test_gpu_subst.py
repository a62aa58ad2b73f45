"""Substitution-matrix scoring of the affine-gap batch calls on the device (subst_fill.hip.h, include/pwalign.h): every pattern class on
both sides of its row bounds, equivalence with the byte-compare gotoh calls under a match / mismatch matrix, the orientation of the
table, the code map, ties, the scores entry points, several ranges, and the errors.  Every device result is compared field for field
with the numpy oracle gotoh_oracle.py under the table (tied to a scalar three-matrix DP and to its byte compare by test_subst_oracle.py): score, end and
start cell, the op list byte for byte, CIGAR / MD:Z against pwa_format_alignment of those ops, and the ops re-scored under the matrix."""
import ctypes as C
import random

import numpy as np
import pytest

import gotoh_oracle as GO
from conftest import load_pkg, switched_context
from gotoh_oracle import random_table
from test_gpu_cigar import fmt

pytestmark = pytest.mark.gpu

MODES = ["nw", "sw", "sg"]
PWA_E_INVALID, PWA_E_CAPACITY = -1, -5
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
PAT_LENS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 150, 255, 256, 257, 511, 512, 513, 1023, 1024]
TEXT_LENS = [0, 1, 16, 17, 150, 257]


def _rand(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def _mutate(rng, s, alpha, rate=0.1):
    out = bytearray()
    for x in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out += _rand(rng, rng.randint(1, 3), alpha)
        out.append(rng.choice(alpha) if 2 * rate / 3 <= r < rate else x)
    return bytes(out)


def _batch(pairs):
    seqs, pa, pb = [], [], []
    for p, t in pairs:
        seqs += [p, t]
        pa.append(len(seqs) - 2)
        pb.append(len(seqs) - 1)
    return seqs, pa, pb


def strings(pkg, p, t, ops, start, end):
    """CIGAR and MD:Z of an op list: pwa_format_alignment (C strings: a sequence with a NUL byte takes the Python restatement)"""
    if 0 in p or 0 in t:
        return fmt(p, t, ops, start)
    f = pkg.format_alignment(p, t, ops, end)
    return f["cigar"], f["mdz"]


def check(c, mode, pairs, want, table, go, ge, cigar=True):
    """one align_subst_batch (+ _cigar) call over `pairs` against the oracle's results `want`"""
    pkg = load_pkg()
    seqs, pa, pb = _batch(pairs)
    got = c.align_subst_batch(mode, seqs, pa, pb, table, go, ge)
    gc = c.align_subst_batch_cigar(mode, seqs, pa, pb, table, go, ge) if cigar else None
    for k, ((p, t), g, w) in enumerate(zip(pairs, got, want)):
        key = (mode, go, ge, len(p), len(t), k)
        assert (g["score"], g["end"], g["start"]) == (w["score"], w["end"], w["start"]), key
        assert g["ops"] == w["ops"], key
        assert GO.op_score(p, t, g["ops"], g["start"], table, go, ge) == g["score"], key
        if cigar:
            assert (gc[k]["score"], gc[k]["end"], gc[k]["start"]) == (w["score"], w["end"], w["start"]), key
            assert (gc[k]["cigar"], gc[k]["mdz"]) == strings(pkg, p, t, g["ops"], g["start"], g["end"]), key
    return got


# ------------------------------------------------------------------ 1. class edges
@pytest.fixture(scope="module")
def edge_groups():
    rng = random.Random(31)
    groups = []
    for n in PAT_LENS:
        p = _rand(rng, n, PROTEIN)
        t = bytearray(_rand(rng, max(TEXT_LENS), PROTEIN))
        core = _mutate(rng, p, PROTEIN)
        t[5:5 + len(core)] = core
        groups.append((p, bytes(t[:max(TEXT_LENS)])))
    return groups


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gaps", [(-11, -1), (0, -3)])
def test_class_edges(ctx, edge_groups, mode, gaps):
    """every pattern length on both sides of each class bound against texts on both sides of the 16-step chunk: a random asymmetric
    20-symbol matrix with entries in -9..11, a positive diagonal and positive off-diagonal entries"""
    table = random_table(41, PROTEIN)
    submat = np.asarray(table[2]).reshape(20, 20)
    assert (submat.diagonal() > 0).all() and (submat - np.diag(submat.diagonal()) > 0).any() and not (submat == submat.T).all()
    pairs, want = [], []
    for p, t in edge_groups:
        want += GO.prefixes(p, t, TEXT_LENS, mode, table, *gaps)
        pairs += [(p, t[:m]) for m in TEXT_LENS]
    check(ctx, mode, pairs, want, table, *gaps)


# ------------------------------------------------------------------ 2. equivalence with the byte-compare calls
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sc", [(1, -4, -6, -1), (5, -4, -16, -4)])
def test_match_mismatch_matrix_equals_the_gotoh_calls(pkg, ctx, mode, sc):
    match, mismatch, go, ge = sc
    table = pkg.subst_table(b"ACGT", np.where(np.eye(4, dtype=bool), match, mismatch))
    rng = random.Random(52)
    pairs = []
    for n in (0, 1, 30, 64, 150, 200, 256, 300, 700, 1024):
        p = _rand(rng, n)
        pairs += [(p, _mutate(rng, p, b"ACGT") + _rand(rng, 20)), (p, _rand(rng, rng.choice([0, 40, 300])))]
    seqs, pa, pb = _batch(pairs)
    assert ctx.align_subst_batch(mode, seqs, pa, pb, table, go, ge) == ctx.align_gotoh_batch(mode, seqs, pa, pb, match, mismatch, go, ge)
    assert ctx.align_subst_batch_cigar(mode, seqs, pa, pb, table, go, ge) == ctx.align_gotoh_batch_cigar(mode, seqs, pa, pb, match, mismatch, go, ge)
    for want_end in (False, True):
        assert ctx.scores_subst(mode, seqs, pa, pb, table, go, ge, want_end) == ctx.scores_gotoh(mode, seqs, pa, pb, match, mismatch, go, ge, want_end)
        assert ctx.scores_subst_oneshot(mode, seqs, pa, pb, table, go, ge, want_end) == \
            ctx.scores_gotoh_oneshot(mode, seqs, pa, pb, match, mismatch, go, ge, want_end)


# ------------------------------------------------------------------ 3. indexing
def _skew_table(pkg, n_sym):
    """s(a, b) != s(b, a) for every pair a != b: above the diagonal +3 + (a + b) % 3, below it -4 - (a + b) % 2; diagonal 2"""
    a, b = np.indices((n_sym, n_sym))
    m = np.where(a < b, 3 + (a + b) % 3, -4 - (a + b) % 2)
    m[a == b] = 2
    alpha = bytes(range(65, 65 + n_sym))
    assert all(m[x, y] != m[y, x] for x in range(n_sym) for y in range(x))
    return alpha, pkg.subst_table(alpha, m), pkg.subst_table(alpha, m.T)


@pytest.mark.parametrize("n_sym", [1, 2, 5, 31, 32])
@pytest.mark.parametrize("mode", MODES)
def test_table_orientation_and_alphabet_sizes(pkg, ctx, mode, n_sym):
    """row = pattern code, column = text code: on these inputs the oracle's results under the transposed matrix differ, so a
    transposed lookup on the device cannot pass"""
    alpha, table, transposed = _skew_table(pkg, n_sym)
    rng = random.Random(60 + n_sym)
    pairs = [(_rand(rng, n, alpha), _rand(rng, m, alpha)) for n, m in [(7, 9), (40, 33), (150, 170), (257, 120), (600, 40)]]
    go, ge = -5, -1
    want = GO.align_many(pairs, mode, table, go, ge)
    if n_sym > 1:
        other = GO.align_many(pairs, mode, transposed, go, ge)
        assert sum((w["score"], w["ops"]) != (o["score"], o["ops"]) for w, o in zip(want, other)) >= 4   # (of the five pairs)
    check(ctx, mode, pairs, want, table, go, ge)


# ------------------------------------------------------------------ 4. the code map
@pytest.mark.parametrize("mode", MODES)
def test_code_map_folds_case_and_wildcards(pkg, ctx, mode):
    """lower case folded to upper; unknown bytes, NUL and '-' on a wildcard code that scores 0; MD:Z reports byte identity"""
    m = np.full((5, 5), -4)
    m[np.arange(4), np.arange(4)] = 5
    m[4, :] = m[:, 4] = 0
    table = pkg.subst_table(b"ACGTN", m, unknown=4, fold_case=True)
    rng = random.Random(70)
    soup = b"ACGTacgtN-\x00xZ"
    pairs = [(b"ACGTACGT", b"acgtacgt"), (b"AC-GT\x00AC", b"ACNGTxAC"), (b"acgtnACGT", b"ACGTNacgt")]
    pairs += [(_rand(rng, n, soup), _rand(rng, m_, soup)) for n, m_ in [(33, 50), (150, 140), (300, 280)]]
    want = GO.align_many(pairs, mode, table, -6, -1)
    got = check(ctx, mode, pairs, want, table, -6, -1)
    assert got[0]["score"] == 40 and got[0]["ops"] == b"M" * 8   # eight positively scored columns ...
    gc = ctx.align_subst_batch_cigar(mode, *_batch(pairs[:1]), table, -6, -1)[0]
    assert gc["cigar"] == b"8M" and gc["mdz"] == fmt(*pairs[0], b"M" * 8, (0, 0))[1] != b"8"   # ... that MD:Z lists as mismatches


def test_bytes_outside_the_alphabet_raise_without_unknown(pkg, ctx):
    table = pkg.subst_table(b"ACGT", np.eye(4, dtype=int))
    seqs, pa, pb = _batch([(b"ACGT", b"ACNT")])
    for call in (ctx.align_subst_batch, ctx.align_subst_batch_cigar, ctx.scores_subst, ctx.scores_subst_oneshot, ctx.batch_subst):
        with pytest.raises(pkg.PwaError):
            call("nw", seqs, pa, pb, table, -2, -1)
    assert ctx.scores_subst("nw", [b"ACGT", b"ACGT"], [0], [1], table, -2, -1) == [4]


# ------------------------------------------------------------------ 5. ties
@pytest.mark.parametrize("mode", MODES)
def test_ties(pkg, ctx, mode):
    """all-equal symbols with s = -gap_extend and gap_open = 0: diag / E / F tie all over the matrix, and open ties extend; s = 0
    with zero gaps: everything ties; gap_extend = 0: every open / extend choice ties"""
    rng = random.Random(80)
    shapes = [(5, 9), (17, 16), (64, 70), (150, 90), (257, 40), (520, 30)]
    for s, go, ge in [(3, 0, -3), (0, 0, 0), (2, -2, 0), (1, 0, -1)]:
        one = pkg.subst_table(b"A", [[s]], unknown=0)
        pairs = [(b"A" * n, b"A" * m) for n, m in shapes]
        check(ctx, mode, pairs, GO.align_many(pairs, mode, one, go, ge), one, go, ge, cigar=False)
        two = pkg.subst_table(b"AB", [[s, -s], [s, s]])
        pairs = [(_rand(rng, n, b"AB"), _rand(rng, m, b"AB")) for n, m in shapes]
        check(ctx, mode, pairs, GO.align_many(pairs, mode, two, go, ge), two, go, ge, cigar=False)


# ------------------------------------------------------------------ 6. scores
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("want_end", [False, True])
def test_scores_equal_the_alignment_call(ctx, mode, want_end):
    import torch
    table = random_table(43, PROTEIN)
    rng = random.Random(90)
    pairs = []
    for n in (0, 1, 16, 64, 65, 150, 256, 257, 512, 513, 1024):
        p = _rand(rng, n, PROTEIN)
        pairs += [(p, _mutate(rng, p, PROTEIN) + _rand(rng, 30, PROTEIN)), (p, _rand(rng, rng.choice([0, 17, 200]), PROTEIN))]
    seqs, pa, pb = _batch(pairs)
    go, ge = -11, -1
    al = ctx.align_subst_batch(mode, seqs, pa, pb, table, go, ge)
    scores = [a["score"] for a in al]
    if want_end:
        want = (scores, [a["end"][0] for a in al], [a["end"][1] for a in al])
    else:
        want = scores
    assert ctx.scores_subst(mode, seqs, pa, pb, table, go, ge, want_end) == want
    assert ctx.scores_subst_oneshot(mode, seqs, pa, pb, table, go, ge, want_end) == want
    b = ctx.batch_subst(mode, seqs, pa, pb, table, go, ge, want_end)
    assert b.cell_bits() == 0 and b.profile_form() == 0 and "subst_scores_kernel" in b.info()["kernel"]
    b.run()
    assert b.fetch() == want
    d = torch.full((len(pa),), -77, dtype=torch.int32, device="cuda")
    b.set_d_scores(d.data_ptr())
    b.run()
    torch.cuda.synchronize()
    assert b.fetch() == want
    assert d.cpu().tolist() == scores
    assert b.last_ms() >= 0 and len(b.run_times()) == 2
    b.close()
    assert ctx.align_subst_stats()["fill_ms"] > 0


def test_empty_lists(ctx):
    table = random_table(43, PROTEIN)
    assert ctx.align_subst_batch("nw", [], [], [], table, -2, -1) == []
    assert ctx.align_subst_batch_cigar("sw", [], [], [], table, -2, -1) == []
    assert ctx.scores_subst("sg", [], [], [], table, -2, -1) == []
    assert ctx.scores_subst_oneshot("nw", [], [], [], table, -2, -1, True) == ([], [], [])


# ------------------------------------------------------------------ 7. several ranges
@pytest.mark.parametrize("mode", MODES)
def test_several_ranges(ctx, mode):
    table = random_table(44, PROTEIN)
    rng = random.Random(100)
    pairs = []
    for k in range(48):
        p = _rand(rng, rng.choice([0, 20, 150, 256, 300, 1000]), PROTEIN)
        pairs.append((p, _mutate(rng, p, PROTEIN) + _rand(rng, rng.choice([0, 100, 700]), PROTEIN)))
    seqs, pa, pb = _batch(pairs)
    one = ctx.align_subst_batch(mode, seqs, pa, pb, table, -11, -1)
    one_c = ctx.align_subst_batch_cigar(mode, seqs, pa, pb, table, -11, -1)
    with switched_context(PWA_RANGE_BYTES="1048576") as c:
        assert c.align_subst_batch(mode, seqs, pa, pb, table, -11, -1) == one
        assert c.align_subst_batch_cigar(mode, seqs, pa, pb, table, -11, -1) == one_c
    for k in range(0, len(pairs), 7):
        w = GO.align(*pairs[k], mode, table, -11, -1)
        assert (one[k]["score"], one[k]["ops"], one[k]["end"], one[k]["start"]) == (w["score"], w["ops"], w["end"], w["start"]), k


# ------------------------------------------------------------------ 8. errors
def _raw(pkg, c, mode, code, n_sym, submat, go, ge, pairs, cigar_cap=None):
    """the C calls themselves -> (rc of pwa_align_subst_batch, rc of _cigar, needed, rc of pwa_subst_batch_create, rc of pwa_scores_subst)"""
    L = pkg.lib()
    seqs, pa_l, pb_l = _batch(pairs)
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = len(pa_l)
    pa, pb = (C.c_uint32 * max(n, 1))(*pa_l), (C.c_uint32 * max(n, 1))(*pb_l)
    code_a = None if code is None else (C.c_uint8 * 256)(*code)
    sub_a = None if submat is None else (C.c_int32 * len(submat))(*submat)
    head = (c._h, pkg.MODE[mode], code_a, n_sym, sub_a, go, ge, blob, off, len(seqs), pa, pb, n)
    tot = sum(len(p) + len(t) for p, t in pairs)
    ooff = (C.c_uint64 * max(n, 1))()
    at = 0
    for k, (p, t) in enumerate(pairs):
        ooff[k] = at
        at += len(p) + len(t)
    sc = (C.c_int32 * max(n, 1))()
    rc_ops = L.pwa_align_subst_batch(*head, sc, C.create_string_buffer(tot + 1), ooff, (C.c_uint64 * max(n, 1))(), None, None)
    cap = 3 * tot + 24 * n + 24 if cigar_cap is None else cigar_cap
    need = (C.c_uint64 * 2)()
    rc_str = L.pwa_align_subst_batch_cigar(*head, sc, C.create_string_buffer(cap + 1), cap, (C.c_uint64 * (n + 1))(),
                                           C.create_string_buffer(3 * tot + 24 * n + 25), 3 * tot + 24 * n + 24, (C.c_uint64 * (n + 1))(), None, None, need)
    h = C.c_void_p()
    rc_b = L.pwa_subst_batch_create(*head, 1, C.byref(h))
    if h.value:
        L.pwa_batch_destroy(h)
    rc_s = L.pwa_scores_subst(*head, sc, None, None)
    return rc_ops, rc_str, (need[0], need[1]), rc_b, rc_s


def _rcs(r):
    return (r[0], r[1], r[3], r[4])


def test_invalid_arguments(pkg, ctx):
    pairs = [(b"ACGT", b"ACGTT")]
    code = [0, 1] * 128
    ok = _raw(pkg, ctx, "nw", code, 2, [1, -1, -1, 1], -2, -1, pairs)
    assert _rcs(ok) == (0, 0, 0, 0)
    for n_sym in (0, 33, -1):
        assert _rcs(_raw(pkg, ctx, "nw", [0] * 256, n_sym, [0] * 33 * 33, -2, -1, pairs)) == (PWA_E_INVALID,) * 4
    for at in (0, 65, 255):   # a code >= n_sym anywhere in the map, whether or not the byte occurs
        bad = list(code)
        bad[at] = 2
        assert _rcs(_raw(pkg, ctx, "nw", bad, 2, [1, -1, -1, 1], -2, -1, pairs)) == (PWA_E_INVALID,) * 4
    assert _rcs(_raw(pkg, ctx, "nw", code, 2, [1, -1, -1, 1], 1, -1, pairs)) == (PWA_E_INVALID,) * 4
    assert _rcs(_raw(pkg, ctx, "sw", code, 2, [1, -1, -1, 1], -1, 1, pairs)) == (PWA_E_INVALID,) * 4
    assert _rcs(_raw(pkg, ctx, "nw", None, 2, [1, -1, -1, 1], -2, -1, pairs)) == (PWA_E_INVALID,) * 4
    assert _rcs(_raw(pkg, ctx, "nw", code, 2, None, -2, -1, pairs)) == (PWA_E_INVALID,) * 4
    assert _rcs(_raw(pkg, ctx, "nw", code, 2, [1, -1, -1, 1], -2, -1, [])) == (0, 0, 0, 0)   # an empty list is fine


@pytest.mark.parametrize("mode", MODES)
def test_shape_and_range_limits(pkg, ctx, mode):
    rng = random.Random(110)
    code = [0, 1] * 128
    alpha = bytes([0, 1])
    assert _rcs(_raw(pkg, ctx, mode, code, 2, [1, -1, -1, 1], -2, -1, [(_rand(rng, 1025, alpha), _rand(rng, 30, alpha))])) == (PWA_E_CAPACITY,) * 4
    # (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|) < 2^28: the largest admitted entry, and one more
    p, t = _rand(rng, 40, alpha), _rand(rng, 58, alpha)
    top = ((1 << 28) - 1) // (len(p) + len(t) + 2)
    for entry in (top, -top):
        sub = [3, entry, -2, 3]
        table = (np.array(code, np.uint8), 2, np.array(sub, np.int32))
        check(ctx, mode, [(p, t)], [GO.align(p, t, mode, table, -2, -1)], table, -2, -1)
        over = [3, entry + (1 if entry > 0 else -1), -2, 3]
        assert _rcs(_raw(pkg, ctx, mode, code, 2, over, -2, -1, [(p, t)])) == (PWA_E_CAPACITY,) * 4
        assert _rcs(_raw(pkg, ctx, mode, code, 2, over, -2, -1, [(b"\x00", b"\x01"), (p, t), (b"", b"\x01")])) == (PWA_E_CAPACITY,) * 4
        assert _rcs(_raw(pkg, ctx, mode, code, 2, over, -2, -1, [(p[:20], t)])) == (0, 0, 0, 0)   # a shorter pair admits it


@pytest.mark.parametrize("mode", MODES)
def test_cigar_capacity(pkg, ctx, mode):
    table = random_table(45, PROTEIN, unknown=0)   # (the raw C call below takes the map as it is: every byte needs a code)
    rng = random.Random(120)
    pairs = []
    for n in (0, 5, 150, 300):
        p = _rand(rng, n, PROTEIN)
        pairs.append((p, _mutate(rng, p, PROTEIN) + _rand(rng, 25, PROTEIN)))
    want = ctx.align_subst_batch_cigar(mode, *_batch(pairs), table, -11, -1)
    need = (sum(len(w["cigar"]) for w in want), sum(len(w["mdz"]) for w in want))
    code, n_sym, submat = table
    args = (pkg, ctx, mode, code.tolist(), n_sym, submat.tolist(), -11, -1, pairs)
    assert _raw(*args)[1:3] == (0, need)
    assert _raw(*args, cigar_cap=need[0] - 1)[1:3] == (PWA_E_CAPACITY, need)
    assert _raw(*args, cigar_cap=need[0])[1:3] == (0, need)
