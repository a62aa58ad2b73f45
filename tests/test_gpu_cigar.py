"""pwa_align_batch_cigar: CIGAR and MD:Z strings of whole alignment batches built on the device.

Every check is on exact bytes: against the reference's fixtures, against the oracle (a C restatement of hw2.cpp), and against
pwa_align_batch + the host formatter pwa_format_alignment on the same lists."""
import ctypes as C
import hashlib
import random
from collections import defaultdict

import pytest

import oracle_lib as O
from conftest import B, load_golden, switched_context

pytestmark = pytest.mark.gpu

SCORINGS = [(1, -1, -1), (2, -3, -5), (5, -4, -4), (0, 0, 0), (1, 1, 1), (-1, 2, 1), (1, -1, 0), (20, -15, -9)]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def fmt(p, t, ops, start):
    """prepareCigarString / prepareMDZString (hw2.cpp:59-116) over an op list in traceback order, in Python: the oracle returns
    C strings, which end at a NUL byte; this does not."""
    fw = ops[::-1]
    i, j = start
    ap, ar = bytearray(), bytearray()
    for o in fw:
        if o == 77:     # M
            ap.append(p[i]); ar.append(t[j]); i += 1; j += 1
        elif o == 68:   # D
            ap.append(p[i]); ar.append(45); i += 1
        else:           # I
            ap.append(45); ar.append(t[j]); j += 1
    cg, k = bytearray(), 0
    while k < len(fw):
        r = k
        while r < len(fw) and fw[r] == fw[k]:
            r += 1
        cg += b"%d" % (r - k) + bytes([fw[k]])
        k = r
    md, mt, c = bytearray(), 0, 0
    while c < len(fw):
        if fw[c] == 77:
            if ap[c] == ar[c]:
                mt += 1
            else:
                md += b"%d" % mt + bytes([ar[c]])
                mt = 0
            c += 1
        elif fw[c] == 68:
            md += b"%d^" % mt
            mt = 0
            while c < len(fw) and fw[c] == 68:
                md.append(ap[c])
                c += 1
        else:
            c += 1
    md += b"%d" % mt
    return bytes(cg), bytes(md)


def batch(c, mode, pairs, sc):
    """pairs: [(pattern, text)] -> align_batch_cigar over a list with every sequence once"""
    seqs = [x for pt in pairs for x in pt]
    return c.align_batch_cigar(mode, seqs, list(range(0, 2 * len(pairs), 2)), list(range(1, 2 * len(pairs), 2)), *sc)


def check_oracle(c, mode, pairs, sc, why=""):
    got = batch(c, mode, pairs, sc)
    for k, (p, t) in enumerate(pairs):
        w = O.align(mode, p, t, *sc)
        assert got[k]["score"] == w["score"], (why, mode, sc, k)
        assert (got[k]["cigar"], got[k]["mdz"]) == fmt(p, t, w["ops"], w["start"]), (why, mode, sc, k)
        if 0 not in p and 0 not in t:   # the oracle's own strings (C strings)
            assert (got[k]["cigar"], got[k]["mdz"]) == (w["cigar"], w["mdz"]), (why, mode, sc, k)
        assert tuple(got[k]["end"]) == tuple(w["end"]) and tuple(got[k]["start"]) == tuple(w["start"]), (why, mode, sc, k)


def mutate(rng, s, rate, alphabet=b"ACGT"):
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alphabet))
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out.append(ch)
            out.append(rng.choice(alphabet))
        else:
            out.append(ch)
    return bytes(out)


def indel_blocks(rng, s, n_events, max_len):
    out = bytearray(s)
    for _ in range(n_events):
        at = rng.randrange(0, max(1, len(out)))
        ln = rng.randint(1, max_len)
        if rng.random() < 0.5:
            del out[at:at + ln]
        else:
            out[at:at] = bytes(rng.choice(b"ACGT") for _ in range(ln))
    return bytes(out)


# ------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize("name", ["bundled", "edge", "random", "dash"])
def test_cigar_batch_matches_reference_fixtures(ctx, name):
    groups = defaultdict(list)
    for rec in load_golden(name):
        groups[(rec["mode"], tuple(rec["scoring"]))].append(rec)
    for (mode, sc), recs in groups.items():
        got = batch(ctx, mode, [(B(r["p"]), B(r["t"])) for r in recs], sc)
        for g, r in zip(got, recs):
            assert (g["score"], g["cigar"], g["mdz"]) == (r["score"], B(r["cigar"]), B(r["mdz"])), (name, mode, sc, r["p"], r["t"])


@pytest.mark.parametrize("name", ["kat", "bigscore"])
def test_cigar_batch_matches_reference_hashes(ctx, name):
    """kat: generator pairs up to 10k x 10k; bigscore: scores x lengths beyond the packed keys (the plain int32 walk)"""
    groups = defaultdict(list)
    for rec in load_golden(name):
        groups[(rec["mode"], tuple(rec["scoring"]))].append(rec)
    for (mode, sc), recs in groups.items():
        got = batch(ctx, mode, [(O.gen(*r["gen_p"]), O.gen(*r["gen_t"])) for r in recs], sc)
        for g, r in zip(got, recs):
            assert g["score"] == r["score"], (name, mode, sc)
            assert sha(g["cigar"]) == r["cigar_sha256"] and sha(g["mdz"]) == r["mdz_sha256"], (name, mode, sc, r["gen_p"])


# ------------------------------------------------------------------ 2. the oracle, on every engine class
ENGINES = {"mini": {}, "wide": {"PWA_TB_ENGINE": "2"}, "stripes": {"PWA_TB_ENGINE": "0"}, "stripes_rl4": {"PWA_FORCE_RL": "4"},
           "int32": {"PWA_NO_KEYED_TB": "1"}, "raw": {"PWA_NO_PAIR_TABLE": "1"}}


@pytest.mark.parametrize("engine", list(ENGINES))
def test_cigar_batch_matches_oracle_on_every_engine(engine):
    rng = random.Random(sum(engine.encode()))
    with switched_context(**ENGINES[engine]) as c:
        for alphabet in (b"ACGT", b"ACDEFGHIKLMNPQRSTVWY"):
            pairs = []
            for rows in (1, 37, 150, 256, 300, 700, 1024, 1500):
                for _ in range(2):
                    p = bytes(rng.choice(alphabet) for _ in range(rows))
                    t = mutate(rng, p, rng.choice([0.03, 0.2]), alphabet) if rng.random() < 0.6 else \
                        bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 2 * rows + 10)))
                    pairs.append((p, t))
            for mode in ("nw", "sw"):
                for sc in rng.sample(SCORINGS, 3):
                    check_oracle(c, mode, pairs, sc, (engine, alphabet[:4]))


@pytest.mark.parametrize("table", [True, False])
def test_cigar_batch_dash_and_nul_bytes(table):
    """'-' inside the sequences (MD:Z prints it like any symbol) and a NUL byte (raw arena; the strings may hold NUL)"""
    rng = random.Random(3)
    with switched_context(**({} if table else {"PWA_NO_PAIR_TABLE": "1"})) as c:
        for alphabet in (b"AC-T", b"AC\x00T", b"A-\x00"):
            pairs = []
            for rows in (5, 64, 200, 600):
                p = bytes(rng.choice(alphabet) for _ in range(rows))
                pairs.append((p, mutate(rng, p, 0.15, alphabet)))
                pairs.append((p, bytes(rng.choice(alphabet) for _ in range(rows + 7))))
            for mode in ("nw", "sw"):
                for sc in [(1, -1, -1), (2, -3, -5), (1, 1, 1)]:
                    check_oracle(c, mode, pairs, sc, alphabet)


# ------------------------------------------------------------------ 3. agreement with align_batch + format_alignment
def _agree(c, pkg, mode, seqs, pa, pb, sc):
    got = c.align_batch_cigar(mode, seqs, pa, pb, *sc)
    ref = c.align_batch(mode, seqs, pa, pb, *sc)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert (g["score"], tuple(g["end"]), tuple(g["start"])) == (r["score"], tuple(r["end"]), tuple(r["start"])), (mode, k)
        f = pkg.format_alignment(seqs[pa[k]], seqs[pb[k]], r["ops"], r["end"])
        assert (g["cigar"], g["mdz"]) == (f["cigar"], f["mdz"]), (mode, k)


def test_cigar_batch_agrees_with_align_batch(ctx, pkg):
    rng = random.Random(21)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 1200))) for _ in range(50)]
    seqs += [mutate(rng, s, 0.05) for s in seqs[:20]]
    pa = [rng.randrange(len(seqs)) for _ in range(300)] + list(range(20))
    pb = [rng.randrange(len(seqs)) for _ in range(300)] + list(range(50, 70))
    for mode in ("nw", "sw"):
        for sc in [(1, -1, -1), (5, -4, -4)]:
            _agree(ctx, pkg, mode, seqs, pa, pb, sc)


def test_cigar_batch_agrees_on_the_g_shape(ctx, pkg):
    """the -g shape at full size: 4096 NW pairs of 150 x 10k (64 texts)"""
    texts = [O.gen(4, 1, i, 10000) for i in range(64)]
    pats = [O.gen(4, 0, i, 150) for i in range(64)]
    seqs = pats + texts
    pa = [i % 64 for i in range(4096)]
    pb = [64 + (i // 64) for i in range(4096)]
    _agree(ctx, pkg, "nw", seqs, pa, pb, (1, -1, -1))


# ------------------------------------------------------------------ 4. long runs and multi-digit counts
def test_cigar_batch_long_runs(ctx):
    rng = random.Random(9)
    same = O.gen(5, 0, 0, 10000)
    got = batch(ctx, "nw", [(same, same)], (1, -1, -1))[0]
    assert (got["cigar"], got["mdz"]) == (b"10000M", b"10000")
    got = batch(ctx, "sw", [(same, same)], (1, -1, -1))[0]
    assert (got["cigar"], got["mdz"]) == (b"10000M", b"10000")
    # 150 x 10k NW: I runs in the thousands
    t = O.gen(5, 1, 0, 10000)
    pairs = [(O.gen(5, 0, i, 150), t) for i in range(4)] + [(t[3000:3150], t), (t[:150], t)]
    check_oracle(ctx, "nw", pairs, (1, -1, -1), "150 x 10k")
    assert any(len(b) >= 4 for b in batch(ctx, "nw", pairs, (1, -1, -1))[4]["cigar"].split(b"I"))
    # gap runs of up to 400 columns in both directions
    pairs = []
    for n in (200, 900, 3000):
        p = bytes(rng.choice(b"ACGT") for _ in range(n))
        pairs.append((p, indel_blocks(rng, p, 4, min(400, n // 4))))
        pairs.append((indel_blocks(rng, p, 4, min(400, n // 4)), p))
    for mode in ("nw", "sw"):
        check_oracle(ctx, mode, pairs, (2, -3, -1), "indel blocks")
    # runs that straddle the kernel's 64-column sub-chunks and 256-column load batches
    pairs = []
    for L in (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513):
        x = bytes(rng.choice(b"ACGT") for _ in range(L))
        pairs.append((x, x))                                           # one M run of L
        for head in (1, 63, 64, 65):
            a, b = bytes(rng.choice(b"ACGT") for _ in range(head)), bytes(rng.choice(b"ACGT") for _ in range(100))
            g = bytes(rng.choice(b"T") for _ in range(L))
            pairs.append((a + b, a + g + b))                           # an I run of ~L after `head` columns
            pairs.append((a + g + b, a + b))                           # a D run (MD:Z: ^ + L symbols)
            pairs.append((a + b"A" * L + b, a + b"C" * L + b))         # L mismatches in a row
    for mode in ("nw", "sw"):
        for sc in [(1, -1, -1), (5, -4, -1)]:
            check_oracle(ctx, mode, pairs, sc, "chunk boundaries")


# ------------------------------------------------------------------ 5. degenerate pairs
def test_cigar_batch_degenerate_pairs(ctx):
    """empty pattern, empty text, both empty, SW all-mismatch (zero score), mixed with ordinary pairs in one list"""
    rng = random.Random(4)
    ordinary = [(O.gen(6, 0, i, 90 + i), O.gen(6, 1, i, 120)) for i in range(6)]
    degenerate = [(b"", b"ACGT"), (b"ACGTA", b""), (b"", b""), (b"AAAA", b"CCCC"), (b"A" * 300, b"C" * 700), (b"", b"-" * 1100),
                  (b"ACG-T\x00" * 50, b"")]
    pairs = ordinary + degenerate + ordinary[:2]
    rng.shuffle(pairs)
    for mode in ("nw", "sw"):
        for sc in [(1, -1, -1), (2, -3, -5)]:
            check_oracle(ctx, mode, pairs, sc, "degenerate")
    got = batch(ctx, "nw", [(b"ACGTA", b""), (b"", b"ACG"), (b"", b"")], (1, -1, -1))
    assert [(g["cigar"], g["mdz"]) for g in got] == [(b"5D", b"0^ACGTA0"), (b"3I", b"0"), (b"", b"0")]
    got = batch(ctx, "sw", [(b"ACGTA", b""), (b"", b"ACG"), (b"AAAA", b"CCCC")], (1, -1, -1))
    assert [(g["score"], g["cigar"], g["mdz"]) for g in got] == [(0, b"", b"0")] * 3


# ------------------------------------------------------------------ 6. several ranges
def test_cigar_batch_several_ranges_are_byte_identical(ctx):
    rng = random.Random(12)
    seqs = [O.gen(7, 0, i, rng.choice([0, 60, 150, 400, 900, 2500])) for i in range(40)]
    seqs += [O.gen(7, 1, i, rng.choice([0, 150, 1000, 4000])) for i in range(20)]
    pa = [rng.randrange(40) for _ in range(400)]
    pb = [40 + rng.randrange(20) for _ in range(400)]
    with switched_context(PWA_RANGE_BYTES="3145728") as c:
        for mode in ("nw", "sw"):
            one = ctx.align_batch_cigar(mode, seqs, pa, pb, 1, -1, -1)
            many = c.align_batch_cigar(mode, seqs, pa, pb, 1, -1, -1)
            assert one == many, mode


# ------------------------------------------------------------------ 7. capacity
def test_cigar_batch_capacity(ctx, pkg):
    import numpy as np
    L = pkg.lib()
    rng = random.Random(13)
    seqs = [O.gen(8, 0, i, rng.randint(0, 500)) for i in range(30)]
    blob, off, seqs = pkg.pack_sequences(seqs)
    n = 60
    pa = (C.c_uint32 * n)(*[rng.randrange(30) for _ in range(n)])
    pb = (C.c_uint32 * n)(*[rng.randrange(30) for _ in range(n)])
    u64p = C.POINTER(C.c_uint64)

    def call(cap_c, cap_m):
        cg, md = np.zeros(max(cap_c, 1), np.uint8), np.zeros(max(cap_m, 1), np.uint8)
        co, mo = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        sc = (C.c_int32 * n)()
        need = (C.c_uint64 * 2)()
        rc = L.pwa_align_batch_cigar(ctx._h, 0, 1, -1, -1, blob, off, len(seqs), pa, pb, n, sc, cg.ctypes.data_as(C.c_void_p), cap_c,
                                     co.ctypes.data_as(u64p), md.ctypes.data_as(C.c_void_p), cap_m, mo.ctypes.data_as(u64p), None, None, need)
        return rc, (need[0], need[1]), cg, co, md, mo

    rc, need, cg, co, md, mo = call(1 << 20, 1 << 20)
    assert rc == 0 and need == (int(co[n]), int(mo[n]))
    want = ctx.align_batch_cigar("nw", seqs, list(pa), list(pb), 1, -1, -1)
    assert [g["cigar"] for g in want] == [cg[int(co[k]):int(co[k + 1])].tobytes() for k in range(n)]
    assert [g["mdz"] for g in want] == [md[int(mo[k]):int(mo[k + 1])].tobytes() for k in range(n)]
    assert call(need[0] - 1, need[1])[:2] == (-5, need)
    assert call(need[0], need[1] - 1)[:2] == (-5, need)
    rc, need2, cg, co, md, mo = call(need[0], need[1])
    assert rc == 0 and need2 == need
    assert [g["cigar"] for g in want] == [cg[int(co[k]):int(co[k + 1])].tobytes() for k in range(n)]
    assert [g["mdz"] for g in want] == [md[int(mo[k]):int(mo[k + 1])].tobytes() for k in range(n)]
    assert L.pwa_align_batch_cigar(ctx._h, 0, 1, -1, -1, blob, off, len(seqs), pa, pb, n, (C.c_int32 * n)(), None, 0, None, None, 0, None,
                                   None, None, None) == -1   # PWA_E_INVALID: offsets are required
