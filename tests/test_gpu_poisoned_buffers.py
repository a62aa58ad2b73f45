"""Every call on a context whose buffers start full of junk (PWA_POISON, include/pwalign.h; the audit table is in DESIGN.md 3.20).

The library keeps device memory between calls (the context's DevMem, dev_mem.h: the thirteen slots of the pwa_align* calls, the parked
hand-off buffer, the free list of batch buffers; and the page-locked staging buffers) and never clears it on acquisition.  With
PWA_POISON=<byte> every buffer a call is handed reads as that byte until the call writes it.  Each family below runs a list of probes
twice in ONE poisoned context -- ascending size, then descending, so that small calls meet oversized retained buffers -- and compares
every specified output, field for field, with the same probe on a fresh unpoisoned context with the same other switches; the mixed
family does so across entry points, which share slots, the free list and the parked buffer.  The control's outputs are checked
against the existing oracles on a seeded sample of at most 8 items per probe.  After every probe the context's poison counters must have grown: a run that poisons nothing
cannot pass.  Everything is integer or byte exact."""
import functools
import random

import numpy as np
import pytest

import approx_locate_oracle as LO
import approx_oracle as AO
import banded_ext_oracle as XO
import banded_oracle as BO
import gotoh_oracle as GO
import oracle_lib as O
import sg_oracle as SG
from conftest import load_pkg, switched_context
from test_gpu_cigar import ENGINES, fmt, mutate   # the six engine switch sets of the alignment batches are defined there

pytestmark = pytest.mark.gpu

POISON = [0x01, 0x80, 0x7f, 0xff]   # a small count or flag; a large negative int; a large positive int / f16 NaN; -1 / the largest unsigned
BYTE_IDS = ["0x%02x" % b for b in POISON]
SAMPLE = 8
DNA = b"ACGT"
LIN = (2, -3, -5)            # match, mismatch, gap
AFF = (1, -4, -6, -1)        # match, mismatch, gap_open, gap_extend
HW3 = (5, -4, -16, -4)
HW4 = (1, -1, -2)
ARENA_LIMIT = 4096           # PWA_ARENA_LIMIT of the one-shot hw3 / hw4 calls: bytes of sequences per run


class Probe:
    """One call (or one short sequence of calls) on a context.  run(c) -> a plain comparable value; n_items, pick(out, k) and
    expect(k): item k of the output and what the oracle says it is (pick / expect None: nothing to anchor); check(out): assertions on
    the output itself (the kernel form a batch reports), run on the control and on every poisoned output."""

    def __init__(self, name, size, run, n_items=0, pick=None, expect=None, check=None):
        self.name, self.size, self.run, self.n_items, self.pick, self.expect, self.check = name, size, run, n_items, pick, expect, check

    def sample(self):
        ks = list(range(self.n_items))
        return ks if len(ks) <= SAMPLE else sorted(random.Random(len(self.name) * 7919 + self.n_items).sample(ks, SAMPLE))


def _capture(run, c):
    """a probe's outcome with its return code as part of it"""
    pkg = load_pkg()
    try:
        return ("ok", run(c))
    except pkg.PwaError as e:
        return ("error", str(e))


def _where(a, b, path="out"):
    """where two nested values first differ"""
    if type(a) is not type(b):
        return "%s: %s against %s" % (path, type(a).__name__, type(b).__name__)
    if isinstance(a, dict):
        if a.keys() != b.keys():
            return "%s: keys %s against %s" % (path, sorted(a), sorted(b))
        for k in a:
            if a[k] != b[k]:
                return _where(a[k], b[k], "%s[%r]" % (path, k))
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return "%s: %d against %d entries" % (path, len(a), len(b))
        for k, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return _where(x, y, "%s[%d]" % (path, k))
    if isinstance(a, bytes) and len(a) > 64:
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        return "%s: %d against %d bytes, first difference at %d: %r against %r" % (path, len(a), len(b), k, a[k:k + 16], b[k:k + 16])
    return "%s: %r against %r" % (path, a, b)


_CONTROL = {}
ZERO = dict(buffers=0, bytes=0)


def control(key, knobs, probes):
    """every probe on a fresh unpoisoned context of its own, anchored to the oracles; once per family and switch set"""
    if key not in _CONTROL:
        outs = []
        for p in probes:
            with switched_context(**knobs) as c:
                out = _capture(p.run, c)
                assert c.poison_stats() == ZERO, p.name
            if out[0] == "error" and "HIP" in out[1]:   # a device fault: nothing more may be started on this GPU
                pytest.exit("control %s %s: %s" % (key, p.name, out[1]), returncode=3)
            assert out[0] == "ok", (key, p.name, out)
            if p.check:
                p.check(out[1])
            for k in p.sample() if p.pick else []:
                got, want = p.pick(out[1], k), p.expect(k)
                assert got == want, "control %s %s item %d: %s" % (key, p.name, k, _where(got, want))
            outs.append(out)
        _CONTROL[key] = outs
    return _CONTROL[key]


def poisoned(key, knobs, probes, byte):
    want = control(key, knobs, probes)
    order = sorted(range(len(probes)), key=lambda i: probes[i].size)   # (stable: equal sizes keep their order)
    with switched_context(PWA_POISON="0x%02x" % byte, **knobs) as c:
        assert c.poison_stats() == ZERO
        for turn, idx in enumerate(order + order[::-1]):
            p = probes[idx]
            before = c.poison_stats()
            got = _capture(p.run, c)
            after = c.poison_stats()
            tag = "%s poison 0x%02x, %s pass, probe %s" % (key, byte, "ascending" if turn < len(order) else "descending", p.name)
            assert after["bytes"] > before["bytes"] and after["buffers"] > before["buffers"], (tag, before, after)
            if got[0] == "error" and "HIP" in got[1]:   # a device fault: nothing more may be started on this GPU
                pytest.exit("%s: %s" % (tag, got[1]), returncode=3)
            if got != want[idx]:
                pytest.fail("%s: %s" % (tag, _where(got, want[idx])))
            if p.check:
                p.check(got[1])


def _rand(rng, n, alpha=DNA):
    return bytes(rng.choice(alpha) for _ in range(n))


def _seqs(pairs):
    seqs = [x for pt in pairs for x in pt]
    return seqs, list(range(0, len(seqs), 2)), list(range(1, len(seqs), 2))


def _ints(x):
    return tuple(int(v) for v in x)


# ---- brute-force references of hw1 and of the approximate search, small enough to stand here
def signed_sa(text):
    """suffixes in signed-char order (a prefix before the longer suffix)"""
    return sorted(range(len(text)), key=lambda i: bytes(b ^ 0x80 for b in text[i:]))


def brute_count(t, p):
    if not p:
        return len(t)
    c, i = 0, t.find(p)
    while i >= 0:
        c += 1
        i = t.find(p, i + 1)
    return c


def brute_occ(t, starts, ranks, p):
    """(header rank, local position) of the occurrences of p that do not start on a reference's terminator, sorted"""
    return sorted((ranks[r], q - starts[r]) for r in range(len(starts) - 1) for q in range(starts[r], starts[r + 1] - 1) if t.startswith(p, q))


def approx_expect(text, patterns, ks):
    """per pattern its (end, dist) list from the last row of the edit-distance table"""
    out = []
    for p, k in zip(patterns, ks):
        row = AO.last_row(p, text)
        out.append([(int(x), int(row[x])) for x in np.nonzero(row[1:] <= k)[0] + 1])
    return out


# ---- PWA_POISON itself
@pytest.mark.parametrize("value", ["256", "0x", "ff", "", "-1", "0x100", "1 "])
def test_a_value_that_is_no_byte_fails_context_creation(value):
    """a run that poisons nothing must not be able to pass: pwa_ctx_create refuses the value with PWA_E_INVALID"""
    pkg = load_pkg()
    with pytest.raises(pkg.PwaError, match="invalid argument"):
        with switched_context(PWA_POISON=value):
            pass
    with switched_context(PWA_POISON="0") as c:   # ... and 0 is a byte like any other
        assert c.poison_stats() == ZERO
        assert c.scores("sw", [b"ACGT", b"ACGA"], [0], [1], *LIN) == [6]
        assert c.poison_stats()["bytes"] > 0


# ====================================================================================== 1. linear scores
@functools.lru_cache(maxsize=None)
def _lin_score(mode, p, t):
    """(score, end) of the linear oracles"""
    if mode == "sg":
        w = SG.align(p, t, *LIN, want_ops=False)
        return int(w["score"]), _ints(w["end"])
    s, ei, ej = O.score(mode, p, t, *LIN)
    return int(s), (int(ei), int(ej))


def _score_probe(tag, size, mode, seqs, pa, pb, check=None):
    """scores, scores with end cells, and two batch objects (with end cells: off the strips; without: the strips where the list admits
    them), each run twice before its fetch"""
    def run(c):
        out = dict(scores=c.scores(mode, seqs, pa, pb, *LIN), ends=c.scores(mode, seqs, pa, pb, *LIN, want_end=True))
        for key, want_end in (("batch_end", True), ("batch", False)):
            b = c.batch(mode, seqs, pa, pb, *LIN, want_end=want_end)
            try:
                forms = dict(bits=b.cell_bits(), profile=b.profile_form(), profile_int=b.profile_int(), kernel=b.info()["kernel"], tasks=b.info()["n_tasks"])
                b.run()
                b.run()
                out[key] = (b.fetch(), forms)
            finally:
                b.close()
        return out

    def pick(out, k):
        s, ei, ej = out["ends"]
        bs, bi, bj = out["batch_end"][0]
        return (out["scores"][k], (s[k], (ei[k], ej[k])), (bs[k], (bi[k], bj[k])), out["batch"][0][k])

    def expect(k):
        s, end = _lin_score(mode, seqs[pa[k]], seqs[pb[k]])
        return (s, (s, end), (s, end), s)

    return Probe("%s/%s/%s" % (tag, mode, size), len(pa), run, len(pa), pick, expect, check)


@functools.lru_cache(maxsize=None)
def _strip_lists():
    """70 patterns of 1 .. 152 rows and 10 of 560 .. 620 (eight and more strips, which cross the hand-off workspace) against texts of
    5, 257 and 1403 symbols; three nested lists"""
    rng = random.Random(2001)
    pats = [_rand(rng, 1 + 151 * i // 69) for i in range(70)] + [_rand(rng, 560 + 60 * i // 9) for i in range(10)]
    assert len(pats[0]) == 1 and len(pats[69]) == 152 and len(pats[70]) == 560 and len(pats[79]) == 620
    texts = [_rand(rng, m) for m in (5, 257, 1403)]
    seqs = pats + texts

    def cross(ps, ts):
        return seqs, [p for p in ps for _ in ts], [80 + t for _ in ps for t in ts]
    return [("small", cross(range(0, 70, 9), [0])), ("medium", cross(range(70), [0, 1])), ("large", cross(range(80), [0, 1, 2]))]


@functools.lru_cache(maxsize=None)
def _stripe_lists():
    """6 pairs of 300 .. 1500 x 200 .. 3000 for the stripe route"""
    rng = random.Random(2002)
    shapes = [(300, 200), (513, 257), (1024, 1500), (700, 3000), (1500, 2000), (1100, 900)]
    pairs = []
    for n, m in shapes:
        p = _rand(rng, n)
        t = (mutate(rng, p, 0.1) + _rand(rng, m))[:m] if n < m else _rand(rng, m)
        pairs.append((p, t))
    return [(name, _seqs(pairs[:k])) for name, k in (("small", 2), ("medium", 4), ("large", 6))]


@functools.lru_cache(maxsize=None)
def _profile_lists():
    """the list of test_gpu_scores_profile.test_pattern_lengths_and_ragged_texts (every pattern length class of the profile form, every
    text length residue mod 8), and its first four patterns against its first six texts"""
    rng = random.Random(505)
    pats = [_rand(rng, n) for n in list(range(1, 153, 7)) + [150, 151, 152]]
    txts = [_rand(rng, m) for m in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257, 1001, 1002, 1003)]
    seqs = pats + txts

    def cross(np_, nt):
        return seqs, [i for i in range(np_) for _ in range(nt)], [len(pats) + j for _ in range(np_) for j in range(nt)]
    return [("small", cross(4, 6)), ("large", cross(len(pats), len(txts)))]


def _forms(bits=None, profile=None, profile_int=None):
    def check(out):
        f = out["batch"][1]
        assert bits is None or f["bits"] == bits, f
        assert profile is None or f["profile"] == profile, f
        assert profile_int is None or f["profile_int"] == profile_int, f
    return check


SCORE_SETS = {
    "strips_int32": (dict(PWA_SCORES_ROUTE="0", PWA_CELL16="0"), _strip_lists, ("nw", "sw", "sg"), dict(sw=_forms(bits=32))),
    "strips_cell16": (dict(PWA_SCORES_ROUTE="0", PWA_CELL16="1"), _strip_lists, ("nw", "sw", "sg"), dict(sw=_forms(bits=16))),
    "stripes": (dict(PWA_SCORES_ROUTE="1"), _stripe_lists, ("nw", "sw", "sg"), dict(sw=_forms(bits=0), nw=_forms(bits=0))),
    "profile_f16": (dict(PWA_SCORES_ROUTE="0", PWA_FORCE_LANES="0", PWA_CELL16="1", PWA_PROF16="1", PWA_PROF16_INT="0"), _profile_lists, ("sw",),
                    dict(sw=_forms(bits=16, profile=1, profile_int=0))),
    "profile_int": (dict(PWA_SCORES_ROUTE="0", PWA_FORCE_LANES="0", PWA_CELL16="1", PWA_PROF16="1"), _profile_lists, ("sw",),
                    dict(sw=_forms(bits=16, profile=1, profile_int=1))),
}


@functools.lru_cache(maxsize=None)
def _score_probes(name):
    _, lists, modes, checks = SCORE_SETS[name]
    # (the form checks skip the small strip list: its one text of 5 symbols does not hold every pattern symbol, which the packed cells need)
    return [_score_probe(name, size, mode, *lst, check=checks.get(mode) if (size != "small" or lists is not _strip_lists) else None)
            for mode in modes for size, lst in lists()]


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
@pytest.mark.parametrize("name", list(SCORE_SETS))
def test_linear_scores(name, byte):
    poisoned(("linear scores", name), SCORE_SETS[name][0], _score_probes(name), byte)


# ====================================================================================== 2. hw3 and hw4 passes
@functools.lru_cache(maxsize=None)
def _family_seqs():
    """12 related sequences of 40 .. 1500 symbols; all pairs of the first 4, 8 and 12.  The library reports no run count, so
    `_one_shot_runs` restates the rule by which scores_in_arena_chunks cuts a list (pwalign.hip) and every list must take three
    runs and more under it: the first four sequences are long ones for that reason"""
    rng = random.Random(2003)
    base = _rand(rng, 1800)
    lens = [1500, 1200, 1024, 40, 64, 257, 100, 513, 700, 333, 900, 1499]
    seqs = [mutate(rng, base[:n + 40 + n // 5], 0.1)[:n] for n in lens]
    assert sorted(len(s) for s in seqs) == sorted(lens)
    out = []
    for name, n in (("small", 4), ("medium", 8), ("large", 12)):
        pa = [i for i in range(n) for j in range(i + 1, n)]
        pb = [j for i in range(n) for j in range(i + 1, n)]
        assert _one_shot_runs(seqs, pa, pb) >= 3, name
        out.append((name, seqs, pa, pb))
    return out


def _one_shot_runs(seqs, pa, pb):
    """runs of a one-shot call: consecutive pairs while 512 bytes + every distinct sequence of the run, each as len + 1 rounded up to
    16, stay within PWA_ARENA_LIMIT; a run holds at least one pair"""
    runs, k0 = 0, 0
    while k0 < len(pa):
        used, size, k1 = set(), 512, k0
        while k1 < len(pa):
            add = sum((len(seqs[x]) + 16) // 16 * 16 for x in {pa[k1], pb[k1]} - used)
            if size + add > ARENA_LIMIT and k1 > k0:
                break
            size += add
            used |= {pa[k1], pb[k1]}
            k1 += 1
        runs, k0 = runs + 1, k1
    return runs


@functools.lru_cache(maxsize=None)
def _hw3(a, b):
    w = O.affine_align(a, b, *HW3)
    assert w["score"] == O.affine_score(a, b, *HW3)
    return int(w["score"]), w["ops"]


def _family_probes():
    probes = []
    for size, seqs, pa, pb in _family_seqs():
        def aff(k, seqs=seqs, pa=pa, pb=pb):
            return _hw3(seqs[pa[k]], seqs[pb[k]])[0]

        def dist(k, seqs=seqs, pa=pa, pb=pb):
            return int(O.nw_distance(seqs[pa[k]], seqs[pb[k]], *HW4)[0])

        def align(k, seqs=seqs, pa=pa, pb=pb):
            s, ops = _hw3(seqs[pa[k]], seqs[pb[k]])
            return dict(score=s, ops=ops)
        n = len(pa)
        item = lambda out, k: out[k]
        probes += [
            Probe("scores_affine/" + size, n, lambda c, a=(seqs, pa, pb): c.scores_affine(*a, *HW3), n, item, aff),
            Probe("scores_affine_oneshot/" + size, n, lambda c, a=(seqs, pa, pb): c.scores_affine_oneshot(*a, *HW3), n, item, aff),
            Probe("distances/" + size, n, lambda c, a=(seqs, pa, pb): c.distances(*a, *HW4), n, item, dist),
            Probe("distances_oneshot/" + size, n, lambda c, a=(seqs, pa, pb): c.distances_oneshot(*a, *HW4), n, item, dist),
            Probe("align_affine_batch/" + size, n, lambda c, a=(seqs, pa, pb): c.align_affine_batch(*a, *HW3), n, item, align),
        ]
    return probes


FAMILY_SETS = {"strips": dict(PWA_SCORES_ROUTE="0", PWA_AFFINE_TB_ROUTE="0", PWA_ARENA_LIMIT=str(ARENA_LIMIT)),
               "stripes": dict(PWA_SCORES_ROUTE="1", PWA_AFFINE_TB_ROUTE="1", PWA_ARENA_LIMIT=str(ARENA_LIMIT))}


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
@pytest.mark.parametrize("name", list(FAMILY_SETS))
def test_hw3_and_hw4_passes(name, byte):
    poisoned(("hw3 hw4", name), FAMILY_SETS[name], _family_probes(), byte)


# ====================================================================================== 3. linear alignments
ROWS = (1, 37, 150, 256, 300, 700, 1024, 1500)
EMPTY_SIDES = [(b"", b"ACGTTGCA"), (b"GATTACA", b""), (b"", b"")]


@functools.lru_cache(maxsize=None)
def _lin_align(mode, p, t):
    """the linear oracles' alignment of one pair: score, end, start, ops, the strings of those ops, overlap (nw, sw)"""
    if mode == "sg":
        w = SG.align(p, t, *LIN)
        out = dict(score=int(w["score"]), end=_ints(w["end"]), start=_ints(w["start"]), ops=bytes(w["ops"]))
    else:
        w = O.align(mode, p, t, *LIN)
        out = dict(score=int(w["score"]), end=_ints(w["end"]), start=_ints(w["start"]), ops=bytes(w["ops"]), overlap=int(w["overlap"]))
    out["cigar"], out["mdz"] = fmt(p, t, out["ops"], out["start"])
    return out


@functools.lru_cache(maxsize=None)
def _align_lists():
    """per pattern length a mutated copy of the pattern and a random text; the three pairs with an empty side in every list"""
    rng = random.Random(2004)
    pairs = {}
    for n in ROWS:
        p = _rand(rng, n)
        pairs[n] = [(p, mutate(rng, p, 0.12) or b"A"), (_rand(rng, n), _rand(rng, rng.randint(1, n + n // 2 + 10)))]

    def lst(rows, both):
        return [pt for n in rows for pt in pairs[n][:2 if both else 1]] + EMPTY_SIDES
    return pairs, [("small", lst(ROWS[:3], False)), ("medium", lst(ROWS[:6], False)), ("large", lst(ROWS, True))]


def _keys(d, *names):
    return {k: d[k] for k in names}


@functools.lru_cache(maxsize=None)
def _lin_matrices(mode, p, t):
    """the linear oracles' score and traceback matrices of one pair, as the matrices probe returns them"""
    if mode == "sg":
        w = SG.align(p, t, *LIN, mats=True)
        dp, tb = w["dp"], w["tb"]
    else:
        dp, tb = O.matrices(mode, p, t, *LIN)
    return (dp.shape, np.ascontiguousarray(dp, dtype=np.int32).tobytes(), np.ascontiguousarray(tb, dtype=np.uint8).tobytes())


def _align_probes():
    pairs, lists = _align_lists()
    probes = []
    for mode in ("nw", "sw", "sg"):
        def want(pr, k, *names, mode=mode):
            return _keys(_lin_align(mode, *pr[k]), *names)
        for size, pr in lists:
            seqs, pa, pb = _seqs(pr)
            n = len(pr)
            item = lambda out, k: out[k]
            probes.append(Probe("align_batch/%s/%s" % (mode, size), n, lambda c, a=(mode, seqs, pa, pb): c.align_batch(*a, *LIN), n, item,
                                lambda k, pr=pr, want=want: want(pr, k, "score", "ops", "end", "start")))
            probes.append(Probe("align_batch_cigar/%s/%s" % (mode, size), n, lambda c, a=(mode, seqs, pa, pb): c.align_batch_cigar(*a, *LIN), n, item,
                                lambda k, pr=pr, want=want: want(pr, k, "score", "cigar", "mdz", "end", "start")))
            if mode != "sg" and size != "medium":
                probes.append(Probe("overlaps/%s/%s" % (mode, size), n, lambda c, a=(mode, seqs, pa, pb): c.overlaps(*a, *LIN), n,
                                    lambda out, k: (out[0][k], out[1][k]),
                                    lambda k, pr=pr, mode=mode: (_lin_align(mode, *pr[k])["score"], _lin_align(mode, *pr[k])["overlap"])))
            if size == "medium":   # op regions that do not tile: the op lists come back through the staging copy
                probes.append(Probe("align_batch_padded/%s" % mode, n, lambda c, a=(mode, seqs, pa, pb): c.align_batch(*a, *LIN, region_pad=64), n, item,
                                    lambda k, pr=pr, want=want: want(pr, k, "score", "ops", "end", "start")))

                def with_score_band(c, a=(mode, seqs, pa, pb)):
                    c.set_score_band(True)
                    try:
                        return c.align_batch(*a, *LIN)
                    finally:
                        c.set_score_band(False)
                probes.append(Probe("align_batch_score_band/%s" % mode, n, with_score_band, n, item,
                                    lambda k, pr=pr, want=want: want(pr, k, "score", "ops", "end", "start")))
        for rows in ROWS:
            p, t = pairs[rows][0]
            probes.append(Probe("align/%s/%d" % (mode, rows), rows, lambda c, a=(mode, p, t): c.align(*a, *LIN, raw=True), 1, lambda out, k: out,
                                lambda k, a=(mode, p, t): _keys(_lin_align(*a), "score", "ops", "end", "start")))
        for rows in ROWS:
            p, t = pairs[rows][0]

            def matrices(c, a=(mode, p, t)):
                c.set_score_band(True)
                try:
                    dp, tb = c.matrices(*a, *LIN)
                finally:
                    c.set_score_band(False)
                return (dp.shape, dp.tobytes(), tb.tobytes())

            probes.append(Probe("matrices/%s/%d" % (mode, rows), rows, matrices, 1, lambda out, k: out, lambda k, a=(mode, p, t): _lin_matrices(*a)))
    return probes


ALIGN_SETS = dict(ENGINES, no_gap_shift={"PWA_NO_GAP_SHIFT": "1"}, no_tiled_ops={"PWA_NO_TILED_OPS": "1"}, ranges={"PWA_RANGE_BYTES": "3145728"})


@functools.lru_cache(maxsize=None)
def _align_probes_once():
    return _align_probes()


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
@pytest.mark.parametrize("name", list(ALIGN_SETS))
def test_linear_alignments(name, byte):
    poisoned(("linear alignments", name), ALIGN_SETS[name], _align_probes_once(), byte)


# ====================================================================================== 4. gotoh and substitution tables
GOTOH_ROWS = ROWS[:7]   # the gotoh kernels take patterns of at most 1024 rows


@functools.lru_cache(maxsize=None)
def _table():
    t = GO.random_table(77, DNA)
    m = np.asarray(t[2]).reshape(4, 4)
    assert (m != m.T).any()
    return t


def _scoring(kind):
    """the oracle's scoring value: (match, mismatch), or the table"""
    return AFF[:2] if kind == "gotoh" else _table()


@functools.lru_cache(maxsize=None)
def _gotoh_align(kind, mode, p, t):
    w = GO.align(p, t, mode, _scoring(kind), AFF[2], AFF[3])
    out = dict(score=int(w["score"]), end=_ints(w["end"]), start=_ints(w["start"]), ops=bytes(w["ops"]))
    out["cigar"], out["mdz"] = fmt(p, t, out["ops"], out["start"])
    return out


@functools.lru_cache(maxsize=None)
def _gotoh_lists():
    rng = random.Random(2005)
    pairs = {}
    for n in GOTOH_ROWS:
        p = _rand(rng, n)
        pairs[n] = [(p, mutate(rng, p, 0.12) or b"A"), (_rand(rng, n), _rand(rng, rng.randint(1, n + n // 2 + 10)))]

    def lst(rows, both):
        return [pt for n in rows for pt in pairs[n][:2 if both else 1]] + EMPTY_SIDES
    return [("small", lst(GOTOH_ROWS[:3], False)), ("medium", lst(GOTOH_ROWS[:5], False)), ("large", lst(GOTOH_ROWS, True))]


def _gotoh_probes():
    probes = []
    for kind in ("gotoh", "subst"):
        for mode in ("nw", "sw", "sg"):
            for size, pr in _gotoh_lists():
                seqs, pa, pb = _seqs(pr)
                n = len(pr)
                if kind == "gotoh":
                    head = (mode, seqs, pa, pb, *AFF)
                    calls = dict(scores=lambda c, h=head: c.scores_gotoh(*h), batch=lambda c, h=head: c.batch_gotoh(*h, want_end=True),
                                 align=lambda c, h=head: c.align_gotoh_batch(*h), cigar=lambda c, h=head: c.align_gotoh_batch_cigar(*h))
                else:
                    head = (mode, seqs, pa, pb, _table(), AFF[2], AFF[3])
                    calls = dict(scores=lambda c, h=head: c.scores_subst(*h), batch=lambda c, h=head: c.batch_subst(*h, want_end=True),
                                 align=lambda c, h=head: c.align_subst_batch(*h), cigar=lambda c, h=head: c.align_subst_batch_cigar(*h))

                def want(k, *names, a=(kind, mode), pr=pr):
                    return _keys(_gotoh_align(*a, *pr[k]), *names)

                def run_batch(c, make=calls["batch"]):
                    b = make(c)
                    try:
                        b.run()
                        b.run()
                        return b.fetch()
                    finally:
                        b.close()
                tag = "%s/%s/%s" % (kind, mode, size)
                probes.append(Probe("scores/" + tag, n, calls["scores"], n, lambda out, k: out[k], lambda k, want=want: want(k, "score")["score"]))
                probes.append(Probe("batch/" + tag, n, run_batch, n, lambda out, k: (out[0][k], (out[1][k], out[2][k])),
                                    lambda k, want=want: (want(k, "score")["score"], want(k, "end")["end"])))
                probes.append(Probe("align/" + tag, n, calls["align"], n, lambda out, k: out[k], lambda k, want=want: want(k, "score", "ops", "end", "start")))
                probes.append(Probe("cigar/" + tag, n, calls["cigar"], n, lambda out, k: out[k],
                                    lambda k, want=want: want(k, "score", "cigar", "mdz", "end", "start")))
    return probes


@functools.lru_cache(maxsize=None)
def _gotoh_probes_once():
    return _gotoh_probes()


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
def test_gotoh_and_substitution_tables(byte):
    poisoned(("gotoh subst", "default"), {}, _gotoh_probes_once(), byte)


# ====================================================================================== 5. the banded class
BANDED_ROWS = (100, 513, 3000)   # one stripe of either height; two 256-row stripes, one 512-row stripe and a row; twelve / six stripes
MAX_WIDTH = 4096
XDROPS = (-1, 30)


@functools.lru_cache(maxsize=None)
def _banded_cases():
    """per pattern length: a substitutions-only copy under bands of width 1 and 33; a copy with indels under a random band and under
    full cover (where that fits the widest band); per mode, valid bands only.  EXT: a copy that turns into noise after 60 % of
    the pattern, so that the drop of 30 stops early"""
    rng = random.Random(2006)
    cases = {mode: {} for mode in ("nw", "sw", "sg", "ext")}
    for n in BANDED_ROWS:
        p = _rand(rng, n)
        subs = bytes(rng.choice(DNA) if rng.random() < 0.05 else x for x in p)
        indel = mutate(rng, p, 0.06)
        m = len(indel)
        for mode in ("nw", "sw", "sg"):
            lst = [((p, subs), (0, 0)), ((p, subs), (-16, 16))]
            for _ in range(50):
                b = BO.random_band(rng, mode, n, m)
                if b[1] - b[0] + 1 <= MAX_WIDTH:
                    break
            else:
                b = (min(0, m - n) - 5, max(0, m - n) + 5)
            lst.append(((p, indel), b))
            if n + m + 1 <= MAX_WIDTH:
                lst.append(((p, indel), (-n, m)))
            assert all(BO.band_valid(mode, len(a), len(t), *bd) for (a, t), bd in lst)
            cases[mode][n] = lst
        cut = n * 6 // 10
        turn = mutate(rng, p[:cut], 0.05) + _rand(rng, n - cut + 20)
        lst = [((p, subs), (0, 0)), ((p, turn), (-16, 16)), ((p, turn), (-rng.randint(1, 40), rng.randint(1, 40)))]
        if n + len(turn) + 1 <= MAX_WIDTH:
            lst.append(((p, turn), (-n, len(turn))))
        cases["ext"][n] = lst
    sizes = [("small", BANDED_ROWS[:1]), ("medium", BANDED_ROWS[:2]), ("large", BANDED_ROWS)]
    for mode in ("nw", "sw", "sg"):   # (full cover is valid in every mode, also for the pairs with an empty side)
        assert all(BO.band_valid(mode, len(p), len(t), -len(p), len(t)) for p, t in EMPTY_SIDES)
    return {mode: [(size, [c for n in rows for c in by_n[n]] + [(pt, (-len(pt[0]), len(pt[1]))) for pt in EMPTY_SIDES]) for size, rows in sizes] for mode, by_n in cases.items()}


@functools.lru_cache(maxsize=None)
def _banded_align(kind, mode, p, t, band):
    w = BO.align(p, t, band, mode, _scoring(kind), AFF[2], AFF[3])
    out = dict(score=int(w["score"]), end=_ints(w["end"]), start=_ints(w["start"]), ops=bytes(w["ops"]))
    out["cigar"], out["mdz"] = fmt(p, t, out["ops"], out["start"])
    return out


@functools.lru_cache(maxsize=None)
def _banded_ext(kind, p, t, band, xdrop):
    w = XO.extend(p, t, band, _scoring(kind), AFF[2], AFF[3], xdrop)
    out = dict(score=int(w["score"]), end=_ints(w["end"]), start=(0, 0), ops=bytes(w["ops"]), rows=int(w["rows"]),
               pend=None if w["pend"] is None else _ints(w["pend"]))
    out["cigar"], out["mdz"] = fmt(p, t, out["ops"], (0, 0))
    return out


def _banded_probes():
    probes = []
    all_cases = _banded_cases()
    for kind in ("gotoh", "subst"):
        sub = kind == "subst"
        for mode in ("nw", "sw", "sg"):
            for size, cs in all_cases[mode]:
                pr, bands = [c[0] for c in cs], [c[1] for c in cs]
                seqs, pa, pb = _seqs(pr)
                n = len(pr)
                head = (mode, seqs, pa, pb, _table(), AFF[2], AFF[3], bands) if sub else (mode, seqs, pa, pb, *AFF, bands)
                tag = "%s/%s/%s" % (kind, mode, size)

                def want(k, *names, a=(kind, mode), pr=pr, bands=bands):
                    return _keys(_banded_align(*a, *pr[k], bands[k]), *names)
                align, cigar, scores = ((lambda c, h=head: c.align_banded_subst_batch(*h)), (lambda c, h=head: c.align_banded_subst_batch_cigar(*h)),
                                        (lambda c, h=head: (c.scores_banded_subst(*h, want_end=True), c.scores_banded_stats()["in_band_cells"]))) if sub else \
                                       ((lambda c, h=head: c.align_banded_batch(*h)), (lambda c, h=head: c.align_banded_batch_cigar(*h)),
                                        (lambda c, h=head: (c.scores_banded(*h, want_end=True), c.scores_banded_stats()["in_band_cells"])))
                probes.append(Probe("align_banded/" + tag, n, align, n, lambda out, k: out[k], lambda k, want=want: want(k, "score", "ops", "end", "start")))
                probes.append(Probe("align_banded_cigar/" + tag, n, cigar, n, lambda out, k: out[k],
                                    lambda k, want=want: want(k, "score", "cigar", "mdz", "end", "start")))
                probes.append(Probe("scores_banded/" + tag, n, scores, n, lambda out, k: (out[0][0][k], (out[0][1][k], out[0][2][k])),
                                    lambda k, want=want: (want(k, "score")["score"], want(k, "end")["end"])))
        for size, cs in all_cases["ext"]:
            pr, bands = [c[0] for c in cs], [c[1] for c in cs]
            seqs, pa, pb = _seqs(pr)
            n = len(pr)
            for xdrop in XDROPS:
                head = (seqs, pa, pb, _table(), AFF[2], AFF[3], bands, xdrop) if sub else (seqs, pa, pb, *AFF, bands, xdrop)
                tag = "%s/x%d/%s" % (kind, xdrop, size)
                names = ("score", "end", "start", "rows") + (("pend",) if sub else ())

                def want(k, *more, a=(kind,), pr=pr, bands=bands, xdrop=xdrop, names=names):
                    return _keys(_banded_ext(*a, *pr[k], bands[k], xdrop), *names, *more)
                ext, cigar, scores = ((lambda c, h=head: c.extend_banded_subst_batch(*h)), (lambda c, h=head: c.extend_banded_subst_batch_cigar(*h)),
                                      (lambda c, h=head: (c.scores_extend_banded_subst(*h, want_end=True), c.extend_banded_stats()["rows_considered"]))) if sub else \
                                     ((lambda c, h=head: c.extend_banded_batch(*h)), (lambda c, h=head: c.extend_banded_batch_cigar(*h)),
                                      (lambda c, h=head: (c.scores_extend_banded(*h, want_end=True), c.extend_banded_stats()["rows_considered"])))
                probes.append(Probe("extend_banded/" + tag, n, ext, n, lambda out, k: out[k], lambda k, want=want: want(k, "ops")))
                probes.append(Probe("extend_banded_cigar/" + tag, n, cigar, n, lambda out, k: out[k], lambda k, want=want: want(k, "cigar", "mdz")))

                def pick(out, k, sub=sub):
                    s = out[0]
                    return (s[0][k], (s[1][k], s[2][k]), s[3][k]) + ((s[4][k],) if sub else ())

                def exp(k, want=want, sub=sub):
                    w = want(k)
                    return (w["score"], w["end"], w["rows"]) + ((w["pend"],) if sub else ())
                probes.append(Probe("scores_extend_banded/" + tag, n, scores, n, pick, exp))
    return probes


@functools.lru_cache(maxsize=None)
def _banded_probes_once():
    return _banded_probes()


BANDED_SETS = {"by_width": {}, "rl4": {"PWA_BANDED_RL": "4"}, "rl8": {"PWA_BANDED_RL": "8"}}


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
@pytest.mark.parametrize("name", list(BANDED_SETS))
def test_banded_class(name, byte):
    if byte == POISON[0] and name == "by_width":   # the drop of 30 does stop some pairs early, and not all of them
        for size, cs in _banded_cases()["ext"]:
            live = [(pt, bd) for pt, bd in cs if pt[0] and pt[1]]
            rows = [_banded_ext("gotoh", *pt, bd, 30)["rows"] for pt, bd in live]
            assert any(r < len(pt[0]) for r, (pt, bd) in zip(rows, live)) and any(r == len(pt[0]) for r, (pt, bd) in zip(rows, live)), size
    poisoned(("banded", name), BANDED_SETS[name], _banded_probes_once(), byte)


# ====================================================================================== 5b. mixed: one context across entry points
def _ends(probes, prefix=""):
    """of the probes whose name starts with prefix: the first of the smallest size and the last of the largest"""
    ps = [p for p in probes if p.name.startswith(prefix)]
    lo, hi = min(p.size for p in ps), max(p.size for p in ps)
    return [next(p for p in ps if p.size == lo), next(p for p in reversed(ps) if p.size == hi)]


def _batch_probe(name, size, make, n, expect, kernel):
    """one score batch without end cells: created, run, fetched, destroyed; it must have run on the strip kernel `kernel`, the only
    user of the hand-off workspace"""
    def run(c):
        b = make(c)
        try:
            b.run()
            return (b.fetch(), b.info()["kernel"])
        finally:
            b.close()

    def check(out):
        assert out[1].startswith(kernel), out[1]
    return Probe(name, size, run, n, lambda out, k: out[0][k], expect, check)


def _hand_off_batches():
    """Three score batches that stay on the strips under the default route, with hand-off workspaces of 8 KiB, 16 KiB and 64 KiB or
    more: the small strip list (one wave task, a text of 5 columns) as NW, one strip per task, and as SW, two; the large gotoh list
    as NW, which the gotoh rule keeps on the strips -- 14 texts, so 14 tasks and 16 workgroups with 4 KiB and more each.  (The two
    linear sizes are what a library that prints them reported; the bound of the third follows from setup_strips' formula.)  A
    probe's size here is that figure in KiB: it only orders the probes."""
    seqs, pa, pb = _strip_lists()[0][1]
    pr = _gotoh_lists()[2][1]
    gs, ga, gb = _seqs(pr)
    lin = lambda mode: (lambda c: c.batch(mode, seqs, pa, pb, *LIN))
    return [_batch_probe("batch/nw/small", 8, lin("nw"), len(pa), lambda k: _lin_score("nw", seqs[pa[k]], seqs[pb[k]])[0], "batch_scores_kernel<"),
            _batch_probe("batch/sw/small", 16, lin("sw"), len(pa), lambda k: _lin_score("sw", seqs[pa[k]], seqs[pb[k]])[0], "batch_scores_kernel<"),
            _batch_probe("batch/gotoh/nw/large", 64, lambda c: c.batch_gotoh("nw", gs, ga, gb, *AFF), len(pr),
                         lambda k: _gotoh_align("gotoh", "nw", *pr[k])["score"], "batch_gotoh_kernel<")]


@functools.lru_cache(maxsize=None)
def _mixed_probes():
    """The families above run in a context each; here ONE context, default switches, serves the two ends of five of them in turn --
    the results slot and the traceback band are shared by the linear, gotoh, banded and hw3 alignment calls, the free list by every
    score batch -- and three score batches whose strip hand-off workspaces grow from one to the next, so that the ascending pass
    parks a larger buffer each time (the displaced one goes to the free list) and the descending pass takes over an oversized
    one.  (The score probes are the first and the last of the strip lists': NW and SG, whose form checks are none -- the route is
    the default one here.)"""
    probes = (_ends(_score_probes("strips_int32")) + _ends(_family_probes(), "align_affine_batch/") + _ends(_align_probes_once(), "align_batch_cigar/") +
              _ends(_gotoh_probes_once()) + _ends(_banded_probes_once()))
    assert all(p.check is None for p in probes) and len({p.name for p in probes}) == 10
    return probes + _hand_off_batches()


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
def test_mixed_entry_points_in_one_context(byte):
    poisoned(("mixed", "default"), {}, _mixed_probes(), byte)


# ====================================================================================== 6. hw1: suffix arrays and exact search
@functools.lru_cache(maxsize=None)
def _hw1_texts():
    rng = random.Random(2007)
    big = _rand(rng, 70000)
    # (70 000 random bases separate in ONE round -- a key holds 21 of them -- so the same text with a 300-base stretch repeated stands
    # beside it: that one needs a second doubling round, as the 5000 A need several)
    return [b"", b"G", _rand(rng, 17), _rand(rng, 4097), b"A" * 5000, big, big[:40000] + big[1000:1300] + big[40300:]]


def _sa_expect(t):
    if t == b"A" * len(t):
        return lambda k: len(t) - 1 - k
    if len(t) <= 5000:
        sa = signed_sa(t)
        return lambda k: sa[k]
    return None


def _sa_check(t, min_rounds):
    """a permutation; 8 seeded neighbours in signed-char order; the doubling rounds the text must take"""
    def check(out):
        sa, rounds = out
        assert sorted(sa) == list(range(len(t)))
        key = lambda i: bytes(b ^ 0x80 for b in t[i:i + 64])
        for j in random.Random(len(t)).sample(range(max(len(t) - 1, 0)), min(SAMPLE, max(len(t) - 1, 0))):
            assert key(sa[j]) < key(sa[j + 1]) or (key(sa[j]) == key(sa[j + 1]) and t[sa[j]:] < t[sa[j + 1]:]), j
        assert rounds >= min_rounds, rounds
    return check


def _hw1_probes():
    probes = []
    rng = random.Random(2008)
    for x, t in enumerate(_hw1_texts()):
        def sa(c, t=t):
            out = c.suffix_array(t)
            return (out, c.sa_stats["rounds"])
        exp = _sa_expect(t)
        probes.append(Probe("suffix_array/%d/%d" % (x, len(t)), len(t), sa, len(t) if exp else 0, (lambda out, k: out[0][k]) if exp else None, exp,
                            _sa_check(t, 2 if x in (4, 6) else 0)))
    for t in (_hw1_texts()[2], _hw1_texts()[3], _hw1_texts()[5]):
        pats = [b"", b"Z", t, t[:1]] + [t[a:a + m] for a, m in ((rng.randrange(len(t)), rng.randint(1, 12)) for _ in range(60))] + [_rand(rng, rng.randint(1, 9)) for _ in range(40)]
        probes.append(Probe("find/%d" % len(t), len(t), lambda c, a=(t, pats): c.find(*a), len(pats), lambda out, k: out[k],
                            lambda k, t=t, pats=pats: brute_count(t, pats[k])))
    for n_ref, size in ((3, 40), (9, 300)):
        seqs = [_rand(rng, rng.choice([0, 1, 5, size]), b"ACG") for _ in range(n_ref)]
        text, starts = b"", []
        for s in seqs:
            starts.append(len(text))
            text += s + b"$"
        starts.append(len(text))
        ranks = [rng.randrange(4) for _ in range(n_ref)]
        pats = [b"", b"$", b"A$", b"T"] + [_rand(rng, rng.randint(1, 4), b"ACG$") for _ in range(120)]
        probes.append(Probe("find_refs/%d" % len(text), len(text), lambda c, a=(text, pats, (starts, ranks)): c.find(*a), len(pats), lambda out, k: out[k],
                            lambda k, a=(text, starts, ranks), pats=pats: brute_occ(*a, pats[k])))
    return probes


@functools.lru_cache(maxsize=None)
def _hw1_probes_once():
    return _hw1_probes()


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
def test_hw1(byte):
    poisoned(("hw1", "chunks of 37"), dict(PWA_OCC_CHUNK_HITS="37"), _hw1_probes_once(), byte)


# ====================================================================================== 7. approximate search
@functools.lru_cache(maxsize=None)
def _approx_case():
    """a text of 3000 with mutated copies of patterns of 5, 64, 65, 130 and 512 symbols (one word, one word and a symbol, three words,
    eight words) and one pattern of a symbol the text does not hold"""
    rng = np.random.default_rng(2009)
    pats = [AO.random_seq(rng, m, DNA) for m in (5, 64, 65, 130, 512)] + [b"N" * 9]
    ks = [1, 4, 4, 8, 20, 2]
    parts = []
    for p, k in zip(pats[:5], ks):
        parts += [AO.random_seq(rng, 150, DNA), AO.mutate(rng, p, k // 2, DNA), AO.random_seq(rng, 90, DNA), p]
    text = b"".join(parts)
    text = (text + AO.random_seq(rng, 3000, DNA))[:3000]
    return text, pats, ks


@functools.lru_cache(maxsize=None)
def _approx_hits(which):
    text, pats, ks = _approx_case()
    return approx_expect(text, [pats[q] for q in which], [ks[q] for q in which])


def _approx_probes():
    text, pats, ks = _approx_case()
    assert len(text) == 3000
    probes = []
    for size, which in (("small", (0, 5)), ("medium", (0, 1, 2)), ("large", (0, 1, 2, 3, 4, 5))):
        ps, kk = [pats[q] for q in which], [ks[q] for q in which]
        hits = _approx_hits(which)
        n = len(ps)
        work = sum(len(p) for p in ps)
        stats = lambda c: (c.approx_stats["tasks"], c.approx_stats["columns"])

        def count(c, a=(text, ps, kk)):
            return (c.count_approx(*a), stats(c))

        def find(c, a=(text, ps, kk)):
            return (c.find_approx(*a), stats(c))

        def starts(c, a=(text, ps, hits)):
            out = c.starts_approx(*a)
            return (out, (c.approx_starts_stats["hits"], c.approx_starts_stats["columns"]))

        def start_of(q, x, ps=ps, hits=hits):
            e, d = hits[q][x]
            return LO.start_of(ps[q], text, e, d)

        def some(q, hits=hits):
            return list(range(len(hits[q]))) if len(hits[q]) <= 3 else [0, len(hits[q]) // 2, len(hits[q]) - 1]
        probes.append(Probe("count_approx/" + size, work, count, n, lambda out, q: (out[0][0][q], out[0][1][q]),
                            lambda q, hits=hits: (len(hits[q]), AO.best(hits[q]))))
        probes.append(Probe("find_approx/" + size, work, find, n, lambda out, q: out[0][q], lambda q, hits=hits: hits[q]))
        probes.append(Probe("starts_approx/" + size, work, starts, n, lambda out, q, some=some: [out[0][q][x] for x in some(q)],
                            lambda q, some=some, start_of=start_of: [start_of(q, x) for x in some(q)]))
        probes.append(Probe("locate_approx/" + size, work, lambda c, a=(text, ps, kk): c.locate_approx(*a), n, lambda out, q: out[q],
                            lambda q, ps=ps, kk=kk, hits=hits: [(LO.start_of(ps[q], text, e, d), e, d) for e, d in LO.minima_from_hits(hits[q], len(ps[q]), kk[q], len(text))]))
        probes.append(Probe("align_approx/" + size, work, lambda c, a=(text, ps, kk): c.align_approx(*a), n,
                            lambda out, q: [(a["start"], a["end"], a["dist"], a["score"]) for a in out[q]],
                            lambda q, ps=ps, kk=kk, hits=hits: [(LO.start_of(ps[q], text, e, d), e, d, -d) for e, d in LO.minima_from_hits(hits[q], len(ps[q]), kk[q], len(text))]))
    return probes


@functools.lru_cache(maxsize=None)
def _approx_probes_once():
    return _approx_probes()


@pytest.mark.parametrize("byte", POISON, ids=BYTE_IDS)
def test_approximate_search(byte):
    text, pats, ks = _approx_case()
    hits = _approx_hits((0, 1, 2, 3, 4, 5))
    assert all(hits[q] for q in range(5)) and not hits[5]   # planted copies are found; one pattern has no hit
    assert sum(len(h) for h in hits) > 100                   # several slices of 100 staged hits
    poisoned(("approx", "chunks"), dict(PWA_APPROX_CHUNK="64", PWA_OCC_CHUNK_HITS="100"), _approx_probes_once(), byte)
