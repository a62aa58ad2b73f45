"""bioinformatics-algorithms_amd -- MI355X-native pairwise alignment (NW / SW, linear gap, int32).

Python is only a thin ctypes binding over the C ABI of ``libpwalign.so`` (include/pwalign.h); all
compute is in hand-written HIP kernels for gfx950.  There is NO CPU fallback: if the shared library
is missing or no MI355X is visible, ``Context()`` raises.

The directory name contains a hyphen, so import it through ``load()`` in ``_loader.py`` (or
``importlib`` with ``spec_from_file_location``); tests/bench do exactly that.

Mirror of the reference interface (Local_Global_Alignment/hw2.cpp):
  ``Context.align('nw'|'sw', pattern, text, match, mismatch, gap)`` returns the five fields of the
  reference's ``AlignmentResult`` (hw2.cpp:17-23) as a dict -- what
  ``globalAlignmentNeedlemanWunsch`` (118) / ``localAlignmentSmithWaterman`` (192) return;
  ``Context.scores(...)`` is the scores-only pass over the pair loop (328-338).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PWA_LIB") or os.path.join(_HERE, "libpwalign.so")   # PWA_LIB: A/B builds in experiments
CLI_PATH = os.path.join(_HERE, "host", "hw2_amd")
HW3_CLI_PATH = os.path.join(_HERE, "host", "hw3_amd")
CLI4_PATH = os.path.join(_HERE, "host", "hw4_amd")
HW1_CLI_PATH = os.path.join(_HERE, "host", "hw1_amd")
HW1_HOST_PATH = os.path.join(_HERE, "libhw1_host.so")   # hw1's reader and DOT writer (host only, host/hw1_host.h)

MODE = {"nw": 0, "sw": 1, "global": 0, "local": 1, "sg": 2, "semiglobal": 2}   # sg: semi-global (pwalign.h, PWA_MODE_SG)

EXPORTS = [
    "pwa_version", "pwa_strerror", "pwa_selftest_host", "pwa_ctx_create", "pwa_ctx_destroy", "pwa_last_error", "pwa_ctx_set_score_band", "pwa_ctx_poison_stats", "pwa_scores",
    "pwa_batch_create", "pwa_affine_batch_create", "pwa_scores_affine", "pwa_align_affine_batch", "pwa_nwdist_batch_create", "pwa_distances", "pwa_upgma_newick", "pwa_batch_run", "pwa_batch_d_scores", "pwa_batch_set_d_scores", "pwa_batch_fetch", "pwa_batch_info", "pwa_batch_cell_bits", "pwa_batch_profile_form", "pwa_batch_profile_int", "pwa_profile_plan", "pwa_strip_table",
    "pwa_pair_form_table", "pwa_pair_forms", "pwa_pair_forms_reset",
    "pwa_batch_last_ms", "pwa_batch_run_times", "pwa_batch_destroy", "pwa_align", "pwa_align_matrices", "pwa_align_last_stats", "pwa_align_affine_last_stats", "pwa_align_batch", "pwa_align_batch_cigar", "pwa_overlaps",
    "pwa_align_gotoh_batch", "pwa_align_gotoh_batch_cigar", "pwa_align_gotoh_last_stats",
    "pwa_gotoh_batch_create", "pwa_scores_gotoh",
    "pwa_align_banded_batch", "pwa_align_banded_batch_cigar", "pwa_align_banded_last_stats",
    "pwa_scores_banded", "pwa_scores_banded_last_stats",
    "pwa_extend_banded_batch", "pwa_extend_banded_batch_cigar", "pwa_scores_extend_banded", "pwa_extend_banded_last_stats",
    "pwa_extend_banded_subst_batch", "pwa_extend_banded_subst_batch_cigar", "pwa_scores_extend_banded_subst",
    "pwa_align_subst_batch", "pwa_align_subst_batch_cigar", "pwa_subst_batch_create", "pwa_scores_subst", "pwa_align_subst_last_stats",
    "pwa_align_banded_subst_batch", "pwa_align_banded_subst_batch_cigar", "pwa_scores_banded_subst",
    "pwa_cigar_bound", "pwa_mdz_bound", "pwa_format_alignment", "pwa_alignment_overlap",
    "pwa_fasta_read", "pwa_fasta_n_seq", "pwa_fasta_bytes", "pwa_fasta_offsets", "pwa_fasta_first_seq", "pwa_fasta_free",
    "pwa_sa_create", "pwa_sa_fetch", "pwa_sa_find", "pwa_sa_occurrences", "pwa_sa_last_stats", "pwa_sa_destroy",
    "pwa_seed_plan", "pwa_sa_seed", "pwa_sa_seed_fetch", "pwa_sa_seed_last_stats",
    "pwa_mm_create", "pwa_mm_destroy", "pwa_mm_fetch", "pwa_mm_last_stats", "pwa_mm_sketch", "pwa_mm_plan", "pwa_mm_seed", "pwa_mm_seed_fetch",
    "pwa_mm_seed_last_stats", "pwa_mm_create_canonical", "pwa_mm_fetch_canonical", "pwa_mm_sketch_canonical", "pwa_mm_seed_strands",
    "pwa_approx_find", "pwa_approx_occurrences", "pwa_approx_last_stats", "pwa_approx_plan",
    "pwa_approx_starts", "pwa_approx_starts_last_stats", "pwa_approx_minima",
    "pwa_wfa_plan", "pwa_scores_wfa", "pwa_align_wfa_batch", "pwa_align_wfa_batch_cigar", "pwa_align_wfa_codes_batch",
    "pwa_align_wfa_codes_batch_cigar", "pwa_wfa_last_stats",
    "pwa_wfa_sg_plan", "pwa_scores_wfa_sg", "pwa_align_wfa_sg_batch", "pwa_align_wfa_sg_batch_cigar",
    "pwa_chain_plan", "pwa_chain_anchors", "pwa_chain_last_stats",
    "pwa_chain_top_plan", "pwa_chain_top", "pwa_chain_top_last_stats", "pwa_mapq",
]


APPROX_NO_START = 0xffffffff   # PWA_APPROX_NO_START
WFA_NONE = -(1 << 31)          # PWA_WFA_NONE: score_out of a pair the bound leaves out
CHAIN_NO_READ = 0xffffffff     # last_out of a read without anchors; pwa_chain_plan's bad_read when no read is at fault
CHAIN_ROOTED = 1               # PWA_CHAIN_ROOTED: pwa_chain_top keeps only walks that end at an anchor without a predecessor


class PwaError(RuntimeError):
    pass


def approx_plan(n, pat_len, max_dist, chunk):
    """pwa_approx_plan (host only): the tasks (pattern, scan_lo, lo, hi) of a text of n against patterns of these lengths and bounds."""
    L = lib()
    n_pat = len(pat_len)
    pl = (C.c_uint32 * max(n_pat, 1))(*pat_len)
    md = (C.c_uint32 * max(n_pat, 1))(*max_dist)
    nt = C.c_uint64(0)
    rc = L.pwa_approx_plan(n, pl, md, n_pat, chunk, None, None, None, None, 0, C.byref(nt))
    if rc not in (0, -5):
        raise PwaError("pwa_approx_plan: %s" % L.pwa_strerror(rc).decode())
    cap = nt.value
    tp = (C.c_uint32 * max(cap, 1))()
    ts, tl, th = ((C.c_uint64 * max(cap, 1))() for _ in range(3))
    rc = L.pwa_approx_plan(n, pl, md, n_pat, chunk, tp, ts, tl, th, cap, C.byref(nt))
    if rc != 0:
        raise PwaError("pwa_approx_plan: %s" % L.pwa_strerror(rc).decode())
    return [(tp[t], ts[t], tl[t], th[t]) for t in range(cap)]


def _min_scores(min_score, n):
    """min_score of the wavefront calls: None, one int, or one per pair -> an int32 array or None"""
    if min_score is None:
        return None
    ms = [min_score] * n if isinstance(min_score, int) else [int(x) for x in min_score]
    if len(ms) != n:
        raise ValueError("min_score: one value, or one per pair")
    return (C.c_int32 * max(n, 1))(*ms)


def _wfa_plan(name, n_pen, match, mismatch, gap_open, gap_extend, lengths, min_score):
    L = lib()
    k = len(lengths)
    ns = (C.c_uint64 * max(k, 1))(*[int(a) for a, _ in lengths])
    ms = (C.c_uint64 * max(k, 1))(*[int(b) for _, b in lengths])
    pen = (C.c_int32 * n_pen)()
    pm, ce = (C.c_uint64 * max(k, 1))(), (C.c_uint64 * max(k, 1))()
    rc = getattr(L, name)(match, mismatch, gap_open, gap_extend, ns, ms, _min_scores(min_score, k), k, pen, pm, ce)
    if rc != 0:
        raise PwaError("%s: %s" % (name, L.pwa_strerror(rc).decode()))
    return dict(pen=tuple(pen), p_max=[None if pm[i] == (1 << 64) - 1 else pm[i] for i in range(k)], cells=list(ce[:k]))


def wfa_plan(match, mismatch, gap_open, gap_extend, lengths, min_score=None):
    """pwa_wfa_plan (host only): the penalties and, for every (n, m) of `lengths`, the sweep bound and the planned wavefront cells ->
    dict(pen=(x, o, e, g), p_max=[...], cells=[...]); p_max is None and cells 0 for a pair the bound already rules out."""
    return _wfa_plan("pwa_wfa_plan", 4, match, mismatch, gap_open, gap_extend, lengths, min_score)


def wfa_sg_plan(match, mismatch, gap_open, gap_extend, lengths, min_score=None):
    """pwa_wfa_sg_plan (host only): wfa_plan for the semi-global form -> dict(pen=(x, o, eI, eD, g), p_max=[...], cells=[...])."""
    return _wfa_plan("pwa_wfa_sg_plan", 5, match, mismatch, gap_open, gap_extend, lengths, min_score)


def _anchor_arrays(anchors):
    """anchors per read ((t, q, len) triples: lists of tuples, or arrays of shape (n, 3)) -> the uint32 arrays t, q, len and the uint64
    offsets of the chain calls, C-contiguous"""
    import numpy as np
    per = [np.asarray(a, dtype=np.int64).reshape(-1, 3) for a in anchors]
    off = np.zeros(len(per) + 1, dtype=np.uint64)
    if per:
        off[1:] = np.cumsum([len(a) for a in per])
    flat = np.concatenate(per) if per else np.zeros((0, 3), dtype=np.int64)
    if flat.size and (flat.min() < 0 or flat.max() > 0xffffffff):
        raise ValueError("anchors: t, q and len are uint32 values")
    cols = [np.ascontiguousarray(flat[:, c], dtype=np.uint32) for c in range(3)]
    cols = [c if c.size else np.zeros(1, dtype=np.uint32) for c in cols]
    return cols[0], cols[1], cols[2], off


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def chain_plan(anchors, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38, budget=0):
    """pwa_chain_plan (host only): what Context.chain would answer to these anchors and parameters before any device work ->
    dict(code, bad_read, ranges): the validation code (0, or a negative PWA_E_* value), the first offending read (None: none, or a
    parameter was at fault), the ranges of reads the call would run under `budget` bytes (0: no limit)."""
    L = lib()
    t, q, ln, off = _anchor_arrays(anchors)
    bad, nr = C.c_uint32(0), C.c_uint64(0)
    rc = L.pwa_chain_plan(_u32p(t), _u32p(q), _u32p(ln), off.ctypes.data_as(C.POINTER(C.c_uint64)), len(off) - 1, lookback, max_dist, bandwidth,
                          gap_scale, budget, C.byref(bad), C.byref(nr))
    return dict(code=rc, bad_read=None if bad.value == CHAIN_NO_READ else bad.value, ranges=nr.value)


def chain_top_plan(anchors, max_chains=4, min_score=40, min_count=3, rooted=False, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38, budget=0,
                   flags=None):
    """pwa_chain_top_plan (host only): chain_plan for Context.chain_top, with that call's parameters and device bytes ->
    dict(code, bad_read, ranges).  flags, where given, is passed as it is in place of rooted."""
    L = lib()
    t, q, ln, off = _anchor_arrays(anchors)
    bad, nr = C.c_uint32(0), C.c_uint64(0)
    rc = L.pwa_chain_top_plan(_u32p(t), _u32p(q), _u32p(ln), off.ctypes.data_as(C.POINTER(C.c_uint64)), len(off) - 1, lookback, max_dist, bandwidth,
                              gap_scale, max_chains, min_score, min_count, (CHAIN_ROOTED if rooted else 0) if flags is None else flags, budget,
                              C.byref(bad), C.byref(nr))
    return dict(code=rc, bad_read=None if bad.value == CHAIN_NO_READ else bad.value, ranges=nr.value)


def mapq(s1, s2, c1):
    """pwa_mapq (host only): the mapping quality 0 .. 60 of a best chain of score s1 and c1 anchors beside a second-best score s2."""
    return lib().pwa_mapq(s1, s2, c1)


def seed_plan(text_len, read_lens, k, step=1, max_occ=64, budget=0):
    """pwa_seed_plan (host only): what TextIndex.seed would answer to reads of these lengths on a text of text_len bytes before any
    device work -> dict(code, bad_read, slots, ranges): the validation code (0, or a negative PWA_E_* value), the first offending
    read (None: none, or a parameter or the total was at fault), the list's slots, the ranges of reads the call would run under a
    budget of `budget` worst-case hits (0: the library's)."""
    import numpy as np
    L = lib()
    off = np.zeros(len(read_lens) + 1, dtype=np.uint64)
    if len(read_lens):
        off[1:] = np.cumsum(np.asarray(read_lens, dtype=np.uint64), dtype=np.uint64)
    bad, ns, nr = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.pwa_seed_plan(text_len, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(read_lens), k, step, max_occ, budget, C.byref(bad), C.byref(ns),
                         C.byref(nr))
    return dict(code=rc, bad_read=None if bad.value == CHAIN_NO_READ else bad.value, slots=ns.value, ranges=nr.value)


def minimizer_plan(n_min, read_lens, k, max_occ=64, budget=0):
    """pwa_mm_plan (host only): seed_plan for a MinimizerIndex of n_min entries -- what MinimizerIndex.seed would answer to reads of
    these lengths before any device work -> dict(code, bad_read, slots, ranges), slots being the list's k-mers."""
    import numpy as np
    L = lib()
    off = np.zeros(len(read_lens) + 1, dtype=np.uint64)
    if len(read_lens):
        off[1:] = np.cumsum(np.asarray(read_lens, dtype=np.uint64), dtype=np.uint64)
    bad, ns, nr = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.pwa_mm_plan(n_min, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(read_lens), k, max_occ, budget, C.byref(bad), C.byref(ns), C.byref(nr))
    return dict(code=rc, bad_read=None if bad.value == CHAIN_NO_READ else bad.value, slots=ns.value, ranges=nr.value)


_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(seq):
    """The reverse complement of a sequence: A <-> T and C <-> G in either case, every other byte unchanged."""
    return _b(seq).translate(_COMPLEMENT)[::-1]


def approx_minima(hits, pat_len, k, n):
    """pwa_approx_minima (host only): per pattern, the locally minimal ends of its COMPLETE hit list [(end, dist)] (find_approx's, for
    a text of n and the bound k: one int, or one per pattern) -> per pattern [(end, dist)], the leftmost end of every plateau that
    is entered by a descent and left by a rise."""
    L = lib()
    n_pat = len(hits)
    ks = [k] * n_pat if isinstance(k, int) else list(k)
    if len(ks) != n_pat or len(pat_len) != n_pat:
        raise ValueError("one pattern length and one k (or one int) per hit list")
    pl = (C.c_uint32 * max(n_pat, 1))(*pat_len)
    md = (C.c_uint32 * max(n_pat, 1))(*ks)
    occ_off, occ = _pack_hits(hits)
    rc = L.pwa_approx_minima(n, pl, md, n_pat, occ_off, occ)
    if rc != 0:
        raise PwaError("pwa_approx_minima: %s" % L.pwa_strerror(rc).decode())
    return [[(occ[x] >> 32, occ[x] & 0xffffffff) for x in range(occ_off[q], occ_off[q + 1])] for q in range(n_pat)]


def _pack_hits(hits):
    """per-pattern [(end, dist)] -> (occ_off, occ) as pwa_approx_occurrences writes them"""
    n_pat = len(hits)
    occ_off = (C.c_uint64 * (n_pat + 1))()
    for q, h in enumerate(hits):
        occ_off[q + 1] = occ_off[q] + len(h)
    total = occ_off[n_pat]
    occ = (C.c_uint64 * max(total, 1))(*[e << 32 | d for h in hits for e, d in h])
    return occ_off, occ


_hw1 = None


def hw1_host():
    """libhw1_host.so: hw1's readSequences and DOT writer (host code only; loads without a GPU)."""
    global _hw1
    if _hw1 is None:
        H = C.CDLL(HW1_HOST_PATH)
        vp, u32p, u64p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        H.hw1_read_sequences.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        H.hw1_read_sequences.restype = vp
        H.hw1_records_count.argtypes = [vp]
        H.hw1_records_count.restype = C.c_uint32
        for f in (H.hw1_records_header, H.hw1_records_sequence):
            f.argtypes = [vp, C.c_uint32, u64p]
            f.restype = vp
        H.hw1_records_free.argtypes = [vp]
        H.hw1_records_free.restype = None
        H.hw1_terminator.argtypes = [C.c_uint32, C.c_uint32]
        H.hw1_write_dot.argtypes = [C.c_char_p, vp, C.c_uint32, u32p, C.c_uint32, u32p, C.POINTER(C.c_char_p), u64p]
        _hw1 = H
    return _hw1


def hw1_read_sequences(path):
    """readSequences of the hw1 reference -> (list of (header bytes, sequence bytes), opened)"""
    H = hw1_host()
    ok = C.c_int(0)
    h = H.hw1_read_sequences(os.fsencode(path), C.byref(ok))
    try:
        out = []
        for i in range(H.hw1_records_count(h)):
            rec = []
            for f in (H.hw1_records_header, H.hw1_records_sequence):
                n = C.c_uint64(0)
                p = f(h, i, C.byref(n))
                rec.append(C.string_at(p, n.value) if n.value else b"")
            out.append(tuple(rec))
        return out, bool(ok.value)
    finally:
        H.hw1_records_free(h)


def hw1_text(refs):
    """(T, ref_start, headers) of hw1: each reference's sequence followed by its terminator"""
    H = hw1_host()
    text, starts = bytearray(), []
    for i, (_, seq) in enumerate(refs):
        starts.append(len(text))
        text += seq + bytes([H.hw1_terminator(len(refs), i)])
    starts.append(len(text))
    return bytes(text), starts, [h for h, _ in refs]


def hw1_write_dot(path, text, sa, ref_start, headers):
    H = hw1_host()
    n_ref = len(headers)
    sa_a = (C.c_uint32 * max(len(sa), 1))(*sa)
    rs = (C.c_uint32 * len(ref_start))(*ref_start)
    hp = (C.c_char_p * max(n_ref, 1))(*headers)
    hl = (C.c_uint64 * max(n_ref, 1))(*[len(h) for h in headers])
    return H.hw1_write_dot(os.fsencode(path), text, len(text), sa_a, n_ref, rs, hp, hl)


_lib = None


def lib():
    """Load libpwalign.so (built in-tree by __graft_entry__.build() / csrc/Makefile). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PwaError("libpwalign.so is not built (%s); run `make -C bioinformatics-algorithms_amd/csrc`: "
                       "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p, i32p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    L.pwa_version.restype = C.c_char_p
    L.pwa_strerror.restype = C.c_char_p
    L.pwa_strerror.argtypes = [C.c_int]
    L.pwa_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.pwa_ctx_destroy.argtypes = [vp]
    L.pwa_ctx_destroy.restype = None
    L.pwa_last_error.argtypes = [vp]
    L.pwa_last_error.restype = C.c_char_p
    L.pwa_ctx_set_score_band.argtypes = [vp, C.c_int]
    L.pwa_ctx_poison_stats.argtypes = [vp, u64p, u64p]
    batch_in = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, u64p, C.c_uint32, u32p, u32p, C.c_uint64]
    L.pwa_scores.argtypes = batch_in + [i32p, u32p, u32p]
    L.pwa_batch_create.argtypes = batch_in + [C.c_int, C.POINTER(vp)]
    affine_in = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, u64p, C.c_uint32, u32p, u32p, C.c_uint64]
    L.pwa_affine_batch_create.argtypes = affine_in + [C.POINTER(vp)]
    L.pwa_scores_affine.argtypes = affine_in + [i32p]
    L.pwa_nwdist_batch_create.argtypes = batch_in[:1] + batch_in[2:] + [C.POINTER(vp)]
    L.pwa_distances.argtypes = batch_in[:1] + batch_in[2:] + [i32p]
    L.pwa_upgma_newick.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_char_p), C.c_uint32, vp, C.c_uint64, u64p]
    L.pwa_batch_run.argtypes = [vp, vp]
    L.pwa_batch_d_scores.argtypes = [vp]
    L.pwa_batch_d_scores.restype = vp
    L.pwa_batch_set_d_scores.argtypes = [vp, vp]
    L.pwa_batch_fetch.argtypes = [vp, i32p, u32p, u32p]
    L.pwa_batch_info.argtypes = [vp, u64p, u64p, u64p, C.POINTER(C.c_char_p)]
    L.pwa_batch_cell_bits.argtypes = [vp]
    L.pwa_batch_profile_form.argtypes = [vp]
    L.pwa_batch_profile_int.argtypes = [vp]
    L.pwa_profile_plan.argtypes = [C.c_uint32, C.c_uint32, u32p, u32p]
    L.pwa_strip_table.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), u32p, u32p]
    L.pwa_pair_form_table.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u32p]
    L.pwa_pair_forms.argtypes = [vp, vp, C.c_uint64, u64p]
    L.pwa_pair_forms_reset.argtypes = [vp]
    L.pwa_batch_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.pwa_batch_run_times.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.pwa_batch_destroy.argtypes = [vp]
    L.pwa_batch_destroy.restype = None
    L.pwa_align.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint64, vp, C.c_uint64, i32p, vp,
                            C.c_uint64, u64p, u64p, u64p]
    L.pwa_align_matrices.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint64, vp, C.c_uint64, vp, vp]
    L.pwa_align_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p]
    L.pwa_align_affine_last_stats.argtypes = [vp, u64p, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p]
    L.pwa_align_batch.argtypes = batch_in + [i32p, vp, u64p, u64p, u64p, u64p]
    L.pwa_align_batch_cigar.argtypes = batch_in + [i32p, vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, u64p, u64p, u64p]
    L.pwa_overlaps.argtypes = batch_in + [i32p, i32p]
    gotoh_in = batch_in[:5] + [C.c_int] + batch_in[5:]   # ctx, mode, match, mismatch, gap_open, gap_extend, sequences, pairs
    L.pwa_align_gotoh_batch.argtypes = gotoh_in + [i32p, vp, u64p, u64p, u64p, u64p]
    L.pwa_align_gotoh_batch_cigar.argtypes = gotoh_in + [i32p, vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, u64p, u64p, u64p]
    L.pwa_align_gotoh_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p]
    L.pwa_align_banded_batch.argtypes = L.pwa_align_gotoh_batch.argtypes + [i32p, i32p]   # ..., band_lo, band_hi
    L.pwa_align_banded_batch_cigar.argtypes = L.pwa_align_gotoh_batch_cigar.argtypes + [i32p, i32p]
    L.pwa_align_banded_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p]
    L.pwa_gotoh_batch_create.argtypes = gotoh_in + [C.c_int, C.POINTER(vp)]
    L.pwa_scores_gotoh.argtypes = gotoh_in + [i32p, u32p, u32p]
    L.pwa_scores_banded.argtypes = gotoh_in + [i32p, u32p, u32p, i32p, i32p]   # ..., score, end_i, end_j, band_lo, band_hi
    L.pwa_scores_banded_last_stats.argtypes = [vp, C.POINTER(C.c_float), u64p]
    ext_in = [vp] + gotoh_in[2:6] + [C.c_int] + gotoh_in[6:]   # ctx, match, mismatch, gap_open, gap_extend, xdrop, sequences, pairs
    L.pwa_extend_banded_batch.argtypes = ext_in + [i32p, vp, u64p, u64p, u64p, u32p, i32p, i32p]   # ..., end_cells, rows, band_lo, band_hi
    L.pwa_extend_banded_batch_cigar.argtypes = ext_in + [i32p, vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, u64p, u32p, u64p, i32p, i32p]
    L.pwa_scores_extend_banded.argtypes = ext_in + [i32p, u32p, u32p, u32p, i32p, i32p]   # ..., score, end_i, end_j, rows, band_lo, band_hi
    L.pwa_extend_banded_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p]
    subst_in = batch_in[:2] + [vp, C.c_int, i32p] + gotoh_in[4:]   # ctx, mode, code[256], n_sym, submat, gap_open, gap_extend, sequences, pairs
    L.pwa_align_subst_batch.argtypes = subst_in + [i32p, vp, u64p, u64p, u64p, u64p]
    L.pwa_align_subst_batch_cigar.argtypes = subst_in + [i32p, vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, u64p, u64p, u64p]
    L.pwa_align_subst_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p]
    L.pwa_subst_batch_create.argtypes = subst_in + [C.c_int, C.POINTER(vp)]
    L.pwa_scores_subst.argtypes = subst_in + [i32p, u32p, u32p]
    L.pwa_align_banded_subst_batch.argtypes = L.pwa_align_subst_batch.argtypes + [i32p, i32p]   # ..., band_lo, band_hi
    L.pwa_align_banded_subst_batch_cigar.argtypes = L.pwa_align_subst_batch_cigar.argtypes + [i32p, i32p]
    L.pwa_scores_banded_subst.argtypes = subst_in + [i32p, u32p, u32p, i32p, i32p]   # ..., score, end_i, end_j, band_lo, band_hi
    ext_subst_in = [vp] + subst_in[2:7] + [C.c_int] + subst_in[7:]   # ctx, code[256], n_sym, submat, gap_open, gap_extend, xdrop, sequences, pairs
    # ..., end_cells, rows, pend_score, pend_j, band_lo, band_hi
    L.pwa_extend_banded_subst_batch.argtypes = ext_subst_in + [i32p, vp, u64p, u64p, u64p, u32p, i32p, u32p, i32p, i32p]
    L.pwa_extend_banded_subst_batch_cigar.argtypes = ext_subst_in + [i32p, vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, u64p, u32p, i32p, u32p, u64p, i32p, i32p]
    L.pwa_scores_extend_banded_subst.argtypes = ext_subst_in + [i32p, u32p, u32p, u32p, i32p, u32p, i32p, i32p]   # ..., score, end_i, end_j, rows, pend_score, pend_j, band_lo, band_hi
    L.pwa_align_affine_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, u64p, C.c_uint32, u32p, u32p, C.c_uint64,
                                         i32p, vp, u64p, u64p]
    L.pwa_cigar_bound.argtypes = [C.c_uint64]
    L.pwa_cigar_bound.restype = C.c_uint64
    L.pwa_mdz_bound.argtypes = [C.c_uint64]
    L.pwa_mdz_bound.restype = C.c_uint64
    L.pwa_alignment_overlap.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, u64p, i32p]
    L.pwa_format_alignment.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, u64p, vp, vp, vp, vp, i32p]
    L.pwa_fasta_read.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_int)]
    L.pwa_fasta_n_seq.argtypes = [vp]
    L.pwa_fasta_n_seq.restype = C.c_uint32
    L.pwa_fasta_bytes.argtypes = [vp]
    L.pwa_fasta_bytes.restype = vp
    L.pwa_fasta_offsets.argtypes = [vp]
    L.pwa_fasta_offsets.restype = u64p
    L.pwa_fasta_first_seq.argtypes = [vp]
    L.pwa_fasta_first_seq.restype = u32p
    L.pwa_fasta_free.argtypes = [vp]
    L.pwa_fasta_free.restype = None
    L.pwa_sa_create.argtypes = [vp, vp, C.c_uint64, C.POINTER(vp)]
    L.pwa_sa_fetch.argtypes = [vp, u32p]
    L.pwa_sa_find.argtypes = [vp, vp, u64p, C.c_uint32, u32p]
    L.pwa_sa_occurrences.argtypes = [vp, vp, u64p, C.c_uint32, u32p, C.c_uint32, u32p, u64p, u64p, C.c_uint64, u64p]
    L.pwa_sa_last_stats.argtypes = [vp, u32p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pwa_sa_destroy.argtypes = [vp]
    L.pwa_sa_destroy.restype = None
    L.pwa_seed_plan.argtypes = [C.c_uint64, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u64p, u64p]
    L.pwa_sa_seed.argtypes = [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p]
    L.pwa_sa_seed_fetch.argtypes = [vp, u32p, u32p, C.c_uint64]
    L.pwa_sa_seed_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p, u64p, u64p]
    f32p = C.POINTER(C.c_float)
    L.pwa_mm_create.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.pwa_mm_destroy.argtypes = [vp]
    L.pwa_mm_destroy.restype = None
    L.pwa_mm_fetch.argtypes = [vp, u64p, u32p, C.c_uint64]
    L.pwa_mm_last_stats.argtypes = [vp, u64p, f32p]
    L.pwa_mm_sketch.argtypes = [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u32p, u64p, C.c_uint64, u64p]
    L.pwa_mm_plan.argtypes = [C.c_uint64, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u64p, u64p]
    L.pwa_mm_seed.argtypes = [vp, vp, u64p, C.c_uint32, C.c_uint32, u64p]
    L.pwa_mm_seed_fetch.argtypes = [vp, u32p, u32p, C.c_uint64]
    L.pwa_mm_seed_last_stats.argtypes = [vp, f32p, f32p, f32p, u64p, u64p, u64p, u64p]
    u8p = C.POINTER(C.c_uint8)
    L.pwa_mm_create_canonical.argtypes = L.pwa_mm_create.argtypes
    L.pwa_mm_fetch_canonical.argtypes = [vp, u64p, u32p, u8p, C.c_uint64]
    L.pwa_mm_sketch_canonical.argtypes = [vp, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u32p, u64p, u8p, C.c_uint64, u64p]
    L.pwa_mm_seed_strands.argtypes = L.pwa_mm_seed.argtypes
    L.pwa_approx_find.argtypes = [vp, vp, C.c_uint64, vp, u64p, C.c_uint32, u32p, u32p, i32p, u32p]
    L.pwa_approx_occurrences.argtypes = [vp, vp, C.c_uint64, vp, u64p, C.c_uint32, u32p, u64p, u64p, C.c_uint64, u64p]
    L.pwa_approx_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p, u64p]
    L.pwa_approx_plan.argtypes = [C.c_uint64, u32p, u32p, C.c_uint32, C.c_uint32, u32p, u64p, u64p, u64p, C.c_uint64, u64p]
    L.pwa_approx_starts.argtypes = [vp, vp, C.c_uint64, vp, u64p, C.c_uint32, u64p, u64p, u32p]
    L.pwa_approx_starts_last_stats.argtypes = [vp, C.POINTER(C.c_float), u64p, u64p]
    L.pwa_approx_minima.argtypes = [C.c_uint64, u32p, u32p, C.c_uint32, u64p, u64p]
    wfa_in = [vp] + gotoh_in[2:]   # ctx, match, mismatch, gap_open, gap_extend, sequences, pairs
    L.pwa_wfa_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u64p, u64p, i32p, C.c_uint64, i32p, u64p, u64p]
    L.pwa_scores_wfa.argtypes = wfa_in + [i32p, i32p, u32p]   # ..., min_score, score, penalty
    L.pwa_align_wfa_batch.argtypes = wfa_in + [i32p, vp, u64p, u64p, i32p]   # ..., score, ops, ops_off, n_ops, min_score
    L.pwa_align_wfa_batch_cigar.argtypes = wfa_in + [i32p, vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, u64p, i32p]
    L.pwa_align_wfa_codes_batch.argtypes = L.pwa_align_wfa_batch.argtypes
    L.pwa_align_wfa_codes_batch_cigar.argtypes = L.pwa_align_wfa_batch_cigar.argtypes
    L.pwa_wfa_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p, u64p]
    L.pwa_wfa_sg_plan.argtypes = L.pwa_wfa_plan.argtypes
    L.pwa_scores_wfa_sg.argtypes = wfa_in + [i32p, i32p, u32p, u64p]   # ..., min_score, score, penalty, end_j
    L.pwa_align_wfa_sg_batch.argtypes = wfa_in + [i32p, vp, u64p, u64p, u64p, u64p, i32p]   # ..., score, ops, ops_off, n_ops, end, start, min_score
    L.pwa_align_wfa_sg_batch_cigar.argtypes = wfa_in + [i32p, vp, C.c_uint64, u64p, vp, C.c_uint64, u64p, u64p, u64p, u64p, i32p]
    chain_in = [u32p, u32p, u32p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]   # anchors, offsets, reads, the four parameters
    L.pwa_chain_plan.argtypes = chain_in + [C.c_uint64, u32p, u64p]
    L.pwa_chain_anchors.argtypes = [vp] + chain_in + [i32p, u32p, u32p, u32p, i32p, i32p, i32p]
    L.pwa_chain_last_stats.argtypes = [vp, C.POINTER(C.c_float), u64p, u64p]
    top_in = chain_in + [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]   # ..., max_chains, min_score, min_count, flags
    L.pwa_chain_top_plan.argtypes = top_in + [C.c_uint64, u32p, u64p]
    L.pwa_chain_top.argtypes = [vp] + top_in + [u32p, i32p, u32p, u32p, u32p, i32p, i32p, u32p, i32p, i32p, i32p]
    L.pwa_chain_top_last_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u64p, u64p, u64p]
    L.pwa_mapq.argtypes = [C.c_int32, C.c_int32, C.c_uint32]
    _lib = L
    return L


STRIP_VARIANTS = ("single", "lanes", "lanes_single", "cell16", "cell16_single", "prof16", "prof16_int")   # PWA_STRIP_* bits 0..6


def strip_table():
    """pwa_strip_table (host only): the instantiated register-strip kernels as dicts -- name (the entry's part of info()["kernel"]), R, mode
    and score (pwalign.h's numbers), variants (the STRIP_VARIANTS the entry carries beside its multi-strip kernel)."""
    L = lib()
    count = C.c_uint32(0)
    L.pwa_strip_table(0xffffffff, None, None, None, None, None, C.byref(count))
    out = []
    for i in range(count.value):
        name, rows, mode, score, var = C.c_char_p(), C.c_int(0), C.c_int(0), C.c_int(0), C.c_uint32(0)
        rc = L.pwa_strip_table(i, C.byref(name), C.byref(rows), C.byref(mode), C.byref(score), C.byref(var), None)
        if rc != 0:
            raise PwaError("pwa_strip_table: %s" % L.pwa_strerror(rc).decode())
        out.append(dict(name=name.value.decode(), R=rows.value, mode=mode.value, score=score.value,
                        variants=tuple(v for k, v in enumerate(STRIP_VARIANTS) if var.value >> k & 1)))
    return out


def pair_form_table():
    """pwa_pair_form_table (host only): the names of the pair-engine forms the library's call sites can build, in the listing's order."""
    L = lib()
    count = C.c_uint32(0)
    L.pwa_pair_form_table(0xffffffff, None, C.byref(count))
    out = []
    for i in range(count.value):
        name = C.c_char_p()
        rc = L.pwa_pair_form_table(i, C.byref(name), None)
        if rc != 0:
            raise PwaError("pwa_pair_form_table: %s" % L.pwa_strerror(rc).decode())
        out.append(name.value.decode())
    return out


def _b(x):
    return bytes(x) if isinstance(x, (bytes, bytearray, memoryview)) else x.encode("latin-1")


def pack_sequences(seqs):
    """list of bytes -> (concatenated bytes, uint64 offsets[n+1], the list); an already packed triple passes through"""
    if (isinstance(seqs, tuple) and len(seqs) == 3 and isinstance(seqs[0], (bytes, bytearray)) and isinstance(seqs[1], C.Array)
            and getattr(seqs[1], "_type_", None) is C.c_uint64 and isinstance(seqs[2], list)):   # (a tuple of three byte strings is a list of sequences)
        return seqs
    seqs = [_b(s) for s in seqs]
    off = (C.c_uint64 * (len(seqs) + 1))()
    tot = 0
    for i, s in enumerate(seqs):
        off[i] = tot
        tot += len(s)
    off[len(seqs)] = tot
    return b"".join(seqs), off, seqs


EXT_NO_PEND = -(1 << 31)   # PWA_EXT_NO_PEND: pend_score_out of a pair whose row n was not reached or not kept


def _pend(score, j):
    """a pair's pattern-end result as the Python calls return it: (score, j), or None where there is none"""
    return None if score == EXT_NO_PEND else (score, j)


_SUBST_NO_CODE = 255   # subst_table(unknown=None): a byte outside the alphabet (no code is that large: n_sym <= 32)


def subst_table(alphabet, matrix, unknown=None, fold_case=False):
    """The scoring of the align_subst_* / scores_subst* calls: symbol k of `alphabet` (bytes or str, at most 32 distinct symbols) gets
    code k, and matrix[a][b] (any nested sequence or array of len(alphabet) x len(alphabet) integers, possibly asymmetric) scores
    pattern symbol a against text symbol b.  Bytes outside the alphabet score as alphabet[unknown] (an index: a wildcard row and column
    the caller put into the matrix); with unknown=None a call whose sequences hold such a byte raises PwaError.  fold_case also maps
    the other case of every letter of the alphabet to the letter's code.  -> (code, n_sym, submat): a 256-entry uint8 map and the flat
    int32 matrix, row = pattern code."""
    import numpy as np
    alpha = _b(alphabet)
    n_sym = len(alpha)
    if not 1 <= n_sym <= 32 or len(set(alpha)) != n_sym:
        raise ValueError("subst_table: an alphabet of 1..32 distinct symbols")
    m = np.asarray(matrix)
    if m.shape != (n_sym, n_sym) or m.dtype.kind not in "iu" or np.abs(m.astype(np.int64)).max() > 0x7fffffff:
        raise ValueError("subst_table: matrix must be %d x %d integers that fit int32" % (n_sym, n_sym))
    if unknown is not None and not 0 <= unknown < n_sym:
        raise ValueError("subst_table: unknown must be an index into the alphabet")
    code = np.full(256, _SUBST_NO_CODE if unknown is None else unknown, dtype=np.uint8)
    if fold_case:
        for k, v in enumerate(alpha):
            other = bytes([v]).swapcase()[0]
            if other not in alpha:
                code[other] = k
    for k, v in enumerate(alpha):
        code[v] = k
    return code, n_sym, np.ascontiguousarray(m, dtype=np.int32).reshape(-1)


def _subst_args(table, blob):
    """(code, n_sym, submat) as the C ABI takes them; raises when the sequences hold a byte that subst_table left without a code"""
    import numpy as np
    code, n_sym, submat = table
    code = np.ascontiguousarray(code, dtype=np.uint8)
    submat = np.ascontiguousarray(submat, dtype=np.int32)
    if code.shape != (256,) or submat.shape != (n_sym * n_sym,):
        raise ValueError("a substitution table is (code[256], n_sym, submat[n_sym * n_sym]), as subst_table returns it")
    if n_sym <= _SUBST_NO_CODE and (code == _SUBST_NO_CODE).any():
        seen = np.bincount(np.frombuffer(blob, dtype=np.uint8), minlength=256) > 0
        bad = np.flatnonzero(seen & (code == _SUBST_NO_CODE))
        if bad.size:
            raise PwaError("substitution table: byte 0x%02x of the sequences is outside the alphabet and no `unknown` code was given" % bad[0])
        code = np.where(code == _SUBST_NO_CODE, 0, code).astype(np.uint8)   # (bytes that do not occur: any valid code)
    return code, int(n_sym), submat, code.ctypes.data_as(C.c_void_p), submat.ctypes.data_as(C.POINTER(C.c_int32))


def band_around(n, m, w, diag=None):
    """(lo, hi) for align_banded_batch.  diag=None: the global band of an n x m pair, half-width w around the corner-to-corner
    diagonals (valid for nw); diag=d: a read seeded on text diagonal d (j - i = d), for sg / sw."""
    if diag is None:
        return (min(0, m - n) - w, max(0, m - n) + w)
    return (diag - w, diag + w)


def read_fasta(paths, n_threads=0):
    """readFasta (hw2.cpp:25-57) over one or more files -> (blob, offsets, first_seq): sequence k is
    blob[offsets[k]:offsets[k + 1]], the sequences of paths[i] are first_seq[i] .. first_seq[i + 1] - 1."""
    L = lib()
    if isinstance(paths, (str, bytes)):
        paths = [paths]
    arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
    h, bad = C.c_void_p(), C.c_int(-1)
    rc = L.pwa_fasta_read(arr, len(paths), n_threads, C.byref(h), C.byref(bad))
    if rc != 0:
        raise PwaError("pwa_fasta_read: %s (%s)" % (L.pwa_strerror(rc).decode(), paths[bad.value] if bad.value >= 0 else "-"))
    try:
        n = L.pwa_fasta_n_seq(h)
        off = list(L.pwa_fasta_offsets(h)[:n + 1])
        first = list(L.pwa_fasta_first_seq(h)[:len(paths) + 1])
        blob = C.string_at(L.pwa_fasta_bytes(h), off[n]) if off[n] else b""
    finally:
        L.pwa_fasta_free(h)
    return blob, off, first


def alignment_overlap(pattern, text, ops, end):
    """overlapLongestExactMatch (hw2.cpp:267-278) from the op list alone."""
    L = lib()
    pattern, text, ops = _b(pattern), _b(text), _b(ops)
    ov = C.c_int32(0)
    endc = (C.c_uint64 * 2)(end[0], end[1])
    rc = L.pwa_alignment_overlap(pattern, len(pattern), text, len(text), ops, len(ops), endc, C.byref(ov))
    if rc != 0:
        raise PwaError("pwa_alignment_overlap: %s" % L.pwa_strerror(rc).decode())
    return ov.value


def format_alignment(pattern, text, ops, end):
    """Host post-processing (hw2.cpp:59-116, 164-184, 267-278) through the C ABI."""
    L = lib()
    pattern, text, ops = _b(pattern), _b(text), _b(ops)
    n_ops = len(ops)
    ap = C.create_string_buffer(n_ops + 1)
    ar = C.create_string_buffer(n_ops + 1)
    cg = C.create_string_buffer(L.pwa_cigar_bound(n_ops))
    md = C.create_string_buffer(L.pwa_mdz_bound(n_ops))
    ov = C.c_int32(0)
    endc = (C.c_uint64 * 2)(end[0], end[1])
    rc = L.pwa_format_alignment(pattern, len(pattern), text, len(text), ops, n_ops, endc, ap, ar, cg, md, C.byref(ov))
    if rc != 0:
        raise PwaError("pwa_format_alignment: %s" % L.pwa_strerror(rc).decode())
    return dict(aligned_pattern=ap.raw[:n_ops], aligned_reference=ar.raw[:n_ops], cigar=cg.value, mdz=md.value,
                overlap=ov.value)


def upgma_newick(dist_rows, names):
    """Host UPGMA + Newick (hw4.cpp:162-228) through the C ABI."""
    L = lib()
    n = len(names)
    flat = (C.c_double * max(n * n, 1))(*[float(x) for row in dist_rows for x in row])
    arr = (C.c_char_p * max(n, 1))(*[_b(x) for x in names])
    need = C.c_uint64(0)
    L.pwa_upgma_newick(flat, arr, n, None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value + 1)
    rc = L.pwa_upgma_newick(flat, arr, n, buf, need.value + 1, C.byref(need))
    if rc != 0:
        raise PwaError("pwa_upgma_newick: %s" % L.pwa_strerror(rc).decode())
    return buf.value


class Context:
    """One MI355X (HIP device ordinal)."""

    def __init__(self, device=0):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.pwa_ctx_create(device, C.byref(h))
        if rc != 0:
            raise PwaError("pwa_ctx_create(%d): %s -- the HIP path is required, there is no CPU fallback"
                           % (device, self._L.pwa_strerror(rc).decode()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.pwa_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_score_band(self, on):
        self._check(self._L.pwa_ctx_set_score_band(self._h, 1 if on else 0), "pwa_ctx_set_score_band")

    def pair_forms(self):
        """pwa_pair_forms: the names (pair_form_table's) of the pair-engine forms this context has prepared launches of since the last
        reset_pair_forms(), distinct, in first-seen order."""
        need = C.c_uint64(0)
        rc = self._L.pwa_pair_forms(self._h, None, 0, C.byref(need))
        if rc != -5:
            self._check(rc, "pwa_pair_forms")
        buf = C.create_string_buffer(need.value)
        self._check(self._L.pwa_pair_forms(self._h, buf, need.value, C.byref(need)), "pwa_pair_forms")
        return buf.value.decode().split("\n") if buf.value else []

    def reset_pair_forms(self):
        self._check(self._L.pwa_pair_forms_reset(self._h), "pwa_pair_forms_reset")

    def poison_stats(self):
        """pwa_ctx_poison_stats: what PWA_POISON has filled on this context so far -> dict(buffers, bytes); zeros with the switch unset."""
        n, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pwa_ctx_poison_stats(self._h, C.byref(n), C.byref(b)), "pwa_ctx_poison_stats")
        return dict(buffers=n.value, bytes=b.value)

    def _check(self, rc, what):
        if rc != 0:
            raise PwaError("%s: %s (%s)" % (what, self._L.pwa_strerror(rc).decode(),
                                            self._L.pwa_last_error(self._h).decode()))

    # -- scores-only pass (hw2.cpp:328-338, score field only)
    def scores(self, mode, seqs, pair_a, pair_b, match, mismatch, gap, want_end=False):
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        sc = (C.c_int32 * max(n, 1))()
        ei = (C.c_uint32 * max(n, 1))() if want_end else None
        ej = (C.c_uint32 * max(n, 1))() if want_end else None
        rc = self._L.pwa_scores(self._h, MODE[mode], match, mismatch, gap, blob, off, len(seqs), pa, pb, n, sc, ei, ej)
        self._check(rc, "pwa_scores")
        if want_end:
            return list(sc[:n]), list(ei[:n]), list(ej[:n])
        return list(sc[:n])

    def batch(self, mode, seqs, pair_a, pair_b, match, mismatch, gap, want_end=False):
        return Batch(self, mode, seqs, pair_a, pair_b, match, mismatch, gap, want_end)

    # -- hw3.cpp affine_alignment score pass (hw3.cpp:23-102, all-pairs loop 232-241)
    def scores_affine(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend):
        b = Batch(self, "affine", seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend=gap_extend)
        b.run()
        out = b.fetch()
        b.close()
        return out

    # -- hw4.cpp all-pairs step: NW (tie-break diag >= up >= left) + gap/mismatch column count (16-72, 146-152)
    def distances(self, seqs, pair_a, pair_b, match, mismatch, gap):
        b = Batch(self, "nwdist", seqs, pair_a, pair_b, match, mismatch, gap)
        b.run()
        out = b.fetch()
        b.close()
        return out

    def _oneshot(self, fn, name, seqs, pair_a, pair_b, *scoring):
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        out = (C.c_int32 * max(n, 1))()
        self._check(fn(self._h, *scoring, blob, off, len(seqs), pa, pb, n, out), name)
        return list(out[:n])

    def distances_oneshot(self, seqs, pair_a, pair_b, match, mismatch, gap):
        """pwa_distances: the one-call form (pair lists of any size: cut into arena-sized runs by the library)."""
        return self._oneshot(self._L.pwa_distances, "pwa_distances", seqs, pair_a, pair_b, match, mismatch, gap)

    def scores_affine_oneshot(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend):
        """pwa_scores_affine: the one-call form."""
        return self._oneshot(self._L.pwa_scores_affine, "pwa_scores_affine", seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend)

    # -- affine-gap (gotoh) scores: the semantics of align_gotoh_batch without the alignments (include/pwalign.h)
    def scores_gotoh(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, want_end=False):
        b = Batch(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, want_end, gap_extend=gap_extend, gotoh=True)
        b.run()
        out = b.fetch()
        b.close()
        return out

    def scores_gotoh_oneshot(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, want_end=False):
        """pwa_scores_gotoh: the one-call form (pair lists of any size: cut into arena-sized runs by the library)."""
        return self._scores_call(self._L.pwa_scores_gotoh, "pwa_scores_gotoh", (self._h, MODE[mode], match, mismatch, gap_open, gap_extend),
                                 seqs, pair_a, pair_b, want_end)

    def batch_gotoh(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, want_end=False):
        return Batch(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, want_end, gap_extend=gap_extend, gotoh=True)

    def batch_distances(self, seqs, pair_a, pair_b, match, mismatch, gap):
        return Batch(self, "nwdist", seqs, pair_a, pair_b, match, mismatch, gap)

    def batch_affine(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend):
        return Batch(self, "affine", seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend=gap_extend)

    # -- one full alignment = one call of hw2.cpp:118 / 192
    def align(self, mode, pattern, text, match, mismatch, gap, raw=False):
        pattern, text = _b(pattern), _b(text)
        n, m = len(pattern), len(text)
        ops = C.create_string_buffer(n + m + 1)
        score = C.c_int32(0)
        n_ops = C.c_uint64(0)
        end = (C.c_uint64 * 2)()
        start = (C.c_uint64 * 2)()
        rc = self._L.pwa_align(self._h, MODE[mode], match, mismatch, gap, pattern, n, text, m, C.byref(score), ops,
                               n + m, C.byref(n_ops), end, start)
        self._check(rc, "pwa_align")
        out = dict(score=score.value, ops=ops.raw[:n_ops.value], end=(end[0], end[1]), start=(start[0], start[1]))
        if not raw:
            out.update(format_alignment(pattern, text, out["ops"], out["end"]))
        return out

    def matrices(self, mode, pattern, text, match, mismatch, gap):
        """(dp, traceback) as numpy arrays (n+1, m+1): the reference's two per-pair matrices (hw2.cpp:119-120)."""
        import numpy as np
        pattern, text = _b(pattern), _b(text)
        n, m = len(pattern), len(text)
        dp = np.zeros((n + 1, m + 1), dtype=np.int32)
        tb = np.zeros((n + 1, m + 1), dtype=np.uint8)
        rc = self._L.pwa_align_matrices(self._h, MODE[mode], match, mismatch, gap, pattern, n, text, m,
                                        dp.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p))
        self._check(rc, "pwa_align_matrices")
        return dp, tb

    def align_batch(self, mode, seqs, pair_a, pair_b, match, mismatch, gap, region_pad=0):
        """region_pad > 0: every pair's op region starts at a multiple of region_pad (a caller with aligned regions; the library then
        returns the op lists through its staging copy instead of one tiled copy)."""
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        ooff = (C.c_uint64 * max(n, 1))()
        tot = 0
        for k in range(n):
            if region_pad:
                tot = (tot + region_pad - 1) // region_pad * region_pad + (region_pad if k % 3 == 1 else 0)
            ooff[k] = tot
            tot += len(seqs[pair_a[k]]) + len(seqs[pair_b[k]])
        ops = C.create_string_buffer(tot + 1)
        sc = (C.c_int32 * max(n, 1))()
        nops = (C.c_uint64 * max(n, 1))()
        endc = (C.c_uint64 * (2 * max(n, 1)))()
        startc = (C.c_uint64 * (2 * max(n, 1)))()
        rc = self._L.pwa_align_batch(self._h, MODE[mode], match, mismatch, gap, blob, off, len(seqs), pa, pb, n, sc, ops,
                                     ooff, nops, endc, startc)
        self._check(rc, "pwa_align_batch")
        res = []
        raw = memoryview(ops)   # no per-pair copy of the whole buffer
        for k in range(n):
            o = bytes(raw[ooff[k]:ooff[k] + nops[k]])
            res.append(dict(score=sc[k], ops=o, end=(endc[2 * k], endc[2 * k + 1]),
                            start=(startc[2 * k], startc[2 * k + 1])))
        return res

    def align_batch_cigar(self, mode, seqs, pair_a, pair_b, match, mismatch, gap):
        """pwa_align_batch_cigar: the alignments of align_batch as the reference's CIGAR and MD:Z strings, built on the device ->
        [dict(score, cigar, mdz, end, start)] (cigar / mdz: bytes).  The buffers are sized by pwa_cigar_bound / pwa_mdz_bound of every
        pair, which always fit: one call, no retry."""
        import numpy as np
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        lens = np.array([len(x) for x in seqs] or [0], dtype=np.uint64)
        nm = lens[np.asarray(pair_a, dtype=np.int64)] + lens[np.asarray(pair_b, dtype=np.int64)] if n else np.zeros(0, np.uint64)
        cap_c, cap_m = int((2 * nm + 24).sum()), int((3 * nm + 24).sum())   # pwa_cigar_bound / pwa_mdz_bound (host/postprocess.cpp)
        cg = np.empty(max(cap_c, 1), dtype=np.uint8)
        md = np.empty(max(cap_m, 1), dtype=np.uint8)
        cg_off = np.zeros(n + 1, dtype=np.uint64)
        md_off = np.zeros(n + 1, dtype=np.uint64)
        sc = (C.c_int32 * max(n, 1))()
        endc = (C.c_uint64 * (2 * max(n, 1)))()
        startc = (C.c_uint64 * (2 * max(n, 1)))()
        u64p = C.POINTER(C.c_uint64)
        rc = self._L.pwa_align_batch_cigar(self._h, MODE[mode], match, mismatch, gap, blob, off, len(seqs), pa, pb, n, sc,
                                           cg.ctypes.data_as(C.c_void_p), cap_c, cg_off.ctypes.data_as(u64p),
                                           md.ctypes.data_as(C.c_void_p), cap_m, md_off.ctypes.data_as(u64p), endc, startc, None)
        self._check(rc, "pwa_align_batch_cigar")
        co, mo = cg_off.tolist(), md_off.tolist()
        cgb, mdb = cg[:co[n]].tobytes(), md[:mo[n]].tobytes()
        return [dict(score=sc[k], cigar=cgb[co[k]:co[k + 1]], mdz=mdb[mo[k]:mo[k + 1]], end=(endc[2 * k], endc[2 * k + 1]),
                     start=(startc[2 * k], startc[2 * k + 1])) for k in range(n)]

    def _scores_call(self, fn, name, head, seqs, pair_a, pair_b, want_end, extra=0, pend=False, tail=()):
        """a one-call score pass whose arguments are `head` (context .. scoring), the sequences, the pairs, score_out, end_i_out and
        end_j_out, `extra` more uint32 outputs (an extension call's rows_out), with `pend` pend_score_out and pend_j_out, and `tail`
        -> scores, or with want_end (scores, end_i, end_j, the extra lists ..., the pattern-end list)"""
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        sc = (C.c_int32 * max(n, 1))()
        u32 = [(C.c_uint32 * max(n, 1))() if want_end else None for _ in range(2 + extra)]
        pe = ()
        if pend:
            pe = ((C.c_int32 * max(n, 1))(), (C.c_uint32 * max(n, 1))()) if want_end else (None, None)
        self._check(fn(*head, blob, off, len(seqs), pa, pb, n, sc, *u32, *pe, *tail), name)
        if not want_end:
            return list(sc[:n])
        out = (list(sc[:n]),) + tuple(list(a[:n]) for a in u32)
        return out + ([_pend(pe[0][k], pe[1][k]) for k in range(n)],) if pend else out

    @staticmethod
    def _align_begin(seqs, pair_a, pair_b, ext, pend):
        """what _align_ops and _align_strings start with: the packed sequences, the pair arrays and the outputs both have
        -> blob, off, seqs, n, pa, pb, sc, endc, startc (ext: rows_out in its place), pe (pend: pend_score_out, pend_j_out)"""
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        sc = (C.c_int32 * max(n, 1))()
        endc = (C.c_uint64 * (2 * max(n, 1)))()
        startc = (C.c_uint32 * max(n, 1))() if ext else (C.c_uint64 * (2 * max(n, 1)))()
        pe = ((C.c_int32 * max(n, 1))(), (C.c_uint32 * max(n, 1))()) if pend else ()
        return blob, off, seqs, n, pa, pb, sc, endc, startc, pe

    @staticmethod
    def _pair_lens(seqs, pair_a, pair_b, lax):
        """(n, m) of every pair; lax: 0 for an index outside the list, which is then the library's to refuse (a PwaError, not an IndexError)"""
        ln = (lambda i: len(seqs[i]) if 0 <= i < len(seqs) else 0) if lax else (lambda i: len(seqs[i]))
        return [(ln(a), ln(b)) for a, b in zip(pair_a, pair_b)]

    @staticmethod
    def _align_results(n, own, sc, endc, startc, pe, ext, none=None, ends=None):
        """... and end with: own(k) = the keys of pair k that only the one call has, between score and end; none: the score that stands
        for "no alignment" and is returned as None; ends: the end cells of a call without cell outputs, whose start cells are (0, 0)"""
        if none is not None:
            sc = [None if v == none else v for v in sc[:n]]
        if ends is not None:
            return [dict(score=sc[k], **own(k), end=ends[k], start=(0, 0)) for k in range(n)]
        if not ext:
            return [dict(score=sc[k], **own(k), end=(endc[2 * k], endc[2 * k + 1]), start=(startc[2 * k], startc[2 * k + 1])) for k in range(n)]
        out = [dict(score=sc[k], **own(k), end=(endc[2 * k], endc[2 * k + 1]), start=(0, 0), rows=startc[k]) for k in range(n)]
        for k in range(n if pe else 0):
            out[k]["pend"] = _pend(pe[0][k], pe[1][k])
        return out

    def _align_ops(self, fn, name, head, seqs, pair_a, pair_b, tail=(), ext=False, pend=False, none=None, cells=True, lax=False):
        """an op-list alignment call whose arguments are `head` (context .. scoring), the sequences, the pairs, the outputs (and `tail`);
        ext: an extension call -- rows_out where the others take start_cells, start = (0, 0) and a `rows` key in the result;
        pend: ... with pend_score_out and pend_j_out behind rows_out, and a `pend` key;
        none, cells, lax (the wavefront calls): see _align_results and _pair_lens; cells=False: no end_cells and start_cells, end = (n, m)"""
        blob, off, seqs, n, pa, pb, sc, endc, startc, pe = self._align_begin(seqs, pair_a, pair_b, ext, pend)
        lens = self._pair_lens(seqs, pair_a, pair_b, lax)
        ooff = (C.c_uint64 * max(n, 1))()
        tot = 0
        for k in range(n):
            ooff[k] = tot
            tot += lens[k][0] + lens[k][1]
        ops = C.create_string_buffer(tot + 1)
        nops = (C.c_uint64 * max(n, 1))()
        rc = fn(*head, blob, off, len(seqs), pa, pb, n, sc, ops, ooff, nops, *((endc, startc) if cells else ()), *pe, *tail)
        self._check(rc, name)
        raw = memoryview(ops)
        return self._align_results(n, lambda k: dict(ops=bytes(raw[ooff[k]:ooff[k] + nops[k]])), sc, endc, startc, pe, ext, none, None if cells else lens)

    def _align_strings(self, fn, name, head, seqs, pair_a, pair_b, tail=(), ext=False, pend=False, none=None, cells=True, lax=False):
        """... and one that returns CIGAR and MD:Z strings (built on the device; the wavefront calls' on the host)"""
        import numpy as np
        blob, off, seqs, n, pa, pb, sc, endc, startc, pe = self._align_begin(seqs, pair_a, pair_b, ext, pend)
        lens = self._pair_lens(seqs, pair_a, pair_b, lax)
        nm = np.array([a + b for a, b in lens], dtype=np.uint64)
        cap_c, cap_m = int((2 * nm + 24).sum()), int((3 * nm + 24).sum())   # pwa_cigar_bound / pwa_mdz_bound
        cg = np.empty(max(cap_c, 1), dtype=np.uint8)
        md = np.empty(max(cap_m, 1), dtype=np.uint8)
        cg_off = np.zeros(n + 1, dtype=np.uint64)
        md_off = np.zeros(n + 1, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        rc = fn(*head, blob, off, len(seqs), pa, pb, n, sc, cg.ctypes.data_as(C.c_void_p), cap_c, cg_off.ctypes.data_as(u64p),
                md.ctypes.data_as(C.c_void_p), cap_m, md_off.ctypes.data_as(u64p), *((endc, startc) if cells else ()), *pe, None, *tail)
        self._check(rc, name)
        co, mo = cg_off.tolist(), md_off.tolist()
        cgb, mdb = cg[:co[n]].tobytes(), md[:mo[n]].tobytes()
        return self._align_results(n, lambda k: dict(cigar=cgb[co[k]:co[k + 1]], mdz=mdb[mo[k]:mo[k + 1]]), sc, endc, startc, pe, ext, none,
                                   None if cells else lens)

    def _stats3(self, fn, name, third):
        """a last-stats call of three values: device ms of the fills and of the walks, and a count under the key `third`"""
        f, w, c = C.c_float(0), C.c_float(0), C.c_uint64(0)
        self._check(fn(self._h, C.byref(f), C.byref(w), C.byref(c)), name)
        return {"fill_ms": f.value, "walk_ms": w.value, third: c.value}

    def align_gotoh_batch(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend):
        """pwa_align_gotoh_batch: affine-gap alignments (a gap of length L scores gap_open + L * gap_extend; include/pwalign.h) ->
        [dict(score, ops, end, start)] as align_batch returns them."""
        return self._align_ops(self._L.pwa_align_gotoh_batch, "pwa_align_gotoh_batch",
                               (self._h, MODE[mode], match, mismatch, gap_open, gap_extend), seqs, pair_a, pair_b)

    def align_gotoh_batch_cigar(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend):
        """pwa_align_gotoh_batch_cigar: the alignments of align_gotoh_batch as CIGAR and MD:Z strings built on the device ->
        [dict(score, cigar, mdz, end, start)] as align_batch_cigar returns them."""
        return self._align_strings(self._L.pwa_align_gotoh_batch_cigar, "pwa_align_gotoh_batch_cigar",
                                   (self._h, MODE[mode], match, mismatch, gap_open, gap_extend), seqs, pair_a, pair_b)

    # -- wavefront (WFA) affine-gap global alignments of long pairs: exact, no band (include/pwalign.h, "Wavefront alignments")
    def _wfa_scores(self, name, seqs, pair_a, pair_b, scoring, min_score, end_j=False):
        """a WFA score pass: min_score before score_out and penalty_out, with end_j an end_j_out behind them
        -> scores and penalties (None for a pair not found), the sequences, end_j_out"""
        blob, off, seqs, n, pa, pb, sc, _, _, _ = self._align_begin(seqs, pair_a, pair_b, False, False)
        pen = (C.c_uint32 * max(n, 1))()
        ej = (C.c_uint64 * max(n, 1))() if end_j else None
        self._check(getattr(self._L, name)(self._h, *scoring, blob, off, len(seqs), pa, pb, n, _min_scores(min_score, n), sc, pen, *([ej] if end_j else [])), name)
        scores = [None if sc[k] == WFA_NONE else sc[k] for k in range(n)]
        return scores, [None if scores[k] is None else pen[k] for k in range(n)], seqs, ej

    def scores_wfa(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, min_score=None, want_penalty=False):
        """pwa_scores_wfa: the global affine-gap score of every pair, None for a pair whose optimum lies below min_score (None, one
        int, or one per pair) -> scores, or with want_penalty (scores, penalties)."""
        scores, pens, _, _ = self._wfa_scores("pwa_scores_wfa", seqs, pair_a, pair_b, (match, mismatch, gap_open, gap_extend), min_score)
        return (scores, pens) if want_penalty else scores

    @staticmethod
    def _wfa_form(form, name):
        """the C call of a form of the WFA alignments: "offsets" keeps every wavefront (12 bytes per planned cell), "codes" a ring and
        one code byte per planned cell; the results are the same"""
        if form == "offsets":
            return name
        if form == "codes":
            return name.replace("pwa_align_wfa_", "pwa_align_wfa_codes_")
        raise ValueError('form: "offsets" or "codes", not %r' % (form,))

    def _wfa_align(self, helper, name, cells, seqs, pair_a, pair_b, scoring, min_score):
        """a WFA alignment call through _align_ops or _align_strings: min_score in the tail, PWA_WFA_NONE as None, a pair index outside
        the list left to the library; cells: the call has end and start cells (the semi-global form)"""
        return helper(getattr(self._L, name), name, (self._h,) + scoring, seqs, pair_a, pair_b, tail=(_min_scores(min_score, len(pair_a)),),
                      none=WFA_NONE, cells=cells, lax=True)

    def align_wfa_batch(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, min_score=None, form="offsets"):
        """pwa_align_wfa_batch (form="offsets") or pwa_align_wfa_codes_batch (form="codes") -> [dict(score, ops, end, start)] as
        align_gotoh_batch returns them (end = (n, m), start = (0, 0)); score None and ops b"" for a pair not found."""
        return self._wfa_align(self._align_ops, self._wfa_form(form, "pwa_align_wfa_batch"), False, seqs, pair_a, pair_b,
                               (match, mismatch, gap_open, gap_extend), min_score)

    def align_wfa_batch_cigar(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, min_score=None, form="offsets"):
        """pwa_align_wfa_batch_cigar (form="offsets") or pwa_align_wfa_codes_batch_cigar (form="codes") -> [dict(score, cigar, mdz, end,
        start)] as align_gotoh_batch_cigar returns them; score None and two empty strings for a pair not found."""
        return self._wfa_align(self._align_strings, self._wfa_form(form, "pwa_align_wfa_batch_cigar"), False, seqs, pair_a, pair_b,
                               (match, mismatch, gap_open, gap_extend), min_score)

    # -- the semi-global form: the whole pattern against any substring of the text (include/pwalign.h, "Semi-global wavefront alignments")
    def scores_wfa_sg(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, min_score=None, want_penalty=False, want_end=False):
        """pwa_scores_wfa_sg: the semi-global affine-gap score of every pair (pattern = pair_a, whole; text = pair_b, ends free), None for
        a pair whose optimum lies below min_score (None, one int, or one per pair) -> scores, or a tuple of scores, then with
        want_penalty the penalties (None where not found), then with want_end the end cells (i, j) ((0, 0) where not found)."""
        scores, pens, seqs, ej = self._wfa_scores("pwa_scores_wfa_sg", seqs, pair_a, pair_b, (match, mismatch, gap_open, gap_extend), min_score, end_j=True)
        out = [scores]
        if want_penalty:
            out.append(pens)
        if want_end:
            out.append([(0, 0) if s is None else (len(seqs[pair_a[k]]), ej[k]) for k, s in enumerate(scores)])
        return scores if len(out) == 1 else tuple(out)

    def align_wfa_sg_batch(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, min_score=None):
        """pwa_align_wfa_sg_batch -> [dict(score, ops, end, start)] as align_gotoh_batch("sg", ...) returns them (end = (n, j), start =
        (0, j0)); score None, ops b"" and both cells (0, 0) for a pair not found."""
        return self._wfa_align(self._align_ops, "pwa_align_wfa_sg_batch", True, seqs, pair_a, pair_b, (match, mismatch, gap_open, gap_extend), min_score)

    def align_wfa_sg_batch_cigar(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, min_score=None):
        """pwa_align_wfa_sg_batch_cigar -> [dict(score, cigar, mdz, end, start)] as align_gotoh_batch_cigar("sg", ...) returns them;
        score None, two empty strings and both cells (0, 0) for a pair not found."""
        return self._wfa_align(self._align_strings, "pwa_align_wfa_sg_batch_cigar", True, seqs, pair_a, pair_b, (match, mismatch, gap_open, gap_extend), min_score)

    def align_wfa_stats(self):
        """The last scores_wfa / align_wfa_batch(_cigar) / scores_wfa_sg / align_wfa_sg_batch(_cigar): device ms of the sweeps and walks,
        wavefront cells swept, workspace bytes."""
        f, w, c, b = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pwa_wfa_last_stats(self._h, C.byref(f), C.byref(w), C.byref(c), C.byref(b)), "pwa_wfa_last_stats")
        return {"sweep_ms": f.value, "walk_ms": w.value, "cells": c.value, "workspace_bytes": b.value}

    # -- banded affine-gap alignments of long pairs: the gotoh calls inside a diagonal band per pair (include/pwalign.h)
    @staticmethod
    def _band_arrays(bands, n):
        if len(bands) != n:
            raise ValueError("bands: one (lo, hi) per pair")
        lo = (C.c_int32 * max(n, 1))(*[int(b[0]) for b in bands])
        hi = (C.c_int32 * max(n, 1))(*[int(b[1]) for b in bands])
        return lo, hi

    def align_banded_batch(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, bands):
        """pwa_align_banded_batch: align_gotoh_batch over the cells with lo <= j - i <= hi, bands = [(lo, hi)] per pair (band_around) ->
        [dict(score, ops, end, start)] as align_gotoh_batch returns them."""
        return self._align_ops(self._L.pwa_align_banded_batch, "pwa_align_banded_batch",
                               (self._h, MODE[mode], match, mismatch, gap_open, gap_extend), seqs, pair_a, pair_b,
                               self._band_arrays(bands, len(pair_a)))

    def align_banded_batch_cigar(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, bands):
        """pwa_align_banded_batch_cigar -> [dict(score, cigar, mdz, end, start)] as align_gotoh_batch_cigar returns them."""
        return self._align_strings(self._L.pwa_align_banded_batch_cigar, "pwa_align_banded_batch_cigar",
                                   (self._h, MODE[mode], match, mismatch, gap_open, gap_extend), seqs, pair_a, pair_b,
                                   self._band_arrays(bands, len(pair_a)))

    def align_banded_stats(self):
        """The last align_banded_batch(_cigar): device ms of its fills and walks, band bytes written."""
        return self._stats3(self._L.pwa_align_banded_last_stats, "pwa_align_banded_last_stats", "band_bytes")

    def scores_banded(self, mode, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, bands, want_end=False):
        """pwa_scores_banded: score (and, with want_end, end cell) of every pair of align_banded_batch's list, without the alignments:
        no traceback band, no walk -> scores, or (scores, end_i, end_j) as scores_gotoh_oneshot returns them."""
        return self._scores_call(self._L.pwa_scores_banded, "pwa_scores_banded", (self._h, MODE[mode], match, mismatch, gap_open, gap_extend),
                                 seqs, pair_a, pair_b, want_end, tail=self._band_arrays(bands, len(pair_a)))

    def scores_banded_stats(self):
        """The last scores_banded: device ms of its score passes, and the in-band cells of its list."""
        f, c = C.c_float(0), C.c_uint64(0)
        self._check(self._L.pwa_scores_banded_last_stats(self._h, C.byref(f), C.byref(c)), "pwa_scores_banded_last_stats")
        return dict(fill_ms=f.value, in_band_cells=c.value)

    # -- banded X-drop extension ("EXT"): anchored at (0, 0), free end, rows given up xdrop below the best (include/pwalign.h)
    def extend_banded_batch(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, bands, xdrop):
        """pwa_extend_banded_batch: extension alignments from (0, 0) inside bands = [(lo, hi)] per pair with lo <= 0 <= hi; xdrop < 0:
        no row stops -> [dict(score, ops, end, start, rows)] as align_banded_batch returns them, start = (0, 0), rows = the rows
        considered before the X-drop stopped the sweep."""
        return self._align_ops(self._L.pwa_extend_banded_batch, "pwa_extend_banded_batch",
                               (self._h, match, mismatch, gap_open, gap_extend, xdrop), seqs, pair_a, pair_b,
                               self._band_arrays(bands, len(pair_a)), ext=True)

    def extend_banded_batch_cigar(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, bands, xdrop):
        """pwa_extend_banded_batch_cigar -> [dict(score, cigar, mdz, end, start, rows)] as align_banded_batch_cigar returns them."""
        return self._align_strings(self._L.pwa_extend_banded_batch_cigar, "pwa_extend_banded_batch_cigar",
                                   (self._h, match, mismatch, gap_open, gap_extend, xdrop), seqs, pair_a, pair_b,
                                   self._band_arrays(bands, len(pair_a)), ext=True)

    def scores_extend_banded(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend, bands, xdrop, want_end=False):
        """pwa_scores_extend_banded: score (and, with want_end, end cell and rows) of every pair of extend_banded_batch's list, without
        the alignments -> scores, or (scores, end_i, end_j, rows)."""
        return self._scores_call(self._L.pwa_scores_extend_banded, "pwa_scores_extend_banded", (self._h, match, mismatch, gap_open, gap_extend, xdrop),
                                 seqs, pair_a, pair_b, want_end, extra=1, tail=self._band_arrays(bands, len(pair_a)))

    def extend_banded_stats(self):
        """The last extend_banded_batch(_cigar) or scores_extend_banded, or their _subst forms: device ms of its fills and walks (walk_ms = 0 after the scores
        call), and the rows it considered (the sum of `rows`)."""
        return self._stats3(self._L.pwa_extend_banded_last_stats, "pwa_extend_banded_last_stats", "rows_considered")

    # -- substitution-matrix scoring (table = subst_table(...)): the gotoh calls with s(i, j) = submat[code[p], code[t]]
    def _subst_head(self, mode, table, gap_open, gap_extend, blob):
        code, n_sym, submat, code_p, submat_p = _subst_args(table, blob)
        return (self._h, MODE[mode], code_p, n_sym, submat_p, gap_open, gap_extend), (code, submat)

    def align_subst_batch(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend):
        """pwa_align_subst_batch -> [dict(score, ops, end, start)] as align_gotoh_batch returns them."""
        packed = pack_sequences(seqs)
        head, _keep = self._subst_head(mode, table, gap_open, gap_extend, packed[0])
        return self._align_ops(self._L.pwa_align_subst_batch, "pwa_align_subst_batch", head, packed, pair_a, pair_b)

    def align_subst_batch_cigar(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend):
        """pwa_align_subst_batch_cigar -> [dict(score, cigar, mdz, end, start)]; MD:Z reports byte identity, not score sign."""
        packed = pack_sequences(seqs)
        head, _keep = self._subst_head(mode, table, gap_open, gap_extend, packed[0])
        return self._align_strings(self._L.pwa_align_subst_batch_cigar, "pwa_align_subst_batch_cigar", head, packed, pair_a, pair_b)

    def scores_subst(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend, want_end=False):
        b = self.batch_subst(mode, seqs, pair_a, pair_b, table, gap_open, gap_extend, want_end)
        b.run()
        out = b.fetch()
        b.close()
        return out

    def scores_subst_oneshot(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend, want_end=False):
        """pwa_scores_subst: the one-call form (pair lists of any size: cut into arena-sized runs by the library)."""
        packed = pack_sequences(seqs)
        head, _keep = self._subst_head(mode, table, gap_open, gap_extend, packed[0])
        return self._scores_call(self._L.pwa_scores_subst, "pwa_scores_subst", head, packed, pair_a, pair_b, want_end)

    # -- ... in a diagonal band per pair: patterns of any length (the banded calls with a table; they report into the banded stats)
    def align_banded_subst_batch(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend, bands):
        """pwa_align_banded_subst_batch: align_subst_batch over the cells with lo <= j - i <= hi, bands = [(lo, hi)] per pair ->
        [dict(score, ops, end, start)] as align_banded_batch returns them."""
        packed = pack_sequences(seqs)
        head, _keep = self._subst_head(mode, table, gap_open, gap_extend, packed[0])
        return self._align_ops(self._L.pwa_align_banded_subst_batch, "pwa_align_banded_subst_batch", head, packed, pair_a, pair_b,
                               self._band_arrays(bands, len(pair_a)))

    def align_banded_subst_batch_cigar(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend, bands):
        """pwa_align_banded_subst_batch_cigar -> [dict(score, cigar, mdz, end, start)] as align_banded_batch_cigar returns them; MD:Z
        reports byte identity, not score sign."""
        packed = pack_sequences(seqs)
        head, _keep = self._subst_head(mode, table, gap_open, gap_extend, packed[0])
        return self._align_strings(self._L.pwa_align_banded_subst_batch_cigar, "pwa_align_banded_subst_batch_cigar", head, packed, pair_a, pair_b,
                                   self._band_arrays(bands, len(pair_a)))

    def scores_banded_subst(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend, bands, want_end=False):
        """pwa_scores_banded_subst: score (and, with want_end, end cell) of every pair of align_banded_subst_batch's list, without the
        alignments -> scores, or (scores, end_i, end_j) as scores_banded returns them."""
        packed = pack_sequences(seqs)
        head, _keep = self._subst_head(mode, table, gap_open, gap_extend, packed[0])
        return self._scores_call(self._L.pwa_scores_banded_subst, "pwa_scores_banded_subst", head, packed, pair_a, pair_b, want_end,
                                 tail=self._band_arrays(bands, len(pair_a)))

    # -- ... and the X-drop extension calls with a table, which also say whether and how the extension reached the pattern's end
    def _ext_subst_head(self, table, gap_open, gap_extend, xdrop, blob):
        code, n_sym, submat, code_p, submat_p = _subst_args(table, blob)
        return (self._h, code_p, n_sym, submat_p, gap_open, gap_extend, xdrop), (code, submat)

    def extend_banded_subst_batch(self, seqs, pair_a, pair_b, table, gap_open, gap_extend, bands, xdrop):
        """pwa_extend_banded_subst_batch: extend_banded_batch under table = subst_table(...) -> [dict(score, ops, end, start, rows,
        pend)]; pend = (score, j) of the best cell of the pattern's last row when the sweep kept that row, else None."""
        packed = pack_sequences(seqs)
        head, _keep = self._ext_subst_head(table, gap_open, gap_extend, xdrop, packed[0])
        return self._align_ops(self._L.pwa_extend_banded_subst_batch, "pwa_extend_banded_subst_batch", head, packed, pair_a, pair_b,
                               self._band_arrays(bands, len(pair_a)), ext=True, pend=True)

    def extend_banded_subst_batch_cigar(self, seqs, pair_a, pair_b, table, gap_open, gap_extend, bands, xdrop):
        """pwa_extend_banded_subst_batch_cigar -> [dict(score, cigar, mdz, end, start, rows, pend)]; MD:Z reports byte identity, not
        score sign."""
        packed = pack_sequences(seqs)
        head, _keep = self._ext_subst_head(table, gap_open, gap_extend, xdrop, packed[0])
        return self._align_strings(self._L.pwa_extend_banded_subst_batch_cigar, "pwa_extend_banded_subst_batch_cigar", head, packed, pair_a, pair_b,
                                   self._band_arrays(bands, len(pair_a)), ext=True, pend=True)

    def scores_extend_banded_subst(self, seqs, pair_a, pair_b, table, gap_open, gap_extend, bands, xdrop, want_end=False):
        """pwa_scores_extend_banded_subst: score (and, with want_end, end cell, rows and pattern-end result) of every pair of
        extend_banded_subst_batch's list, without the alignments -> scores, or (scores, end_i, end_j, rows, pend) with pend a list of
        (score, j) or None.  Stats: extend_banded_stats."""
        packed = pack_sequences(seqs)
        head, _keep = self._ext_subst_head(table, gap_open, gap_extend, xdrop, packed[0])
        return self._scores_call(self._L.pwa_scores_extend_banded_subst, "pwa_scores_extend_banded_subst", head, packed, pair_a, pair_b, want_end,
                                 extra=1, pend=True, tail=self._band_arrays(bands, len(pair_a)))

    def batch_subst(self, mode, seqs, pair_a, pair_b, table, gap_open, gap_extend, want_end=False):
        return Batch(self, mode, seqs, pair_a, pair_b, 0, 0, gap_open, want_end, gap_extend=gap_extend, subst=table)

    def align_subst_stats(self):
        """The last align_subst_batch(_cigar): device ms of its fills and walks, band bytes written."""
        return self._stats3(self._L.pwa_align_subst_last_stats, "pwa_align_subst_last_stats", "band_bytes")

    def align_gotoh_stats(self):
        """The last align_gotoh_batch(_cigar): device ms of its fills and walks, band bytes written."""
        return self._stats3(self._L.pwa_align_gotoh_last_stats, "pwa_align_gotoh_last_stats", "band_bytes")

    def align_batch_arrays(self, mode, packed, pair_a, pair_b, match, mismatch, gap, out=None):
        """pwa_align_batch on caller-held buffers, the way a compiled host calls it: `packed` = pack_sequences(seqs) done once,
        pair_a / pair_b numpy uint32 arrays, `out` the dict a previous call returned (its arrays are reused, nothing is
        allocated or converted per call).  Returns dict(scores, n_ops, ops, ops_off, end, start) of numpy arrays; the ops of
        pair k are ops[ops_off[k] : ops_off[k] + n_ops[k]]."""
        import numpy as np
        blob, off, seqs = packed
        n = len(pair_a)
        if out is None:
            lens = np.array([len(x) for x in seqs], dtype=np.uint64)
            cap = lens[pair_a] + lens[pair_b]
            ops_off = np.zeros(max(n, 1), dtype=np.uint64)
            if n > 1:
                ops_off[1:n] = np.cumsum(cap[:-1])
            out = dict(scores=np.zeros(max(n, 1), dtype=np.int32), n_ops=np.zeros(max(n, 1), dtype=np.uint64),
                       ops=np.zeros(int(cap.sum()) + 1, dtype=np.uint8), ops_off=ops_off,
                       end=np.zeros((max(n, 1), 2), dtype=np.uint64), start=np.zeros((max(n, 1), 2), dtype=np.uint64))
        u32p, u64p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
        rc = self._L.pwa_align_batch(self._h, MODE[mode], match, mismatch, gap, blob, off, len(seqs),
                                     pair_a.ctypes.data_as(u32p), pair_b.ctypes.data_as(u32p), n, out["scores"].ctypes.data_as(i32p),
                                     out["ops"].ctypes.data_as(C.c_void_p), out["ops_off"].ctypes.data_as(u64p),
                                     out["n_ops"].ctypes.data_as(u64p), out["end"].ctypes.data_as(u64p), out["start"].ctypes.data_as(u64p))
        self._check(rc, "pwa_align_batch")
        return out

    def align_affine_batch(self, seqs, pair_a, pair_b, match, mismatch, gap_open, gap_extend):
        """hw3.cpp:23-135 for a pair list -> [dict(score, ops)], ops in traceback order ('M' / 'D' / 'I')."""
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        ooff = (C.c_uint64 * max(n, 1))()
        tot = 0
        for k in range(n):
            ooff[k] = tot
            tot += len(seqs[pair_a[k]]) + len(seqs[pair_b[k]])
        ops = C.create_string_buffer(tot + 1)
        sc = (C.c_int32 * max(n, 1))()
        nops = (C.c_uint64 * max(n, 1))()
        rc = self._L.pwa_align_affine_batch(self._h, match, mismatch, gap_open, gap_extend, blob, off, len(seqs), pa, pb, n, sc,
                                            ops, ooff, nops)
        self._check(rc, "pwa_align_affine_batch")
        raw = memoryview(ops)
        return [dict(score=sc[k], ops=bytes(raw[ooff[k]:ooff[k] + nops[k]])) for k in range(n)]

    def overlaps(self, mode, seqs, pair_a, pair_b, match, mismatch, gap):
        """(scores, overlaps) of full alignments without their op lists: the -g selection inputs (hw2.cpp:342-350)."""
        blob, off, seqs = pack_sequences(seqs)
        n = len(pair_a)
        pa = (C.c_uint32 * max(n, 1))(*pair_a)
        pb = (C.c_uint32 * max(n, 1))(*pair_b)
        sc = (C.c_int32 * max(n, 1))()
        ov = (C.c_int32 * max(n, 1))()
        rc = self._L.pwa_overlaps(self._h, MODE[mode], match, mismatch, gap, blob, off, len(seqs), pa, pb, n, sc, ov)
        self._check(rc, "pwa_overlaps")
        return list(sc[:n]), list(ov[:n])

    def align_stats(self):
        f, t, b = C.c_float(0), C.c_float(0), C.c_uint64(0)
        self._L.pwa_align_last_stats(self._h, C.byref(f), C.byref(t), C.byref(b))
        return dict(fill_ms=f.value, traceback_ms=t.value, band_bytes=b.value)

    def align_affine_stats(self):
        """The last align_affine_batch: pairs on the stripe engine, device ms of their fills / walks, band bytes written."""
        p, f, w, b = C.c_uint64(0), C.c_float(0), C.c_float(0), C.c_uint64(0)
        self._check(self._L.pwa_align_affine_last_stats(self._h, C.byref(p), C.byref(f), C.byref(w), C.byref(b)), "pwa_align_affine_last_stats")
        return dict(stripe_pairs=p.value, fill_ms=f.value, walk_ms=w.value, band_bytes=b.value)


    # -- hw1: suffix array of one text, exact pattern search (include/pwalign.h, pwa_sa_*)
    def _sa_index(self, text):
        text = _b(text)
        ix = C.c_void_p()
        self._check(self._L.pwa_sa_create(self._h, text, len(text), C.byref(ix)), "pwa_sa_create")
        return ix

    def _sa_stats(self, ix):
        r, b, s = C.c_uint32(0), C.c_float(0), C.c_float(0)
        self._L.pwa_sa_last_stats(ix, C.byref(r), C.byref(b), C.byref(s))
        self.sa_stats = dict(rounds=r.value, build_ms=b.value, search_ms=s.value)

    def suffix_array(self, text):
        """The suffixes of text in signed-char order, as a list of start positions (built on the device)."""
        ix = self._sa_index(text)
        try:
            n = len(text)
            out = (C.c_uint32 * max(n, 1))()
            self._check(self._L.pwa_sa_fetch(ix, out), "pwa_sa_fetch")
            self._sa_stats(ix)
            return list(out[:n])
        finally:
            self._L.pwa_sa_destroy(ix)

    def find(self, text, patterns, refs=None):
        """refs None: per pattern, the number of its occurrences anywhere in text.  refs = (ref_start, header_rank): reference r is
        text[ref_start[r]:ref_start[r + 1]] with its terminator last; per pattern, the sorted list of (header_rank, local position)
        of its occurrences that do not start on a terminator."""
        blob, off, pats = pack_sequences(patterns)
        n_pat = len(pats)
        ix = self._sa_index(text)
        try:
            cnt = (C.c_uint32 * max(n_pat, 1))()
            self._check(self._L.pwa_sa_find(ix, blob, off, n_pat, cnt), "pwa_sa_find")
            if refs is None:
                self._sa_stats(ix)
                return list(cnt[:n_pat])
            ref_start, header_rank = refs
            rs = (C.c_uint32 * len(ref_start))(*ref_start)
            hr = (C.c_uint32 * max(len(header_rank), 1))(*header_rank)
            cap = sum(cnt[:n_pat])
            occ_off = (C.c_uint64 * (n_pat + 1))()
            occ = (C.c_uint64 * max(cap, 1))()
            need = C.c_uint64(0)
            self._check(self._L.pwa_sa_occurrences(ix, blob, off, n_pat, rs, len(ref_start) - 1, hr, occ_off, occ, cap, C.byref(need)),
                        "pwa_sa_occurrences")
            self._sa_stats(ix)
            return [[(occ[e] >> 32, occ[e] & 0xffffffff) for e in range(occ_off[k], occ_off[k + 1])] for k in range(n_pat)]
        finally:
            self._L.pwa_sa_destroy(ix)

    # -- k-edit approximate search of one text (include/pwalign.h, pwa_approx_*)
    def _approx_args(self, text, patterns, k):
        blob, off, pats = pack_sequences(patterns)
        n_pat = len(pats)
        ks = [k] * n_pat if isinstance(k, int) else list(k)
        if len(ks) != n_pat:
            raise ValueError("k: one int, or one per pattern")
        return _b(text), blob, off, n_pat, (C.c_uint32 * max(n_pat, 1))(*ks)

    def _approx_stats(self):
        c, f, t, col = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pwa_approx_last_stats(self._h, C.byref(c), C.byref(f), C.byref(t), C.byref(col)), "pwa_approx_last_stats")
        self.approx_stats = dict(count_ms=c.value, fill_ms=f.value, tasks=t.value, columns=col.value)

    def count_approx(self, text, patterns, k):
        """Per pattern, the ends e in 1 .. len(text) where it matches text[.. e) within k edits (k: one int, or one per pattern):
        (counts, best), best[q] = (dist, end) of the smallest distance and, at that distance, the smallest end, or None."""
        text, blob, off, n_pat, kd = self._approx_args(text, patterns, k)
        cnt = (C.c_uint32 * max(n_pat, 1))()
        bd = (C.c_int32 * max(n_pat, 1))()
        be = (C.c_uint32 * max(n_pat, 1))()
        self._check(self._L.pwa_approx_find(self._h, text, len(text), blob, off, n_pat, kd, cnt, bd, be), "pwa_approx_find")
        self._approx_stats()
        return list(cnt[:n_pat]), [(bd[q], be[q]) if bd[q] >= 0 else None for q in range(n_pat)]

    def find_approx(self, text, patterns, k):
        """Per pattern, the list of (end, dist) of its hits in ascending end."""
        text, blob, off, n_pat, kd = self._approx_args(text, patterns, k)
        cnt = (C.c_uint32 * max(n_pat, 1))()
        self._check(self._L.pwa_approx_find(self._h, text, len(text), blob, off, n_pat, kd, cnt, None, None), "pwa_approx_find")
        cap = sum(cnt[:n_pat])
        occ_off = (C.c_uint64 * (n_pat + 1))()
        occ = (C.c_uint64 * max(cap, 1))()
        need = C.c_uint64(0)
        self._check(self._L.pwa_approx_occurrences(self._h, text, len(text), blob, off, n_pat, kd, occ_off, occ, cap, C.byref(need)),
                    "pwa_approx_occurrences")
        self._approx_stats()
        return [[(occ[x] >> 32, occ[x] & 0xffffffff) for x in range(occ_off[q], occ_off[q + 1])] for q in range(n_pat)]

    # -- from a hit to a placement: starts, locally minimal ends, alignments (include/pwalign.h, pwa_approx_starts / pwa_approx_minima)
    def starts_approx(self, text, patterns, hits):
        """Per pattern, the starts of its hits [(end, dist)], parallel to them: the largest s with ed(pattern, text[s:end]) <= dist,
        None where there is none (a dist below the true distance of that end).  Any subset of find_approx's hits, in any order."""
        blob, off, pats = pack_sequences(patterns)
        n_pat = len(pats)
        if len(hits) != n_pat:
            raise ValueError("hits: one list of (end, dist) per pattern")
        text = _b(text)
        occ_off, occ = _pack_hits(hits)
        total = occ_off[n_pat]
        out = (C.c_uint32 * max(total, 1))()
        self._check(self._L.pwa_approx_starts(self._h, text, len(text), blob, off, n_pat, occ_off, occ, out), "pwa_approx_starts")
        ms, nh, col = C.c_float(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pwa_approx_starts_last_stats(self._h, C.byref(ms), C.byref(nh), C.byref(col)), "pwa_approx_starts_last_stats")
        self.approx_starts_stats = dict(ms=ms.value, hits=nh.value, columns=col.value)
        return [[None if out[x] == APPROX_NO_START else out[x] for x in range(occ_off[q], occ_off[q + 1])] for q in range(n_pat)]

    def locate_approx(self, text, patterns, k, select="minima"):
        """Per pattern, [(start, end, dist)] in ascending end of its hits within k edits: find_approx, then the selection -- "all":
        every hit; "minima": the locally minimal ends (approx_minima); "best": the one hit count_approx names -- then starts_approx."""
        if select not in ("minima", "all", "best"):
            raise ValueError('select: "minima", "all" or "best"')
        blob, off, pats = packed = pack_sequences(patterns)
        hits = self.find_approx(text, packed, k)
        if select == "minima":
            hits = approx_minima(hits, [len(p) for p in pats], k, len(_b(text)))
        elif select == "best":
            hits = [[min(h, key=lambda x: (x[1], x[0]))] if h else [] for h in hits]
        starts = self.starts_approx(text, packed, hits)
        return [[(s, e, d) for s, (e, d) in zip(ss, h)] for ss, h in zip(starts, hits)]

    def align_approx(self, text, patterns, k, select="minima"):
        """Per pattern, [dict(start, end, dist, score, cigar, mdz)] of locate_approx's placements: the global alignment of the pattern
        against text[start:end] under unit costs (align_gotoh_batch_cigar("nw", ..., 0, -1, 0, -1)), so score == -dist; a hit with
        start == end follows that call's empty-side convention."""
        blob, off, pats = packed = pack_sequences(patterns)
        text = _b(text)
        placed = self.locate_approx(text, packed, k, select)
        seqs, pa, pb = list(pats), [], []
        for q, pl in enumerate(placed):
            for s, e, _ in pl:
                pa.append(q)
                pb.append(len(seqs))
                seqs.append(text[s:e])
        al = self.align_gotoh_batch_cigar("nw", seqs, pa, pb, 0, -1, 0, -1) if pa else []
        out, at = [], 0
        for pl in placed:
            out.append([dict(start=s, end=e, dist=d, score=a["score"], cigar=a["cigar"], mdz=a["mdz"]) for (s, e, d), a in zip(pl, al[at:at + len(pl)])])
            at += len(pl)
        return out

    # -- from seeds to placements: seeding on the suffix array, collinear chaining (include/pwalign.h, pwa_chain_*), banded alignment
    def chain(self, anchors, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38, want_dp=False):
        """pwa_chain_anchors: the best collinear chain of every read's anchors.  anchors: per read its (t, q, len) triples in
        non-decreasing order of (t + len, q + len) -> per read dict(score, count, last, q_begin, q_end, t_begin, t_end, diag_lo,
        diag_hi), and with want_dp the whole DP as lists f and pred (local indices).  A read without anchors: score 0, count 0,
        last None.  Sets chain_stats = dict(chain_ms, anchors, ranges)."""
        import numpy as np
        t, q, ln, off = _anchor_arrays(anchors)
        n = len(off) - 1
        sc = np.zeros(max(n, 1), dtype=np.int32)
        cnt, last, span = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(4 * max(n, 1), dtype=np.uint32)
        diag = np.zeros(2 * max(n, 1), dtype=np.int32)
        tot = int(off[n])
        f = np.zeros(max(tot, 1), dtype=np.int32) if want_dp else None
        pr = np.zeros(max(tot, 1), dtype=np.int32) if want_dp else None
        i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        rc = self._L.pwa_chain_anchors(self._h, _u32p(t), _u32p(q), _u32p(ln), off.ctypes.data_as(C.POINTER(C.c_uint64)), n, lookback, max_dist,
                                       bandwidth, gap_scale, i32(sc), _u32p(cnt), _u32p(last), _u32p(span), i32(diag), i32(f), i32(pr))
        self._check(rc, "pwa_chain_anchors")
        ms, na, nr = C.c_float(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pwa_chain_last_stats(self._h, C.byref(ms), C.byref(na), C.byref(nr)), "pwa_chain_last_stats")
        self.chain_stats = dict(chain_ms=ms.value, anchors=na.value, ranges=nr.value)
        sc, cnt, last, span, diag, o = sc.tolist(), cnt.tolist(), last.tolist(), span.tolist(), diag.tolist(), off.tolist()
        out = []
        for r in range(n):
            d = dict(score=sc[r], count=cnt[r], last=None if last[r] == CHAIN_NO_READ else last[r], q_begin=span[4 * r], q_end=span[4 * r + 1],
                     t_begin=span[4 * r + 2], t_end=span[4 * r + 3], diag_lo=diag[2 * r], diag_hi=diag[2 * r + 1])
            if want_dp:
                d["f"] = f[o[r]:o[r + 1]].tolist()
                d["pred"] = pr[o[r]:o[r + 1]].tolist()
            out.append(d)
        return out

    def chain_top(self, anchors, max_chains=4, min_score=40, min_count=3, rooted=False, lookback=64, max_dist=5000, bandwidth=500, gap_scale=38,
                  want_dp=False, want_ids=False):
        """pwa_chain_top: up to max_chains chains of every read's anchors, best first, selected on the device by marked back-walks
        over chain()'s DP (a walk that runs into an anchor of an earlier walk stops there and scores what it adds; with rooted such a
        walk is not kept), and the read's mapping quality.  anchors as for chain() -> per read dict(chains=[dict(chain()'s keys plus
        branch: the anchor the walk stopped before, or -1)], mapq), with want_dp the lists f and pred, with want_ids the list chain_id
        (per anchor its kept chain's index, or -1).  Sets chain_top_stats = dict(chain_ms, top_ms, anchors, rounds, ranges)."""
        import numpy as np
        t, q, ln, off = _anchor_arrays(anchors)
        n, N = len(off) - 1, max(int(max_chains), 1)
        slots = max(n, 1) * N
        nch, mq = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        sc, br = np.zeros(slots, dtype=np.int32), np.zeros(slots, dtype=np.int32)
        cnt, last, span = np.zeros(slots, dtype=np.uint32), np.zeros(slots, dtype=np.uint32), np.zeros(4 * slots, dtype=np.uint32)
        diag = np.zeros(2 * slots, dtype=np.int32)
        tot = int(off[n])
        f = np.zeros(max(tot, 1), dtype=np.int32) if want_dp else None
        pr = np.zeros(max(tot, 1), dtype=np.int32) if want_dp else None
        ids = np.zeros(max(tot, 1), dtype=np.int32) if want_ids else None
        i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        rc = self._L.pwa_chain_top(self._h, _u32p(t), _u32p(q), _u32p(ln), off.ctypes.data_as(C.POINTER(C.c_uint64)), n, lookback, max_dist, bandwidth,
                                   gap_scale, max_chains, min_score, min_count, CHAIN_ROOTED if rooted else 0, _u32p(nch), i32(sc), _u32p(cnt), _u32p(last),
                                   _u32p(span), i32(diag), i32(br), _u32p(mq), i32(f), i32(pr), i32(ids))
        self._check(rc, "pwa_chain_top")
        cm, tm, na, nro, nr = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.pwa_chain_top_last_stats(self._h, C.byref(cm), C.byref(tm), C.byref(na), C.byref(nro), C.byref(nr)), "pwa_chain_top_last_stats")
        self.chain_top_stats = dict(chain_ms=cm.value, top_ms=tm.value, anchors=na.value, rounds=nro.value, ranges=nr.value)
        nch, mq, sc, br, cnt, last, span, diag, o = (a.tolist() for a in (nch, mq, sc, br, cnt, last, span, diag, off))
        out = []
        for r in range(n):
            d = dict(chains=[dict(score=sc[s], count=cnt[s], last=last[s], q_begin=span[4 * s], q_end=span[4 * s + 1], t_begin=span[4 * s + 2],
                                  t_end=span[4 * s + 3], diag_lo=diag[2 * s], diag_hi=diag[2 * s + 1], branch=br[s]) for s in range(r * N, r * N + nch[r])],
                     mapq=mq[r])
            if want_dp:
                d["f"] = f[o[r]:o[r + 1]].tolist()
                d["pred"] = pr[o[r]:o[r + 1]].tolist()
            if want_ids:
                d["chain_id"] = ids[o[r]:o[r + 1]].tolist()
            out.append(d)
        return out

    def index(self, text, minimizers=None, canonical=False):
        """A TextIndex of text: its suffix array, built once on the device and kept for any number of seed() / map_reads() calls.
        With minimizers=(k, w) a MinimizerIndex instead: the text's (w, k)-minimizer sketch sorted by hash, for the same calls; with
        canonical=True its canonical form (pwa_mm_create_canonical), which seed_strands() and map_reads() seed on both strands from
        one sketch of every read."""
        if minimizers is not None:
            k, w = minimizers
            return MinimizerIndex(self, text, k, w, canonical)
        if canonical:
            raise ValueError("index: canonical=True goes with minimizers=(k, w)")
        return TextIndex(self, text)

    def sketch(self, seqs, k, w, as_arrays=False, canonical=False):
        """pwa_mm_sketch: the (w, k)-minimizer sketch of every sequence -> per sequence a list of (pos, hash) in ascending pos, or
        with as_arrays a pair of arrays (pos uint32, hash uint64).  With canonical=True pwa_mm_sketch_canonical: (pos, hash, strand),
        the hash that of the smaller of the k-mer and its reverse complement, strand 1 where that is the reverse complement (uint8)."""
        import numpy as np
        if not (1 <= k <= 31 and 1 <= w <= 128):
            raise ValueError("sketch: k is 1 .. 31 and w is 1 .. 128")
        seqs = [_b(s) for s in seqs]
        n = len(seqs)
        u64p = C.POINTER(C.c_uint64)
        off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum([len(s) for s in seqs])
        cap = sum(max(len(s) - k + 1, 0) for s in seqs)
        min_off = np.zeros(n + 1, dtype=np.uint64)
        pos, hsh = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint64)
        need = C.c_uint64(0)
        if canonical:
            std = np.zeros(max(cap, 1), dtype=np.uint8)
            self._check(self._L.pwa_mm_sketch_canonical(self._h, b"".join(seqs), off.ctypes.data_as(u64p), n, k, w, min_off.ctypes.data_as(u64p), _u32p(pos),
                                                        hsh.ctypes.data_as(u64p), std.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(need)),
                        "pwa_mm_sketch_canonical")
            cut = min_off.astype(np.int64).tolist()
            if as_arrays:
                return [(pos[cut[i]:cut[i + 1]], hsh[cut[i]:cut[i + 1]], std[cut[i]:cut[i + 1]]) for i in range(n)]
            rows = list(zip(pos[:cut[n]].tolist(), hsh[:cut[n]].tolist(), std[:cut[n]].tolist()))
            return [rows[cut[i]:cut[i + 1]] for i in range(n)]
        self._check(self._L.pwa_mm_sketch(self._h, b"".join(seqs), off.ctypes.data_as(u64p), n, k, w, min_off.ctypes.data_as(u64p), _u32p(pos),
                                          hsh.ctypes.data_as(u64p), cap, C.byref(need)), "pwa_mm_sketch")
        cut = min_off.astype(np.int64).tolist()
        if as_arrays:
            return [(pos[cut[i]:cut[i + 1]], hsh[cut[i]:cut[i + 1]]) for i in range(n)]
        pairs = list(zip(pos[:cut[n]].tolist(), hsh[:cut[n]].tolist()))
        return [pairs[cut[i]:cut[i + 1]] for i in range(n)]

    @staticmethod
    def _on_minimizers(index, k, step):
        if k != index.k or step != 1:
            raise ValueError("a MinimizerIndex seeds with its own k (%d) and step 1" % index.k)

    def seed(self, text, reads, k, step=1, max_occ=64, as_arrays=False):
        """Exact k-mer anchors of every read in the text (bytes: a temporary index of it is built; or a TextIndex), pwa_sa_seed: the
        k-mers read[q:q + k] at q = 0, step, 2 step, ... are cut, searched, gathered and sorted on the device; a k-mer with more than
        max_occ occurrences is dropped.  -> per read its anchors (t, q, k) in the order chain() requires (by t, then q), as a list of
        tuples, or with as_arrays as a uint32 array of shape (n, 3).  Sets seed_stats = dict(search_ms, sort_ms, slots, hits, ranges).
        On a MinimizerIndex (k its own, step 1, else ValueError) the anchors are those of MinimizerIndex.seed; a canonical one is
        seeded by its seed_strands() instead (ValueError here)."""
        if isinstance(text, MinimizerIndex):
            self._on_minimizers(text, k, step)
            return text.seed(reads, max_occ, as_arrays)
        if isinstance(text, TextIndex):
            return text.seed(reads, k, step, max_occ, as_arrays)
        if k < 1 or step < 1 or max_occ < 1:
            raise ValueError("seed: k, step and max_occ are at least 1")
        with TextIndex(self, text) as ix:
            return ix.seed(reads, k, step, max_occ, as_arrays)

    def map_reads(self, text, reads, k, match, mismatch, gap_open, gap_extend, w=100, step=1, max_occ=64, both_strands=False, lookback=64,
                  max_dist=5000, bandwidth=500, gap_scale=38, secondary=0, min_chain_score=40, min_chain_count=3):
        """Seed, chain, align (text: bytes, or a TextIndex or MinimizerIndex kept across calls; the latter with its own k and step 1; a canonical MinimizerIndex is seeded by seed_strands() of the reads as given, no reverse complement is built but that of a read placed on '-'): seed() of every read (with both_strands also of its reverse complement; the strand with the higher
        chain score is kept, ties go forward), chain() of the anchors, then align_banded_batch_cigar("sg", ...) of the read against
        the text window [max(0, t_begin - q_begin - w), min(len(text), t_end + (n - q_end) + w)) in the band (diag_lo - window start -
        w, diag_hi - window start + w).  -> per read dict(pos, end, score, cigar, mdz, strand, chain_score) in text coordinates
        (strand '+' or '-'; cigar and mdz are of the aligned strand), or None for a read without a chain, or whose band is wider than
        the banded call's 4096 or fails its semi-global validity rule.  Sets map_stats = dict(seed_s, chain_s, align_s): wall seconds.
        With secondary = S in 1 .. 15 the chains come from chain_top(max_chains=S + 1, min_chain_score, min_chain_count, rooted) of
        every strand's anchors: a read's kept chains of both strands are pooled and ordered by score descending, then forward strand
        first, then chain index; the first is the primary, the next up to S the secondaries, all aligned in the one banded call.  The
        primary's dict gains mapq = mapq(its chain score, the second pooled score or 0, its chain count) and secondary: a list of
        dicts with the keys above (a secondary whose band fails is left out; a primary whose band fails makes the read None)."""
        import time
        if secondary:
            if not 1 <= secondary <= 15:
                raise ValueError("map_reads: secondary is 0 .. 15")
            return self._map_reads_secondary(text, reads, k, match, mismatch, gap_open, gap_extend, w, step, max_occ, both_strands, lookback, max_dist,
                                             bandwidth, gap_scale, secondary, min_chain_score, min_chain_count)
        index = text if isinstance(text, (TextIndex, MinimizerIndex)) else None   # bytes: seed() builds a temporary index, inside seed_s
        text = index.text if index else _b(text)
        fw = [_b(r) for r in reads]
        nr = len(fw)
        strands = self._strand_lists(index, fw, both_strands)
        t0 = time.perf_counter()
        anchors = self._seed_strand_lists(index, text, strands, k, step, max_occ)
        t1 = time.perf_counter()
        chains = self.chain(anchors, lookback, max_dist, bandwidth, gap_scale)
        t2 = time.perf_counter()
        pats, wins, bands, placed = [], [], [], []   # placed: (read, strand, window start, chain score)
        for i in range(nr):
            s = 1 if both_strands and chains[nr + i]["score"] > chains[i]["score"] else 0
            c = chains[s * nr + i]
            if not c["count"]:
                continue
            n = len(fw[i])
            ws = max(0, c["t_begin"] - c["q_begin"] - w)
            we = min(len(text), c["t_end"] + (n - c["q_end"]) + w)
            lo, hi = c["diag_lo"] - ws - w, c["diag_hi"] - ws + w
            if hi - lo + 1 > 4096 or hi < 0 or n + lo > we - ws:
                continue
            pats.append(self._strand_read(strands, s, i))
            wins.append(text[ws:we])
            bands.append((lo, hi))
            placed.append((i, "+-"[s], ws, c["score"]))
        np_ = len(pats)
        al = self.align_banded_batch_cigar("sg", pats + wins, list(range(np_)), list(range(np_, 2 * np_)), match, mismatch, gap_open, gap_extend,
                                           bands) if np_ else []
        t3 = time.perf_counter()
        self.map_stats = dict(seed_s=t1 - t0, chain_s=t2 - t1, align_s=t3 - t2)
        out = [None] * nr
        for (i, strand, ws, cs), a in zip(placed, al):
            out[i] = dict(pos=ws + a["start"][1], end=ws + a["end"][1], score=a["score"], cigar=a["cigar"], mdz=a["mdz"], strand=strand, chain_score=cs)
        return out

    @staticmethod
    def _strand_lists(index, fw, both_strands):
        """map_reads' strands: strands[s][i] = read i as strand s is aligned.  Under a canonical MinimizerIndex the reverse strand
        starts as None entries, which _strand_read fills for the reads placed there."""
        if not both_strands:
            return [fw]
        if isinstance(index, MinimizerIndex) and index.canonical:
            return [fw, [None] * len(fw)]
        return [fw, [revcomp(r) for r in fw]]

    def _seed_strand_lists(self, index, text, strands, k, step, max_occ):
        """map_reads' seeding: anchors[s * n + i] = the anchor list of strands[s][i].  A canonical MinimizerIndex seeds both
        strands from the reads as given."""
        if isinstance(index, MinimizerIndex) and index.canonical:
            self._on_minimizers(index, k, step)
            anchors = index.seed_strands(strands[0], max_occ, as_arrays=True)
            return anchors[:len(strands) * len(strands[0])]
        return self.seed(index or text, [r for s in strands for r in s], k, step, max_occ, as_arrays=True)

    @staticmethod
    def _strand_read(strands, s, i):
        if strands[s][i] is None:
            strands[s][i] = revcomp(strands[0][i])
        return strands[s][i]

    def _map_reads_secondary(self, text, reads, k, match, mismatch, gap_open, gap_extend, w, step, max_occ, both_strands, lookback, max_dist, bandwidth,
                             gap_scale, secondary, min_chain_score, min_chain_count):
        """map_reads with secondary >= 1: the top chains of every strand pooled per read, one banded call for all their windows"""
        import time
        index = text if isinstance(text, (TextIndex, MinimizerIndex)) else None
        text = index.text if index else _b(text)
        fw = [_b(r) for r in reads]
        nr = len(fw)
        strands = self._strand_lists(index, fw, both_strands)
        t0 = time.perf_counter()
        anchors = self._seed_strand_lists(index, text, strands, k, step, max_occ)
        t1 = time.perf_counter()
        tops = self.chain_top(anchors, secondary + 1, min_chain_score, min_chain_count, True, lookback, max_dist, bandwidth, gap_scale)
        t2 = time.perf_counter()
        pats, wins, bands, placed = [], [], [], []   # placed: (read, rank in its pool, strand, window start, chain)
        second = [0] * nr
        for i in range(nr):
            pool = sorted(((s, ci, c) for s in range(len(strands)) for ci, c in enumerate(tops[s * nr + i]["chains"])),
                          key=lambda e: (-e[2]["score"], e[0], e[1]))[:secondary + 1]
            second[i] = pool[1][2]["score"] if len(pool) > 1 else 0
            n = len(fw[i])
            for rank, (s, _, c) in enumerate(pool):
                ws = max(0, c["t_begin"] - c["q_begin"] - w)
                we = min(len(text), c["t_end"] + (n - c["q_end"]) + w)
                lo, hi = c["diag_lo"] - ws - w, c["diag_hi"] - ws + w
                if hi - lo + 1 > 4096 or hi < 0 or n + lo > we - ws:
                    if rank == 0:
                        break    # no primary: the read is None
                    continue
                pats.append(self._strand_read(strands, s, i))
                wins.append(text[ws:we])
                bands.append((lo, hi))
                placed.append((i, rank, "+-"[s], ws, c))
        np_ = len(pats)
        al = self.align_banded_batch_cigar("sg", pats + wins, list(range(np_)), list(range(np_, 2 * np_)), match, mismatch, gap_open, gap_extend,
                                           bands) if np_ else []
        t3 = time.perf_counter()
        self.map_stats = dict(seed_s=t1 - t0, chain_s=t2 - t1, align_s=t3 - t2)
        out = [None] * nr
        for (i, rank, strand, ws, c), a in zip(placed, al):
            d = dict(pos=ws + a["start"][1], end=ws + a["end"][1], score=a["score"], cigar=a["cigar"], mdz=a["mdz"], strand=strand, chain_score=c["score"])
            if rank == 0:
                d["mapq"] = mapq(c["score"], second[i], c["count"])
                d["secondary"] = []
                out[i] = d
            else:
                out[i]["secondary"].append(d)
        return out


class TextIndex:
    """The suffix-array index of one text, resident on the context's GPU (pwa_sa_create): built once, then seeded against by any number
    of read lists (pwa_sa_seed).  Keeps the text bytes (map_reads cuts its windows from them).  stats = dict(rounds, build_ms) of the
    build; close() frees it, and it works as a context manager.  Close it before its context."""

    def __init__(self, ctx, text):
        self._ctx, self._L = ctx, ctx._L
        self.text = _b(text)
        self._ix = ctx._sa_index(self.text)
        ctx._sa_stats(self._ix)
        self.stats = dict(rounds=ctx.sa_stats["rounds"], build_ms=ctx.sa_stats["build_ms"])
        self.seed_stats = None

    def close(self):
        if getattr(self, "_ix", None):
            self._L.pwa_sa_destroy(self._ix)
            self._ix = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def seed(self, reads, k, step=1, max_occ=64, as_arrays=False):
        """pwa_sa_seed + pwa_sa_seed_fetch: Context.seed on this index -> per read its anchors (t, q, k) by t, then q, as a list of
        tuples or, with as_arrays, a uint32 array of shape (n, 3).  Sets seed_stats = dict(search_ms, sort_ms, slots, hits, ranges)
        here and on the context: device ms of the search kernel and of gather + sort + split, the list's k-mers, the hits kept, the
        ranges of reads the call ran."""
        import numpy as np
        if k < 1 or step < 1 or max_occ < 1:
            raise ValueError("seed: k, step and max_occ are at least 1")
        if not self._ix:
            raise PwaError("TextIndex.seed: the index is closed")
        reads = [_b(r) for r in reads]
        n = len(reads)
        off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum([len(r) for r in reads])
        u64p = C.POINTER(C.c_uint64)
        anc_off = np.zeros(n + 1, dtype=np.uint64)
        ck = self._ctx._check
        ck(self._L.pwa_sa_seed(self._ix, b"".join(reads), off.ctypes.data_as(u64p), n, k, step, max_occ, anc_off.ctypes.data_as(u64p)), "pwa_sa_seed")
        total = int(anc_off[n])
        trip = np.empty((total, 3), dtype=np.uint32)
        t, q = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.uint32)
        ck(self._L.pwa_sa_seed_fetch(self._ix, _u32p(t), _u32p(q), total), "pwa_sa_seed_fetch")
        trip[:, 0], trip[:, 1], trip[:, 2] = t[:total], q[:total], k
        sm, om, ns, nh, nr = C.c_float(0), C.c_float(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ck(self._L.pwa_sa_seed_last_stats(self._ix, C.byref(sm), C.byref(om), C.byref(ns), C.byref(nh), C.byref(nr)), "pwa_sa_seed_last_stats")
        self.seed_stats = self._ctx.seed_stats = dict(search_ms=sm.value, sort_ms=om.value, slots=ns.value, hits=nh.value, ranges=nr.value)
        cut = anc_off.astype(np.int64).tolist()
        if as_arrays:
            return [trip[cut[i]:cut[i + 1]] for i in range(n)]
        rows = trip.tolist()
        return [[tuple(x) for x in rows[cut[i]:cut[i + 1]]] for i in range(n)]


class MinimizerIndex:
    """The (w, k)-minimizer index of one text, resident on the context's GPU (pwa_mm_create): the text's sketch as (hash, pos) pairs in
    that order, built once, then seeded against by any number of read lists (pwa_mm_seed).  Keeps the text bytes (map_reads cuts its
    windows from them).  k, w; stats = dict(minimizers, build_ms) of the build; close() frees it, and it works as a context manager.
    Close it before its context.  With canonical=True (pwa_mm_create_canonical) a k-mer and its reverse complement share one hash
    and every entry has a strand bit: seed_strands() then finds a read's anchors on both strands from one sketch of the read, and
    seed() is refused; on a plain index it is the other way round."""

    def __init__(self, ctx, text, k, w, canonical=False):
        if not (1 <= k <= 31 and 1 <= w <= 128):
            raise ValueError("MinimizerIndex: k is 1 .. 31 and w is 1 .. 128")
        self._ctx, self._L = ctx, ctx._L
        self.text = _b(text)
        self.k, self.w, self.canonical = k, w, bool(canonical)
        ix = C.c_void_p()
        create = "pwa_mm_create_canonical" if self.canonical else "pwa_mm_create"
        ctx._check(getattr(self._L, create)(ctx._h, self.text, len(self.text), k, w, C.byref(ix)), create)
        self._ix = ix
        n, ms = C.c_uint64(0), C.c_float(0)
        ctx._check(self._L.pwa_mm_last_stats(ix, C.byref(n), C.byref(ms)), "pwa_mm_last_stats")
        self.stats = dict(minimizers=n.value, build_ms=ms.value)
        self.seed_stats = None

    def close(self):
        if getattr(self, "_ix", None):
            self._L.pwa_mm_destroy(self._ix)
            self._ix = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def entries(self):
        """pwa_mm_fetch -> (hash uint64 array, pos uint32 array), in ascending (hash, pos); on a canonical index
        pwa_mm_fetch_canonical -> (hash, pos, strand uint8 array)"""
        import numpy as np
        if not self._ix:
            raise PwaError("MinimizerIndex.entries: the index is closed")
        n = self.stats["minimizers"]
        h, p = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
        if self.canonical:
            s = np.zeros(max(n, 1), dtype=np.uint8)
            self._ctx._check(self._L.pwa_mm_fetch_canonical(self._ix, h.ctypes.data_as(C.POINTER(C.c_uint64)), _u32p(p),
                                                            s.ctypes.data_as(C.POINTER(C.c_uint8)), n), "pwa_mm_fetch_canonical")
            return h[:n], p[:n], s[:n]
        self._ctx._check(self._L.pwa_mm_fetch(self._ix, h.ctypes.data_as(C.POINTER(C.c_uint64)), _u32p(p), n), "pwa_mm_fetch")
        return h[:n], p[:n]

    def seed(self, reads, max_occ=64, as_arrays=False):
        """pwa_mm_seed + pwa_mm_seed_fetch: every read's minimizers looked up among the text's -> what TextIndex.seed returns, per read
        its anchors (t, q, k) by t, then q.  Sets seed_stats = dict(sketch_ms, search_ms, sort_ms, slots, minimizers, hits, ranges)
        here and on the context: device ms of the sketch passes, the lookup kernel and gather + sort + split, the list's k-mers, the
        read minimizers looked up, the hits kept, the ranges of reads the call ran.  ValueError on a canonical index."""
        if self.canonical:
            raise ValueError("MinimizerIndex.seed: the index is canonical; seed_strands() seeds it")
        return self._seed(reads, max_occ, as_arrays, 1)

    def seed_strands(self, reads, max_occ=64, as_arrays=False):
        """pwa_mm_seed_strands + pwa_mm_seed_fetch on a canonical index (ValueError on a plain one): every read sketched once, as
        given, its hits split by strand -> a list of 2 n anchor lists in seed()'s form, entry i read i forward, anchors (t, q, k),
        entry n + i read i reverse, anchors (t, q', k) in the coordinates of revcomp(read i) -- the shape of
        seed(reads + [revcomp(r) for r in reads]) on a plain index, so chain() and chain_top() take it unchanged.  Sets seed_stats as
        seed() does; minimizers counts each read minimizer once, and max_occ counts a minimizer's hits over both strands."""
        if not self.canonical:
            raise ValueError("MinimizerIndex.seed_strands: the index is not canonical; seed() seeds it")
        lists = self._seed(reads, max_occ, as_arrays, 2)
        return lists[0::2] + lists[1::2]

    def _seed(self, reads, max_occ, as_arrays, per):
        """the seeding call with `per` lists per read, in the call's order"""
        import numpy as np
        if max_occ < 1:
            raise ValueError("seed: max_occ is at least 1")
        if not self._ix:
            raise PwaError("MinimizerIndex.seed: the index is closed")
        reads = [_b(r) for r in reads]
        n = len(reads)
        off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum([len(r) for r in reads])
        u64p = C.POINTER(C.c_uint64)
        anc_off = np.zeros(per * n + 1, dtype=np.uint64)
        ck = self._ctx._check
        call = "pwa_mm_seed_strands" if per == 2 else "pwa_mm_seed"
        ck(getattr(self._L, call)(self._ix, b"".join(reads), off.ctypes.data_as(u64p), n, max_occ, anc_off.ctypes.data_as(u64p)), call)
        total = int(anc_off[per * n])
        trip = np.empty((total, 3), dtype=np.uint32)
        t, q = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.uint32)
        ck(self._L.pwa_mm_seed_fetch(self._ix, _u32p(t), _u32p(q), total), "pwa_mm_seed_fetch")
        trip[:, 0], trip[:, 1], trip[:, 2] = t[:total], q[:total], self.k
        km, sm, om = C.c_float(0), C.c_float(0), C.c_float(0)
        ns, nm, nh, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ck(self._L.pwa_mm_seed_last_stats(self._ix, C.byref(km), C.byref(sm), C.byref(om), C.byref(ns), C.byref(nm), C.byref(nh), C.byref(nr)),
           "pwa_mm_seed_last_stats")
        self.seed_stats = self._ctx.seed_stats = dict(sketch_ms=km.value, search_ms=sm.value, sort_ms=om.value, slots=ns.value, minimizers=nm.value,
                                                      hits=nh.value, ranges=nr.value)
        cut = anc_off.astype(np.int64).tolist()
        if as_arrays:
            return [trip[cut[i]:cut[i + 1]] for i in range(per * n)]
        rows = trip.tolist()
        return [[tuple(x) for x in rows[cut[i]:cut[i + 1]]] for i in range(per * n)]


class Batch:
    """Prepared scores-only batch: inputs resident in HBM, run() only enqueues kernels."""

    def __init__(self, ctx, mode, seqs, pair_a, pair_b, match, mismatch, gap, want_end=False, gap_extend=0, gotoh=False, subst=None):
        self._ctx, self._L = ctx, ctx._L
        blob, off, seqs = pack_sequences(seqs)
        self.n_pairs = len(pair_a)
        n = self.n_pairs
        if hasattr(pair_a, "ctypes"):   # numpy uint32 arrays
            pa = pair_a.ctypes.data_as(C.POINTER(C.c_uint32))
            pb = pair_b.ctypes.data_as(C.POINTER(C.c_uint32))
            self._keep = (pair_a, pair_b)
        else:
            pa = (C.c_uint32 * max(n, 1))(*pair_a)
            pb = (C.c_uint32 * max(n, 1))(*pair_b)
        h = C.c_void_p()
        if subst is not None:   # ... under a substitution table (subst_table): the library copies code and matrix during the call
            _code, n_sym, _submat, code_p, submat_p = _subst_args(subst, blob)
            rc = self._L.pwa_subst_batch_create(ctx._h, MODE[mode], code_p, n_sym, submat_p, gap, gap_extend, blob, off, len(seqs), pa, pb, n,
                                                1 if want_end else 0, C.byref(h))
        elif gotoh:   # affine-gap scores of `mode` (nw / sw / sg): gap = gap_open
            rc = self._L.pwa_gotoh_batch_create(ctx._h, MODE[mode], match, mismatch, gap, gap_extend, blob, off, len(seqs), pa, pb, n,
                                                1 if want_end else 0, C.byref(h))
        elif mode == "nwdist":
            rc = self._L.pwa_nwdist_batch_create(ctx._h, match, mismatch, gap, blob, off, len(seqs), pa, pb, n, C.byref(h))
        elif mode == "affine":
            rc = self._L.pwa_affine_batch_create(ctx._h, match, mismatch, gap, gap_extend, blob, off, len(seqs), pa, pb, n,
                                                 C.byref(h))
        else:
            rc = self._L.pwa_batch_create(ctx._h, MODE[mode], match, mismatch, gap, blob, off, len(seqs), pa, pb, n,
                                          1 if want_end else 0, C.byref(h))
        ctx._check(rc, "pwa_batch_create")
        self._h = h
        self.want_end = want_end

    def run(self, stream=None):
        self._ctx._check(self._L.pwa_batch_run(self._h, stream), "pwa_batch_run")

    def d_scores(self):
        return self._L.pwa_batch_d_scores(self._h)

    def set_d_scores(self, device_ptr):
        """Redirect the score vector to caller-owned device memory (e.g. tensor.data_ptr())."""
        self._ctx._check(self._L.pwa_batch_set_d_scores(self._h, device_ptr), "pwa_batch_set_d_scores")

    def last_ms(self):
        ms = C.c_float(0)
        self._ctx._check(self._L.pwa_batch_last_ms(self._h, C.byref(ms)), "pwa_batch_last_ms")
        return ms.value

    def run_times(self, cap=64):
        arr = (C.c_float * cap)()
        n = C.c_int(0)
        self._ctx._check(self._L.pwa_batch_run_times(self._h, arr, cap, C.byref(n)), "pwa_batch_run_times")
        return list(arr[:n.value])

    def info(self):
        cells, padded, nt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        name = C.c_char_p()
        self._L.pwa_batch_info(self._h, C.byref(cells), C.byref(padded), C.byref(nt), C.byref(name))
        return dict(cells=cells.value, padded_cells=padded.value, n_tasks=nt.value, kernel=name.value.decode())

    def cell_bits(self):
        """16: the strips run two pairs per lane in packed f16 cells; 32: int32 cells; 0: no pair on the strips."""
        return self._L.pwa_batch_cell_bits(self._h)

    def profile_form(self):
        """1: the packed f16 strips run in their profile form (one pattern against 128 texts per wave task); 0: otherwise."""
        return self._L.pwa_batch_profile_form(self._h)

    def profile_int(self):
        """1: that profile form runs its integer-coded row step (mismatch >= gap and match >= gap); 0: otherwise."""
        return self._L.pwa_batch_profile_int(self._h)

    def fetch(self, numpy_out=False):
        n = self.n_pairs
        sc = (C.c_int32 * max(n, 1))()
        ei = (C.c_uint32 * max(n, 1))() if self.want_end else None
        ej = (C.c_uint32 * max(n, 1))() if self.want_end else None
        self._ctx._check(self._L.pwa_batch_fetch(self._h, sc, ei, ej), "pwa_batch_fetch")
        if numpy_out:
            import numpy as np
            s = np.ctypeslib.as_array(sc)[:n].copy()
            return (s, np.ctypeslib.as_array(ei)[:n].copy(), np.ctypeslib.as_array(ej)[:n].copy()) if self.want_end else s
        if self.want_end:
            return list(sc[:n]), list(ei[:n]), list(ej[:n])
        return list(sc[:n])

    def fetch_into(self, scores):
        """pwa_batch_fetch straight into a caller-owned C-contiguous numpy int32 array of n_pairs elements."""
        assert scores.dtype.str in ("<i4", "=i4") and scores.flags["C_CONTIGUOUS"] and scores.size == self.n_pairs
        self._ctx._check(self._L.pwa_batch_fetch(self._h, scores.ctypes.data_as(C.POINTER(C.c_int32)), None, None), "pwa_batch_fetch")

    def close(self):
        if getattr(self, "_h", None):
            self._L.pwa_batch_destroy(self._h)
            self._h = None

    __del__ = close
