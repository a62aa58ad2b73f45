// pwalign_align.hip -- alignment batches: pwa_align_batch(_cigar), pwa_align_gotoh_batch(_cigar), pwa_align_subst_batch(_cigar),
// pwa_align_banded_batch(_cigar) and its scores-only form pwa_scores_banded, their substitution-matrix forms
// pwa_align_banded_subst_batch(_cigar) and pwa_scores_banded_subst, the X-drop extension calls pwa_extend_banded_batch(_cigar) and
// pwa_scores_extend_banded with their substitution-matrix forms pwa_extend_banded_subst_batch(_cigar) and
// pwa_scores_extend_banded_subst, pwa_overlaps (the range planner and its stages), pwa_align and
// pwa_align_matrices.
#include "pwalign_internal.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <numeric>

#include "banded_fill.hip.h"
#include "cigar.hip.h"
#include "sufarr_ctx.h"

using namespace pwa;

namespace pwa {
hipError_t cigar_launch(const CigarParams& p, bool write, hipStream_t s);   // cigar_kernels.hip
}

// ------------------------------------------------------------------------- full alignments
// Full alignments of a pair list.  With `ops` the op lists come back (pwa_align_batch); without, only the
// per-pair scores and -- with `overlap_out` -- the overlap lengths computed by the walk itself (pwa_overlaps).
//
// Every pair gets the geometry ITS pattern asks for (r03; hw2.cpp:328-338: the reference's loop has no coupling between
// pairs): patterns of up to 256 rows run on the mini-stripe engine (16 lanes per pair, RL = 4 .. 16 rows per lane: the
// smallest RL that holds the pattern), longer ones on the stripe engine with their own (RL, W).  The list is cut into
// RANGES of consecutive pairs whose bands fit the chunk budget; inside a range the pairs of each class form one launch
// (fill + walk); the device op buffer mirrors the caller's regions of the whole range, so the op lists of all its classes
// come back with one copy.
namespace {
struct TbClass {
    bool mini;
    int rl, w;   // mini: rows per lane (w unused); stripe engine: its PairGeom
    bool banded = false;   // banded_fill.hip.h: one wave per pair (mini, w = 64), stripes of 64 rl rows over a diagonal band
    bool operator==(const TbClass& o) const { return mini == o.mini && rl == o.rl && w == o.w && banded == o.banded; }
};
// pwa_align_batch_cigar: the walks' op lists stay on the device; per range the CIGAR / MD:Z passes (cigar.hip.h) pack the strings and
// only those come back, at the running offsets
struct StrOut {
    char *cigar, *mdz;
    uint64_t cigar_cap, mdz_cap;
    uint64_t *cigar_off, *mdz_off, *needed;
};
// bytes a pair's two strings can take: the range's string buffer is sized by this, and a range's total stays below 2^32 (the scan is 32-bit)
uint64_t str_bound(uint64_t n_plus_m) { return pwa_cigar_bound(n_plus_m) + pwa_mdz_bound(n_plus_m); }
// pwa_align_gotoh_batch(_cigar): affine gaps on the gotoh mini-stripe kernels (the request's gap = gap_open)
struct GotohSpec {
    int gap_open, gap_extend;
};
// pwa_align_subst_batch(_cigar): the gotoh classes with the diagonal score from the caller's table (always beside a GotohSpec); beside a
// BandSpec too: pwa_align_banded_subst_batch(_cigar), pwa_scores_banded_subst; beside an ExtSpec as well: pwa_extend_banded_subst_batch(_cigar),
// pwa_scores_extend_banded_subst
struct SubstSpec {
    SubstRef tab;      // SubstTable::dev and its layout
    int64_t max_abs;   // max |submat|: the range rule's score term
};
constexpr uint64_t kGotohMaxN = 1024;   // patterns of the gotoh classes: 16 x kMiniRL rows, then 64 x 8 | 16 rows
// pwa_align_banded_batch(_cigar): the gotoh cell over a diagonal band per pair (always beside a GotohSpec); patterns of any length
struct BandSpec {
    const int32_t *lo, *hi;   // cell (i, j) of pair k is in the band iff lo[k] <= j - i <= hi[k]
    // the band of pair k clamped to its matrix: -n <= lo, hi <= m.  The same cells -- except for a band that lies wholly outside the
    // matrix (lo > m or hi < -n; valid for SW only), which becomes the corner diagonal m or -n: that adds the boundary cell (0, m) or
    // (n, 0), whose H is 0 and from which no cell is reachable, so the result (score 0, end (0, 0), no ops) is the empty band's
    int64_t lo_in(uint64_t k, uint64_t n, uint64_t m) const { return std::min<int64_t>(std::max<int64_t>(lo[k], -(int64_t)n), (int64_t)m); }
    int64_t hi_in(uint64_t k, uint64_t n, uint64_t m) const { return std::max<int64_t>(std::min<int64_t>(hi[k], (int64_t)m), -(int64_t)n); }
};
// pwa_extend_banded_batch(_cigar), pwa_scores_extend_banded ("EXT"; always beside a BandSpec, mode = PWA_MODE_NW: the matrix, the band
// layout and the walk are NW's): the end is the first row-major maximum with (0, 0), rows are given up xdrop below the best.  The planner
// (TbPlan::class_of / band_of) sizes a pair's band for all n rows: the host cannot know the stop row
struct ExtSpec {
    int xdrop;   // < 0: no row ever stops
};
constexpr int64_t kExtMaxXdrop = 1 << 27;
// Stripe height of a banded pair.  A stripe of S = 64 rl rows over a band of B diagonals runs S + B + 62 steps (+ up to 15 of text
// alignment) of ~F + C rl instructions (F: per-step moves, hand-off and store; C: the masked cell), so its cost per row is
// (S + B + 77) (F + C rl) / S: with F ~ 27 and C ~ 22 the two heights built break even near B = 900, and the share of wasted steps
// (S + 77) / (S + B + 77) falls with B.  Narrow bands take 256-row stripes, wide ones 512-row stripes.
int banded_rl_for(int64_t width) { return width >= 1024 ? 8 : 4; }

// What a call hands back next to the scores: the op lists (pwa_align_batch), the strings the device formats from them
// (pwa_align_batch_cigar), the overlap lengths the walk computes itself (pwa_overlaps), or nothing: scores and end cells of a banded
// list (pwa_scores_banded), whose launches write no band and run no walk
enum AlignOutMode { OUT_OPS, OUT_STRINGS, OUT_OVERLAP, OUT_SCORES };
struct AlignOut {
    AlignOutMode mode = OUT_OPS;
    int32_t* score = nullptr;
    uint64_t *end_cells = nullptr, *start_cells = nullptr;   // 2 * n_pairs each, or null
    uint8_t* ops = nullptr;                                  // OUT_OPS
    const uint64_t* ops_off = nullptr;
    uint64_t* n_ops = nullptr;
    int32_t* overlap = nullptr;                              // OUT_OVERLAP
    StrOut str = {};                                         // OUT_STRINGS
    uint32_t *end_i = nullptr, *end_j = nullptr;             // OUT_SCORES: n_pairs each, or null
    uint32_t* rows = nullptr;                                // EXT: rows considered per pair (n_pairs), or null
    int32_t* pend_score = nullptr;                           // EXT with a table: the pattern-end result per pair (n_pairs each), or null
    uint32_t* pend_j = nullptr;
    // the EXT calls' additions to any of the three below
    AlignOut& ext(uint32_t* r, int32_t* ps = nullptr, uint32_t* pj = nullptr) { return rows = r, pend_score = ps, pend_j = pj, *this; }
};
AlignOut out_ops(int32_t* score, uint64_t* end_cells, uint64_t* start_cells, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops) {
    return AlignOut{OUT_OPS, score, end_cells, start_cells, ops, ops_off, n_ops};
}
AlignOut out_strings(int32_t* score, uint64_t* end_cells, uint64_t* start_cells, const StrOut& str) {
    AlignOut o{OUT_STRINGS, score, end_cells, start_cells};
    o.str = str;
    return o;
}
AlignOut out_scores(int32_t* score, uint32_t* end_i, uint32_t* end_j) {
    AlignOut o{OUT_SCORES, score};
    o.end_i = end_i, o.end_j = end_j;
    return o;
}
// The caller's scoring, sequences, pair list and outputs, as the stages of align_batch_impl see them
struct AlignRequest {
    int mode, match, mismatch, gap;
    const GotohSpec* gt;   // null: linear gaps
    const SubstSpec* sb;   // null: match / mismatch on raw bytes
    const uint8_t* seq_bytes;
    const uint64_t* seq_off;
    uint32_t n_seq;
    const uint32_t *pair_a, *pair_b;
    uint64_t n_pairs;
    AlignOut out;
    const BandSpec* bd = nullptr;   // null: the whole matrix
    const ExtSpec* ext = nullptr;   // EXT: extension from (0, 0) with an X-drop, else null
    uint64_t slen(uint32_t s) const { return seq_off[s + 1] - seq_off[s]; }
    bool local() const { return mode == PWA_MODE_SW; }
    bool semi() const { return mode == PWA_MODE_SG; }   // (semi-global: NW's classes, guards and codes; no gap shift)
    bool want_ops() const { return out.mode == OUT_OPS; }
    bool want_str() const { return out.mode == OUT_STRINGS; }
    bool scores_only() const { return out.mode == OUT_SCORES; }   // no band, no walk, no ops (walk_ops() only says: not pwa_overlaps)
    bool walk_ops() const { return out.mode != OUT_OVERLAP; }   // WALK_OPS; the op lists come back (want_ops) or are formatted on the device (want_str)
    // the EXT calls with a table also return the pattern-end result: a {score, j} record per pair travels behind the range's PairResults
    bool pend() const { return ext && sb; }
    size_t res_bytes() const { return sizeof(PairResult) + (pend() ? 2 * sizeof(int32_t) : 0); }
};
// ... as an entry point has them: scoring (gap: the linear gap, or gap_open), sequences, pair list, outputs; no spec yet
AlignRequest request(int mode, int match, int mismatch, int gap, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a,
                     const uint32_t* pair_b, uint64_t n_pairs, const AlignOut& out) {
    return AlignRequest{mode, match, mismatch, gap, nullptr, nullptr, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out};
}

// PWA_DEBUG: host-side time between marks
struct AlignClock {
    bool on;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pwa] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};

int validate_align(pwa_ctx* ctx, const AlignRequest& rq) {
    const AlignOut& o = rq.out;
    // (pwa_overlaps is hw2 -g's selection over global or local alignments: no semi-global form)
    if (rq.mode != PWA_MODE_NW && rq.mode != PWA_MODE_SW && (rq.mode != PWA_MODE_SG || !rq.walk_ops())) return fail(ctx, PWA_E_INVALID, "unknown mode");
    if (!rq.seq_off || !o.score || (rq.want_ops() && (!o.ops_off || !o.n_ops)) || (!rq.walk_ops() && !o.overlap) ||
        (rq.want_str() && (!o.str.cigar_off || !o.str.mdz_off || (o.str.cigar_cap && !o.str.cigar) || (o.str.mdz_cap && !o.str.mdz))) ||
        (rq.n_pairs && (!rq.pair_a || !rq.pair_b)))
        return fail(ctx, PWA_E_INVALID, "null input");
    if (rq.ext && (int64_t)rq.ext->xdrop > kExtMaxXdrop) return fail(ctx, PWA_E_INVALID, "EXT: xdrop must be at most 2^27 (negative: no row stops)");
    const int rc = check_pair_list(ctx, rq.pair_a, rq.pair_b, rq.n_pairs, rq.n_seq);
    if (rc != PWA_OK || !rq.gt) return rc;
    // the gotoh classes' shape limit, and the range every key of theirs stays exact in
    const int64_t gaps = (int64_t)std::llabs((long long)rq.gt->gap_open) + std::llabs((long long)rq.gt->gap_extend);
    const int64_t mx = rq.sb ? std::max(rq.sb->max_abs, gaps) : max_abs({rq.match, rq.mismatch, gaps});
    for (uint64_t k = 0; k < rq.n_pairs; ++k) {
        const uint64_t n = rq.slen(rq.pair_a[k]), m = rq.slen(rq.pair_b[k]);
        if (rq.bd) {   // the band's validity per mode (include/pwalign.h), its width, then the range rule (an all-zero scoring counts as 1)
            const int64_t lo = rq.bd->lo[k], hi = rq.bd->hi[k], d = (int64_t)m - (int64_t)n;
            if (lo > hi) return fail(ctx, PWA_E_INVALID, "banded alignment: band_lo > band_hi");
            if (rq.ext && !(lo <= 0 && 0 <= hi)) return fail(ctx, PWA_E_INVALID, "banded EXT alignment: the band must hold the anchor, band_lo <= 0 <= band_hi");
            if (!rq.ext && rq.mode == PWA_MODE_NW && !(lo <= 0 && 0 <= hi && lo <= d && d <= hi))
                return fail(ctx, PWA_E_INVALID, "banded NW alignment: the band must hold the diagonals 0 and m - n");
            if (rq.mode == PWA_MODE_SG && !(hi >= 0 && (int64_t)n + lo <= (int64_t)m))
                return fail(ctx, PWA_E_INVALID, "banded SG alignment: needs band_hi >= 0 and n + band_lo <= m");
            if (hi - lo + 1 > (int64_t)kBandedMaxWidth) return fail(ctx, PWA_E_CAPACITY, "banded alignment: band wider than 4096 diagonals");
            // (EXT: one bit tighter -- its row keys hold H * 16 with H of either sign, banded_fill.hip.h)
            if (rq.ext && (n > 0x7fffffc0ull || m > 0x7fffffc0ull || (long double)(n + m + 2) * (long double)std::max<int64_t>(mx, 1) >= (long double)(1u << 27)))
                return fail(ctx, PWA_E_CAPACITY, rq.sb ? "EXT scores out of range: (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|, 1) must stay below 2^27"
                                                       : "EXT scores out of range: (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|, 1) must stay below 2^27");
            if (n > 0x7fffffc0ull || m > 0x7fffffc0ull || (long double)(n + m + 2) * (long double)std::max<int64_t>(mx, 1) >= (long double)(1u << 28))
                return fail(ctx, PWA_E_CAPACITY, rq.sb ? "substitution-matrix scores out of range: (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|, 1) must stay below 2^28"
                                                       : "gotoh scores out of range: (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|) must stay below 2^28");
            continue;
        }
        if (n > kGotohMaxN) return fail(ctx, PWA_E_CAPACITY, "gotoh alignments take patterns of at most 1024 symbols");
        if (rq.sb && (m > 0x7fffffc0ull || (long double)(n + m + 2) * (long double)mx >= (long double)(1u << 28)))
            return fail(ctx, PWA_E_CAPACITY, "substitution-matrix scores out of range: (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|) must stay below 2^28");
        if (m > 0x7fffffc0ull || (long double)(n + m + 2) * (long double)mx >= (long double)(1u << 28))
            return fail(ctx, PWA_E_CAPACITY, "gotoh scores out of range: (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|) must stay below 2^28");
    }
    return PWA_OK;
}

// The device arena of the used sequences (raw bytes, or codes for alphabets of at most 7 symbols: code_alphabet) and what the scan of
// their bytes found
struct AlignArena {
    std::vector<uint64_t> aoff;
    bool seen[256];
    uint8_t code_of[256];
    bool coded = false;
    int32_t dash_sym = 0x100;
    Lease arena;
    uint8_t* base() const { return arena.as<uint8_t>(); }
};
int build_align_arena(pwa_ctx* ctx, const AlignRequest& rq, AlignClock& clock, AlignArena& ar) {
    std::vector<uint8_t> is_used(rq.n_seq, 0);
    for (uint64_t k = 0; k < rq.n_pairs; ++k) is_used[rq.pair_a[k]] = is_used[rq.pair_b[k]] = 1;
    const uint64_t arena_bytes = layout_arena(rq.seq_off, rq.n_seq, is_used, 256, ar.aoff);
    // one pass over every used byte, on a few threads once the input reaches megabytes
    scan_bytes(rq.seq_bytes, rq.seq_off, rq.n_seq, is_used, ar.seen, 1ull << 20);
    ar.coded = !rq.gt && code_alphabet(ar.seen, ar.code_of, rq.match, rq.mismatch, rq.gap, ctx->knobs);   // (gotoh: raw bytes, compared)
    const bool dash_seen = ar.seen[(unsigned char)'-'], nul_seen = ar.seen[0];
    // overlapLongestExactMatch (hw2.cpp:269) does not count a column whose symbols are '-' -- also when the '-' is part
    // of the input sequence itself: the walk needs the arena's value for that byte
    ar.dash_sym = !dash_seen ? 0x100 : (ar.coded ? (int32_t)ar.code_of[(unsigned char)'-'] : (int32_t)'-');
    clock.mark("validate + alphabet scan");
    HIPC(ctx, workspace(ctx, DevMem::ARENA, arena_bytes, ar.arena));
    HIPC(ctx, build_arena(ctx, ar.base(), arena_bytes, rq.seq_bytes, rq.seq_off, rq.n_seq, is_used, ar.aoff, ar.coded ? ar.code_of : nullptr, !nul_seen));
    clock.mark("arena upload");
    return PWA_OK;
}

// The mini-stripe engine exists for keyed cells with table scoring; PWA_FORCE_RL / PWA_FORCE_W address the stripe engine.  (n_plus_m: the
// call's longest pair; local: the first-maximum records hold H * 16)
bool mini_eligible(const Knobs& kn, bool coded, bool keyed, bool local, uint64_t n_plus_m, int match, int mismatch, int gap) {
    return coded && keyed && kn.tb_engine != 0 && !kn.force_rl && !kn.force_w && (!local || tb_range_ok(n_plus_m, match, mismatch, gap, 26));
}

// Everything that decides a pair's class and band, from the call's lengths, scores and switches alone (no device, no context)
struct TbPlan {
    const Knobs* kn;
    bool gotoh;
    bool sband;          // the fills also write the int32 score band (the gotoh kernels write none)
    bool keyed, gap0;    // cell form of the fills; k_*: the scores their kernels are given
    int k_match, k_mismatch, k_gap;
    bool mini_ok, wide_ok, tall_stripes;
    const AlignRequest* banded = nullptr;   // the banded call's request (its BandSpec and lengths), else null
    bool scores = false;                    // ... and it is pwa_scores_banded: no pair has a band or op bytes
    uint64_t band_mult() const { return sband ? 5 : 1; }   // band bytes in HBM per byte of codes
    // (k: the pair's index in the call's list; only the banded class looks at it -- its stripe height follows the pair's band width)
    TbClass class_of(uint64_t n, uint64_t k = 0) const {   // (w of a mini class = its lanes per pair)
        if (banded) {
            const uint64_t m = banded->slen(banded->pair_b[k]);
            return TbClass{true, kn->banded_rl ? kn->banded_rl : banded_rl_for(banded->bd->hi_in(k, n, m) - banded->bd->lo_in(k, n, m) + 1), 64, true};
        }
        if (gotoh) return n <= 256 ? TbClass{true, mini_rl_for(n), 16} : TbClass{true, n <= 512 ? 8 : 16, 64};
        if (mini_ok && n <= 256) return TbClass{true, mini_rl_for(n), 16};
        if (wide_ok && n <= 1024) return TbClass{true, wide_rl_for(n), 64};
        PairGeom g = choose_geom(*kn, n, keyed, true);
        if (tall_stripes && g.rl == 2 && g.w == 4) g.rl = 4;
        return TbClass{false, g.rl, g.w};
    }
    // band bytes of a pair: the stripe engine's own (also the one-pair-per-wave form's: a single stripe of 64 RL rows); the four-pair
    // mini-stripe form's for a text of m_task columns (its task's longest)
    // (the banded class: stripes x pitch x 64 rl -- from n, the band width and the stripe height; m only clips the widest window)
    uint64_t band_of(const TbClass& c, uint64_t n, uint64_t m_task, uint64_t k = 0) const {
        if (scores) return 0;
        if (c.banded) {
            const int64_t S = 64 * c.rl, B = banded->bd->hi_in(k, n, m_task) - banded->bd->lo_in(k, n, m_task) + 1;
            return (uint64_t)(((int64_t)n + S - 1) / S * banded_steps(S, B, (int64_t)m_task) * S);
        }
        if (c.mini && c.w == 16) return (uint64_t)mini_band_steps(m_task) * 16 * (uint64_t)c.rl;
        if (c.mini) return (uint64_t)band_steps(m_task) * 64 * (uint64_t)c.rl;
        return ::tb_band_bytes(n, m_task, c.rl);
    }
};
TbPlan make_tb_plan(const AlignRequest& rq, const Knobs& kn, bool coded, bool score_band) {
    const bool local = rq.local();
    const int match = rq.match, mismatch = rq.mismatch, gap = rq.gap;
    TbPlan pl;
    pl.kn = &kn;
    pl.gotoh = rq.gt != nullptr;
    pl.banded = rq.bd ? &rq : nullptr;
    pl.scores = rq.scores_only();
    pl.sband = score_band && !rq.gt;
    uint64_t longest_sum = 0;
    for (uint64_t k = 0; k < rq.n_pairs; ++k) longest_sum = std::max(longest_sum, rq.slen(rq.pair_a[k]) + rq.slen(rq.pair_b[k]));
    // scores x lengths beyond the packed keys' 2^28: the plain int32 form, exact for anything the reference's int holds
    pl.keyed = tb_range_ok(longest_sum, match, mismatch, gap, local ? 26 : 28) && !kn.no_keyed_tb;   // (local: H * 16 in the first-maximum records)
    // Global alignments with table scoring run in gap-shifted coordinates G = H - gap (i + j): the same recurrence with gap 0 and
    // scores s - 2 gap, identical comparisons and codes, one instruction less per cell (pair_fill.hip.h, GAP0: gap0_ok)
    pl.gap0 = !rq.gt && !local && !rq.semi() && coded && pl.keyed && !score_band && !kn.no_gap_shift && gap0_ok(longest_sum, match, mismatch, gap);
    pl.k_match = pl.gap0 ? match - 2 * gap : match;
    pl.k_mismatch = pl.gap0 ? mismatch - 2 * gap : mismatch;
    pl.k_gap = pl.gap0 ? 0 : gap;
    pl.mini_ok = mini_eligible(kn, coded, pl.keyed, local, longest_sum, match, mismatch, gap);
    // patterns of 257 .. 1024 rows: ONE wave per pair (mini-stripe kernels with 64 lanes per pair, RL = 8 | 16) instead of 4 - 8 pipelined
    // stripes -- when the call has enough of them to occupy the chip that way (a few such pairs are faster spread over more waves)
    uint64_t n_mid = 0;
    for (uint64_t k = 0; k < rq.n_pairs; ++k) {
        const uint64_t n = rq.slen(rq.pair_a[k]);
        n_mid += n > 256 && n <= 1024 && rq.slen(rq.pair_b[k]) > 0;
    }
    pl.wide_ok = pl.mini_ok && (n_mid >= 256 || kn.tb_engine == 2);
    // the stripe engine's pairs: RL = 2 gives ONE pair more waves in flight (10 % at 10k x 10k), but a list whose stripes fill the chip anyway
    // runs faster on fewer, taller ones -- [gpu, r03] fills at RL = 2 / RL = 4, NW: 16 pairs 10k x 10k 1.90 / 1.22 ms, 64 pairs 4.12 / 3.33,
    // 256 pairs 12.8 / 8.7, 512 pairs 2000 x 2000 1.07 / 0.75, 32 pairs 30k x 30k 18.0 / 12.4 (profiles/r03_align_shapes.txt)
    uint64_t stripes2 = 0;
    for (uint64_t k = 0; k < rq.n_pairs; ++k) {
        const uint64_t n = rq.slen(rq.pair_a[k]);
        if (!rq.slen(rq.pair_b[k]) || n > 0x7fffffc0ull || (pl.mini_ok && n <= 256) || (pl.wide_ok && n <= 1024)) continue;
        stripes2 += (n + 127) / 128;
    }
    pl.tall_stripes = stripes2 >= 1024 && !kn.force_rl;
    return pl;
}

// How much a range may hold.  A range's band is written once and read along one path per pair, so nothing is gained by a huge one, and
// hipMalloc gets slow for very large requests ([gpu] profiles/r01_malloc_probe.txt: 0.3 ms up to 8 GiB, 0.24 s for 10.5 GB, > 1 s for
// 16 GiB): a list that fits 8 GiB of band (x 5 with the int32 score band) and op bytes, or 80 % of the free HBM if that is less, is one
// range.  But a range is a launch of its own, and a launch takes at least the time ONE wave needs for its longest pair ([gpu, r03] 1.3 ms
// for a 10k-column text on the mini-stripe engine, whatever the number of pairs): so a range should hold ~8192 pairs where the list has
// them (2048+ waves) and may use up to 48 GiB for that (PWA_RANGE_BYTES: that many; the workspace is kept in the context, the slow
// hipMalloc is paid once), and a list that needs several ranges is cut into EQUAL ones, not into full ones and a remainder.
struct RangeTarget {
    uint64_t chunk_target;   // band (x band_mult) + op bytes of a range
    uint64_t pairs_target;   // live pairs of a range, when the list is cut into several
};
RangeTarget range_target(const AlignRequest& rq, const TbPlan& plan, uint64_t budget) {
    RangeTarget t{std::min<uint64_t>(budget, 8ull << 30), ~0ull};
    uint64_t total = 0, live = 0;
    for (uint64_t k = 0; k < rq.n_pairs; ++k) {
        const uint64_t n = rq.slen(rq.pair_a[k]), m = rq.slen(rq.pair_b[k]);
        if (!(n && m) || n > 0x7fffffc0ull || m > 0x7fffffc0ull) continue;
        total += align_up(plan.band_of(plan.class_of(n, k), n, m, k), 256) * plan.band_mult() + (plan.scores ? 0 : align_up(n + m + 1, 16));
        ++live;
    }
    if (!live) return t;
    const uint64_t cap = plan.kn->range_bytes ? plan.kn->range_bytes : std::min<uint64_t>(budget, 48ull << 30);
    const uint64_t for_8192 = (uint64_t)((long double)total / (long double)live * 8192.0L);
    t.chunk_target = std::min<uint64_t>(cap, std::max<uint64_t>(t.chunk_target, for_8192));
    const uint64_t n_ranges = (total + t.chunk_target - 1) / t.chunk_target;
    if (n_ranges > 1) {
        t.chunk_target = std::min<uint64_t>(cap, total / n_ranges + total / live + (1ull << 20));   // equal shares (+ one average pair)
        // ... counted in PAIRS, in whole rounds of the chip: a launch lasts as long as its busiest wave, and 8193 pairs are 2049
        // tasks for 2048 wave slots -- [gpu, r03] 16 384 pairs 150 x 10k cut 8193 + 8191: the first fill took 4.1 ms, the second 3.0
        t.pairs_target = (live + n_ranges - 1) / n_ranges;
        if (t.pairs_target > 4096) t.pairs_target = (t.pairs_target + 4095) / 4096 * 4096;   // 1024 waves of four pairs (or 4 x 1024 of one)
        const uint64_t fit = cap / std::max<uint64_t>(total / live, 1);
        if (t.pairs_target > fit) t.pairs_target = std::max<uint64_t>(fit / 4096 * 4096, std::min<uint64_t>(fit, 4096));
        t.chunk_target = std::min<uint64_t>(cap, std::max<uint64_t>(t.chunk_target, (uint64_t)((long double)total / (long double)live * (long double)t.pairs_target * 1.02L)));
    }
    return t;
}

struct Launch {                    // the pairs of one class inside one range
    TbClass cls;
    std::vector<uint32_t> q;       // pair index inside the range, in launch order (mini: longest text first)
    std::vector<uint64_t> bo;      // band offset of each (bytes; the int32 score band uses the same offsets in elements)
    std::vector<uint64_t> mt;      // mini: the text length the pair's band is sized for (its task's longest)
    uint64_t dummy_bo[3] = {0, 0, 0};
    uint32_t n_dummy = 0;
};
struct Range {
    uint64_t k0, k1, band, opsb, strb;   // strb: string bound of the range (pwa_align_batch_cigar)
    bool tiled;      // the caller's op regions ops_off[k] .. + n_k + m_k of the range's pairs follow one another without a gap:
    uint64_t span;   // the device op buffer then mirrors that range and comes back with ONE copy, straight into `ops`
    std::vector<Launch> launches;
};
// The ranges of a call, the sizes of the workspaces that serve the largest of them -- or why the list cannot be planned
struct RangePlan {
    std::vector<Range> ranges;
    uint64_t band_cap = 0, ops_cap_b = 0, nc_cap = 0, str_cap = 0;
    int err = PWA_OK;
    const char* msg = nullptr;
};

// The launches of the range rg.k0 .. rg.k1: one per class present, pairs in caller order (mini: by text length, so that the four pairs of
// a wave run about the same number of steps; the band of each is sized for its task's longest text); their bands one behind the other
void lay_out_launches(const AlignRequest& rq, const TbPlan& plan, Range& rg) {
    const uint64_t k0 = rg.k0;
    for (uint64_t k = k0; k < rg.k1; ++k) {
        const uint64_t n = rq.slen(rq.pair_a[k]), m = rq.slen(rq.pair_b[k]);
        if (!(n && m)) continue;
        const TbClass c = plan.class_of(n, k);
        size_t li = 0;
        while (li < rg.launches.size() && !(rg.launches[li].cls == c)) ++li;
        if (li == rg.launches.size()) {
            rg.launches.emplace_back();
            rg.launches.back().cls = c;
        }
        rg.launches[li].q.push_back((uint32_t)(k - k0));
    }
    uint64_t bo = 0;
    for (Launch& L : rg.launches) {
        const size_t np = L.q.size();
        L.bo.resize(np);
        if (L.cls.mini) {
            const size_t ppw = (size_t)(64 / L.cls.w);
            sort_by_length_desc(L.q, [&](uint32_t x) { return rq.slen(rq.pair_b[k0 + x]); });
            L.mt.resize(np);
            for (size_t p = 0; p < np; ++p) L.mt[p] = rq.slen(rq.pair_b[k0 + L.q[p / ppw * ppw]]);   // the task's first pair has its longest text
            L.n_dummy = (uint32_t)((ppw - np % ppw) % ppw);
        }
        for (size_t p = 0; p < np; ++p) {
            L.bo[p] = bo;
            bo += align_up(plan.band_of(L.cls, rq.slen(rq.pair_a[k0 + L.q[p]]), L.cls.mini ? L.mt[p] : rq.slen(rq.pair_b[k0 + L.q[p]]), k0 + L.q[p]), 256);
        }
        for (uint32_t d = 0; d < L.n_dummy; ++d) {   // the last task's empty patterns write their padding here
            L.dummy_bo[d] = bo;
            bo += align_up(plan.band_of(L.cls, 0, L.mt[np - 1]), 256);
        }
    }
    rg.band = bo;
}

// Ranges of consecutive pairs whose traceback bands fit the target (a single pair: whatever it needs, if the free HBM holds it).
// A scores-only list has neither band nor op bytes: nothing here cuts it (its arena is built whole before the ranges are planned).
RangePlan plan_ranges(const AlignRequest& rq, const TbPlan& plan, const RangeTarget& target, uint64_t budget, uint64_t free_b) {
    RangePlan rp;
    auto stop = [&rp](int code, const char* msg) -> RangePlan& {
        rp.err = code;
        rp.msg = msg;
        return rp;
    };
    const bool want_ops = rq.want_ops(), want_str = rq.want_str(), scores = rq.scores_only();
    const uint64_t band_mult = plan.band_mult();
    for (uint64_t k0 = 0; k0 < rq.n_pairs;) {
        uint64_t k1 = k0, est = 0, opsb = 0, live_in = 0, strb = 0;
        while (k1 < rq.n_pairs) {
            const uint64_t n = rq.slen(rq.pair_a[k1]), m = rq.slen(rq.pair_b[k1]);
            if (n > 0x7fffffc0ull || m > 0x7fffffc0ull) return stop(PWA_E_CAPACITY, "sequence longer than 2^31");
            const uint64_t need = (n && m) ? align_up(plan.band_of(plan.class_of(n, k1), n, m, k1), 256) : 0;
            const uint64_t sneed = want_str ? str_bound(n + m) : 0;
            if (sneed > 0xffffffffull) return stop(PWA_E_CAPACITY, "strings of one pair may exceed 2^32 bytes");
            if (k1 > k0 && !scores && ((est + need) * band_mult + opsb + n + m > target.chunk_target || (need && live_in >= target.pairs_target) ||
                            strb + sneed > 0xffffffffull))
                break;
            live_in += need != 0;
            est += need;
            opsb += scores ? 0 : align_up(n + m + 1, 16);
            strb += sneed;
            ++k1;
        }
        Range rg{k0, k1, 0, opsb, strb, want_ops, 0, {}};
        lay_out_launches(rq, plan, rg);
        if (rg.band * band_mult + opsb > budget && rg.band + opsb > (uint64_t)(free_b * 0.97))
            return stop(PWA_E_NOMEM, "traceback band of a single pair exceeds free HBM");
        if (want_ops) {
            for (uint64_t k = k0; k < k1; ++k) {
                const uint64_t cap = rq.slen(rq.pair_a[k]) + rq.slen(rq.pair_b[k]);
                if (k + 1 < k1 && rq.out.ops_off[k + 1] != rq.out.ops_off[k] + cap) rg.tiled = false;
                rg.span += cap;
            }
            if (plan.kn->no_tiled_ops) rg.tiled = false;
        }
        rp.band_cap = std::max(rp.band_cap, rg.band);
        rp.ops_cap_b = std::max(rp.ops_cap_b, std::max(opsb, rg.tiled ? rg.span + 16 : 0));
        rp.nc_cap = std::max(rp.nc_cap, k1 - k0);
        rp.str_cap = std::max(rp.str_cap, rg.strb);
        rp.ranges.push_back(std::move(rg));
        k0 = k1;
    }
    return rp;
}

// The device workspaces of a call, sized for its largest range and kept in the context between calls
struct AlignWorkspaces {
    Lease band, sband, d_ops, d_res, str, aux;
    // pwa_align_batch_cigar's device side per range (aux): the pair list, the 2 nc + 2 string lengths (then offsets), the scan's partials
    uint64_t aux_len_at = 0, aux_part_at = 0;
    uint8_t* ops() const { return d_ops.as<uint8_t>(); }
    PairResult* res() const { return d_res.as<PairResult>(); }
};
int take_align_workspaces(pwa_ctx* ctx, const AlignRequest& rq, const TbPlan& plan, const RangePlan& rp, AlignWorkspaces& ws) {
    const uint64_t len_words = 2 * rp.nc_cap + 2;
    ws.aux_len_at = rp.nc_cap * sizeof(CigarPair);
    ws.aux_part_at = ws.aux_len_at + align_up(len_words * 4, 256);
    if (rp.ranges.empty()) return PWA_OK;
    // + one traceback window: the walk stages whole windows
    if (!rq.scores_only()) HIPC(ctx, workspace(ctx, DevMem::BAND, rp.band_cap + 32768, ws.band));
    if (plan.sband) HIPC(ctx, workspace(ctx, DevMem::SBAND, rp.band_cap * sizeof(int32_t), ws.sband));
    HIPC(ctx, workspace(ctx, DevMem::OPS, rq.walk_ops() && !rq.scores_only() ? rp.ops_cap_b : 16, ws.d_ops));
    HIPC(ctx, workspace(ctx, DevMem::RES, rp.nc_cap * rq.res_bytes(), ws.d_res));
    if (rq.want_str()) {
        HIPC(ctx, workspace(ctx, DevMem::STR, rp.str_cap, ws.str));
        HIPC(ctx, workspace(ctx, DevMem::STR_AUX, ws.aux_part_at + pwa::scan_part_words(len_words) * 4, ws.aux));
    }
    return PWA_OK;
}

// Host side of the range in flight (the page-locked result and string records, each pair's offset in the device op buffer) and what the
// ranges before it left
struct RangeHost {
    PairResult* res = nullptr;     // uploaded, and read back after the walk
    int32_t* pend = nullptr;       // AlignRequest::pend(): the range's {score, j} records, behind its results on the host and on the device
    CigarPair* cpairs = nullptr;   // pwa_align_batch_cigar: the range's pair list, then (same page-locked buffer) its string offsets
    uint32_t* clen = nullptr;
    std::vector<uint64_t> ooff;
    uint64_t ops_lo = 0;             // tiled: the caller's op offset of the range's first pair
    std::vector<uint8_t> host_ops;   // staging, only for ranges whose op regions do not tile
    uint64_t str_at[2] = {0, 0};     // pwa_align_batch_cigar: bytes of CIGAR / MD:Z so far (the output offsets of the next range)
    float fmt_ms[2] = {0.f, 0.f};    // ... and the device ms of its two passes
};

// The range's result records: zeros, or the whole answer of a pair with an empty side; on the device before the first launch
int init_range_results(pwa_ctx* ctx, const AlignRequest& rq, const AlignArena& ar, const AlignWorkspaces& ws, const Range& rg, RangeHost& rh) {
    const uint64_t k0 = rg.k0, nc = rg.k1 - rg.k0;
    const bool local = rq.local(), semi = rq.semi(), want_ops = rq.want_ops(), want_str = rq.want_str();
    HIPC(ctx, ctx->pin[pwa_ctx::PIN_RES].reserve(nc * rq.res_bytes()));
    PairResult* const res = rh.res = ctx->pin[pwa_ctx::PIN_RES].as<PairResult>();
    rh.pend = rq.pend() ? reinterpret_cast<int32_t*>(res + nc) : nullptr;
    if (want_str) {
        HIPC(ctx, ctx->pin[pwa_ctx::PIN_STR].reserve(nc * sizeof(CigarPair) + (2 * nc + 2) * 4));
        rh.cpairs = ctx->pin[pwa_ctx::PIN_STR].as<CigarPair>();
        rh.clen = reinterpret_cast<uint32_t*>(rh.cpairs + nc);
    }
    rh.ooff.resize(nc);
    uint64_t oo = 0;
    rh.ops_lo = (want_ops && nc) ? rq.out.ops_off[k0] : 0;
    if (want_ops && !rg.tiled) rh.host_ops.resize(rg.opsb);
    for (uint64_t q = 0; q < nc; ++q) {
        const uint64_t k = k0 + q, n = rq.slen(rq.pair_a[k]), m = rq.slen(rq.pair_b[k]);
        std::memset(&res[q], 0, sizeof(PairResult));
        rh.ooff[q] = rg.tiled ? rq.out.ops_off[k] - rh.ops_lo : oo;
        if (!(n && m) && !local && !rq.ext) {   // (semi-global: column 0, or nothing for an empty pattern; EXT: score 0 at (0, 0))
            res[q].score = wrap_mul((int64_t)(semi ? n : n + m), rq.gap);
            if (rq.gt) {   // one gap of length L: gap_open + L * gap_extend
                const uint64_t L = semi ? n : n + m;
                res[q].score = L ? (int32_t)((uint32_t)rq.gt->gap_open + (uint32_t)wrap_mul((int64_t)L, rq.gt->gap_extend)) : 0;
            }
            res[q].end_i = (uint32_t)n;
            res[q].end_j = semi ? 0u : (uint32_t)m;
        }
        if (rh.pend) {   // what the host reads when the kernel writes nothing: no value -- or, for an empty pattern, the anchor itself
            rh.pend[2 * q] = n ? PWA_EXT_NO_PEND : 0;
            rh.pend[2 * q + 1] = 0;
        }
        if (want_str) rh.cpairs[q] = CigarPair{ar.aoff[rq.pair_a[k]], ar.aoff[rq.pair_b[k]], rh.ooff[q], (uint32_t)n, (uint32_t)m};
        oo += align_up(n + m + 1, 16);
    }
    HIPC(ctx, hipMemcpy(ws.res(), res, nc * rq.res_bytes(), hipMemcpyHostToDevice));
    if (want_str) HIPC(ctx, hipMemcpyAsync(ws.aux.get(), rh.cpairs, nc * sizeof(CigarPair), hipMemcpyHostToDevice, ctx->stream));
    return PWA_OK;
}

// Cells (i, j) of an n x m matrix, 1 <= i <= n, 1 <= j <= m, with lo <= j - i <= hi: what a banded fill computes
uint64_t banded_cells(int64_t n, int64_t m, int64_t lo, int64_t hi) {
    uint64_t cells = 0;
    for (int64_t d = std::max(lo, 1 - n); d <= std::min(hi, m - 1); ++d) cells += (uint64_t)(d >= 0 ? std::min(n, m - d) : std::min(n + d, m));
    return cells;
}

// One launch of the banded class: the descriptors carry the clamped band, the band pitch and the stripe count; the request and the
// class make one BandedForm, whose kernels pwa::banded_launch (pwalign_ctx.hip) resolves, sizes the grid for and launches -- fill +
// walk, or for a scores-only request the score pass alone over the same descriptors without band and op regions --; the device times
// (and a scores-only request's in-band cells) into `stats`.  EXT with a table: PairDesc::rows (unused by the banded class otherwise)
// points at the pair's pattern-end record
int run_banded_launch(pwa_ctx* ctx, const AlignRequest& rq, const AlignArena& ar, const AlignWorkspaces& ws, const Range& rg, const Launch& L,
                      const RangeHost& rh, AlignStats& stats, AlignClock& clock) {
    const size_t np = L.q.size();
    const int64_t S = 64 * L.cls.rl;
    const bool scores = rq.scores_only();
    std::vector<PairDesc> pd(np);
    int64_t row_cap = 1;
    for (size_t p = 0; p < np; ++p) {
        const uint64_t q = L.q[p], k = rg.k0 + q, n = rq.slen(rq.pair_a[k]), m = rq.slen(rq.pair_b[k]);
        const int64_t lo = rq.bd->lo_in(k, n, m), hi = rq.bd->hi_in(k, n, m);
        PairDesc& d = pd[p];
        std::memset(&d, 0, sizeof d);
        d.pat = ar.base() + ar.aoff[rq.pair_a[k]];
        d.txt = ar.base() + ar.aoff[rq.pair_b[k]];
        d.n = (int32_t)n;
        d.m = (int32_t)m;
        d.tb = scores ? nullptr : ws.band.as<uint8_t>() + L.bo[p];
        d.res = ws.res() + q;
        if (rq.pend()) d.rows = reinterpret_cast<int32_t*>(ws.res() + (rg.k1 - rg.k0)) + 2 * q;
        d.ops = scores ? nullptr : ws.ops() + rh.ooff[q];
        d.ops_cap = (uint32_t)std::min<uint64_t>(n + m, 0xffffffffu);
        d.n_stripes = (uint32_t)(((int64_t)n + S - 1) / S);
        d.row_stride = (uint32_t)banded_steps(S, hi - lo + 1, (int64_t)m);
        d.pad[0] = (uint32_t)(int32_t)lo;
        d.pad[1] = (uint32_t)(int32_t)hi;
        row_cap = std::max(row_cap, hi - lo + 1);
        if (scores && !rq.ext) stats.cells += banded_cells((int64_t)n, (int64_t)m, lo, hi);   // (EXT counts the rows it considered: scatter_range)
        for (int64_t s = 0; !scores && s < (int64_t)d.n_stripes; ++s) stats.band_bytes += (uint64_t)(banded_chunks(s * S + 1, S, lo, hi, (int64_t)m) * 16 * S);   // what the fill stores
    }
    PairLaunch pl;
    pl.mem = PairLaunch::MEM_SLOTS;
    if (const int rc = pl.upload_desc(ctx, pd)) return rc;
    // (a table launch: match / mismatch = +- max |submat| -- banded_body places its sentinel by them; the range rule keeps them below 2^27)
    const int k_match = rq.sb ? (int)rq.sb->max_abs : rq.match, k_mismatch = rq.sb ? -(int)rq.sb->max_abs : rq.mismatch;
    pl.set_params((uint32_t)np, (uint32_t)np, k_match, k_mismatch, rq.gap, rq.gt->gap_extend);
    clock.mark("descriptor build + upload");
    if (clock.on) std::fprintf(stderr, "[pwa] banded %s RL=%d pairs=%zu hand-off row=%lld entries\n", scores ? "scores" : "fill", L.cls.rl, np, (long long)row_cap);
    HIPC(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    // (EXT: the same descriptors; the fill leaves rows_out in PairResult::overlap, the walk is NW's)
    const BandedForm form{L.cls.rl, rq.mode, rq.ext != nullptr, rq.sb != nullptr, !scores};
    HIPC(ctx, pwa::banded_launch(form, pl.G, (int)row_cap, rq.ext ? rq.ext->xdrop : 0, rq.sb ? rq.sb->tab : SubstRef{}, ctx->num_cu, ctx->stream, ctx->ev[1]));
    HIPC(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    clock.mark(scores ? "scores pass (device)" : "fill + walk (device)");
    float a = 0, c = 0;
    HIPC(ctx, hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
    HIPC(ctx, hipEventElapsedTime(&c, ctx->ev[1], ctx->ev[2]));
    stats.fill_ms += a;
    if (!scores) stats.tb_ms += c;
    return PWA_OK;
}

// One launch: the pairs' descriptors, fill + walk, the device times into `stats`
int run_launch(pwa_ctx* ctx, const AlignRequest& rq, const AlignArena& ar, const TbPlan& plan, const AlignWorkspaces& ws, const Range& rg,
               const Launch& L, const RangeHost& rh, AlignStats& stats, AlignClock& clock) {
    if (L.cls.banded) return run_banded_launch(ctx, rq, ar, ws, rg, L, rh, stats, clock);
    const size_t np = L.q.size();
    const bool walk_ops = rq.walk_ops();
    std::vector<PairDesc> pd;
    pd.reserve(np + L.n_dummy);
    for (size_t p = 0; p < np; ++p) {
        const uint64_t q = L.q[p], k = rg.k0 + q, n = rq.slen(rq.pair_a[k]), m = rq.slen(rq.pair_b[k]);
        PairDesc d;
        std::memset(&d, 0, sizeof d);
        d.pat = ar.base() + ar.aoff[rq.pair_a[k]];
        d.txt = ar.base() + ar.aoff[rq.pair_b[k]];
        d.n = (int32_t)n;
        d.m = (int32_t)m;
        d.tb = ws.band.as<uint8_t>() + L.bo[p];
        if (plan.sband) d.sband = ws.sband.as<int32_t>() + L.bo[p];
        d.res = ws.res() + q;
        d.ops = walk_ops ? ws.ops() + rh.ooff[q] : ws.ops();   // WALK_OVERLAP never writes ops
        d.ops_cap = (uint32_t)std::min<uint64_t>(n + m, 0xffffffffu);
        d.score_bias = plan.gap0 ? wrap_mul((int64_t)(n + m), rq.gap) : 0;
        pd.push_back(d);
        stats.band_bytes += plan.band_of(L.cls, n, L.cls.mini ? L.mt[p] : m) * plan.band_mult();
    }
    for (uint32_t dmy = 0; dmy < L.n_dummy; ++dmy) {   // empty patterns that fill the last task: every cell of theirs is padding
        PairDesc d = pd[np - 1];
        d.n = 0;
        d.tb = ws.band.as<uint8_t>() + L.dummy_bo[dmy];
        if (plan.sband) d.sband = ws.sband.as<int32_t>() + L.dummy_bo[dmy];
        pd.push_back(d);
    }
    PairLaunch pl;
    pl.mem = PairLaunch::MEM_SLOTS;
    const PairCells cells = plan.gap0 ? CELLS_GAP0 : ar.coded && plan.keyed ? CELLS_CODED : plan.keyed ? CELLS_KEYED : CELLS_PLAIN;
    PairForm form{L.cls.mini ? PF_MINI_FILL : PF_STRIPE_FILL, rq.mode, plan.sband ? BAND_TB_SCORES : BAND_TB, walk_ops ? WALK_OPS : WALK_OVERLAP, cells, L.cls.rl, L.cls.w};
    if (rq.gt) form.family = rq.sb ? PF_MINI_SUBST : PF_MINI_GOTOH, form.cells = CELLS_KEYED;   // (raw bytes, compared; always a mini class)
    if (rq.sb) form.subst = rq.sb->tab;
    int rc = L.cls.mini ? pl.build_mini(ctx, pd, (uint32_t)np, form, plan.k_match, plan.k_mismatch, plan.k_gap)
                        : pl.build(ctx, pd, form, plan.k_match, plan.k_mismatch, plan.k_gap);
    if (rc != PWA_OK) return rc;
    pl.G.dash = ar.dash_sym;
    if (rq.gt) pl.G.gap_extend = rq.gt->gap_extend;
    clock.mark("task list build + upload");
    if (clock.on) std::fprintf(stderr, "[pwa] fill launch %s RL=%d W|LN=%d grid=%u pairs=%u tasks=%u rows=%llu\n", L.cls.mini ? "mini" : "stripes", L.cls.rl,
                               L.cls.w, pl.grid, pl.G.n_pairs, pl.G.n_tasks, (unsigned long long)pl.row_bytes);
    HIPC(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    rc = pl.launch(ctx, ctx->stream, ctx->ev[1]);
    if (rc != PWA_OK) return rc;
    HIPC(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    clock.mark("fill + walk (device)");
    rc = pl.check(ctx);
    if (rc != PWA_OK) return rc;
    float a = 0, c = 0;
    HIPC(ctx, hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
    HIPC(ctx, hipEventElapsedTime(&c, ctx->ev[1], ctx->ev[2]));
    stats.fill_ms += a;
    stats.tb_ms += c;
    return PWA_OK;
}

// The strings of the range: lengths, their exclusive scan (= offsets in the string buffer: every CIGAR, then every MD:Z), the bytes;
// then the offsets come back and, when they fit the caller's buffers, the two packed blocks
int format_range_strings(pwa_ctx* ctx, const AlignRequest& rq, const AlignArena& ar, const AlignWorkspaces& ws, const Range& rg,
                         RangeHost& rh) {
    const uint64_t k0 = rg.k0, nc = rg.k1 - rg.k0;
    const StrOut& str = rq.out.str;
    uint32_t* const clen = rh.clen;
    CigarParams cp;
    cp.arena = ar.base();
    cp.ops = ws.ops();
    cp.res = ws.res();
    cp.pairs = ws.aux.as<const CigarPair>();
    cp.len = reinterpret_cast<uint32_t*>(ws.aux.as<uint8_t>() + ws.aux_len_at);
    cp.out = ws.str.as<uint8_t>();
    cp.decode = 0;
    if (ar.coded)
        for (int v = 255; v >= 0; --v)
            if (ar.seen[v]) cp.decode = cp.decode << 8 | (uint64_t)v;   // code c = the c-th symbol seen, in byte order
    cp.nc = (uint32_t)nc;
    cp.coded = ar.coded;
    cp.local = rq.local() || rq.ext;   // (EXT: a pair with an empty side has no ops, as SW's)
    cp.semi = rq.semi();
    HIPC(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    HIPC(ctx, pwa::cigar_launch(cp, false, ctx->stream));
    pwa::scan_excl(ctx->stream, cp.len, 2 * nc + 2, reinterpret_cast<uint32_t*>(ws.aux.as<uint8_t>() + ws.aux_part_at));
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    HIPC(ctx, pwa::cigar_launch(cp, true, ctx->stream));
    HIPC(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    HIPC(ctx, hipMemcpyAsync(clen, cp.len, (2 * nc + 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    float a = 0, c = 0;
    HIPC(ctx, hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
    HIPC(ctx, hipEventElapsedTime(&c, ctx->ev[1], ctx->ev[2]));
    rh.fmt_ms[0] += a;
    rh.fmt_ms[1] += c;
    const uint64_t tot_c = clen[nc], tot_m = (uint64_t)clen[2 * nc + 1] - tot_c;
    for (uint64_t q = 0; q < nc; ++q) {
        str.cigar_off[k0 + q] = rh.str_at[0] + clen[q];
        str.mdz_off[k0 + q] = rh.str_at[1] + (clen[nc + 1 + q] - tot_c);
    }
    if (tot_c && rh.str_at[0] + tot_c <= str.cigar_cap) HIPC(ctx, hipMemcpy(str.cigar + rh.str_at[0], ws.str.get(), tot_c, hipMemcpyDeviceToHost));
    if (tot_m && rh.str_at[1] + tot_m <= str.mdz_cap)
        HIPC(ctx, hipMemcpy(str.mdz + rh.str_at[1], ws.str.as<uint8_t>() + tot_c, tot_m, hipMemcpyDeviceToHost));
    rh.str_at[0] += tot_c;
    rh.str_at[1] += tot_m;
    return PWA_OK;
}

// The range's results (and op lists) back on the host and into the caller's arrays
// (EXT: rows_out travels in PairResult::overlap, which the banded class does not use otherwise; their sum goes into stats.cells;
// with a table the pattern-end records come back behind the results, in the same copy)
int scatter_range(pwa_ctx* ctx, const AlignRequest& rq, const AlignWorkspaces& ws, const Range& rg, RangeHost& rh, AlignStats& stats, AlignClock& clock) {
    const uint64_t k0 = rg.k0, nc = rg.k1 - rg.k0;
    const AlignOut& o = rq.out;
    const bool local = rq.local(), semi = rq.semi(), want_ops = rq.want_ops();
    PairResult* const res = rh.res;
    HIPC(ctx, hipMemcpy(res, ws.res(), nc * rq.res_bytes(), hipMemcpyDeviceToHost));
    if (want_ops && rg.tiled && rg.span) HIPC(ctx, hipMemcpy(o.ops + rh.ops_lo, ws.ops(), rg.span, hipMemcpyDeviceToHost));   // straight into the caller's list
    if (want_ops && !rg.tiled) HIPC(ctx, hipMemcpy(rh.host_ops.data(), ws.ops(), rg.opsb, hipMemcpyDeviceToHost));
    clock.mark("results (+ ops) to host");
    if (clock.on && want_ops) {   // the op-list walk leaves its LDS round trips in `overlap` (unused by that walk)
        uint64_t trips = 0, nops = 0;
        for (uint64_t q = 0; q < nc; ++q) trips += res[q].overlap, nops += res[q].n_ops;
        std::fprintf(stderr, "[pwa] walk: %llu ops in %llu trips\n", (unsigned long long)nops, (unsigned long long)trips);
    }
    for (uint64_t q = 0; q < nc; ++q) {
        const uint64_t k = k0 + q, n = rq.slen(rq.pair_a[k]), m = rq.slen(rq.pair_b[k]);
        uint64_t cnt = res[q].n_ops;
        if (!(n && m)) {
            // one side empty: NW walks the boundary (hw2.cpp:170-179), SW emits nothing (239), SG walks column 0; no
            // column without a gap, so the overlap is 0 (hw2.cpp:267-278)
            cnt = local || rq.ext ? 0 : semi ? n : n + m;
            if (want_ops)
                for (uint64_t c = 0; c < cnt; ++c) o.ops[o.ops_off[k] + c] = n ? 'D' : 'I';
            if (o.start_cells) o.start_cells[2 * k] = o.start_cells[2 * k + 1] = 0;
            if (o.overlap) o.overlap[k] = 0;
        } else {
            if (res[q].overflow) return fail(ctx, PWA_E_CAPACITY, "internal: traceback longer than n+m");
            if (want_ops && !rg.tiled) std::memcpy(o.ops + o.ops_off[k], rh.host_ops.data() + rh.ooff[q], cnt);
            if (o.start_cells) {
                o.start_cells[2 * k] = res[q].start_i;
                o.start_cells[2 * k + 1] = res[q].start_j;
            }
            if (o.overlap) o.overlap[k] = res[q].overlap;
        }
        o.score[k] = res[q].score;
        if (o.n_ops) o.n_ops[k] = cnt;
        if (o.end_cells) {
            o.end_cells[2 * k] = res[q].end_i;
            o.end_cells[2 * k + 1] = res[q].end_j;
        }
        if (rq.ext) {
            const uint32_t rows = (n && m) ? (uint32_t)res[q].overlap : 0u;
            if (o.rows) o.rows[k] = rows;
            stats.cells += rows;
            if (rh.pend && o.pend_score) o.pend_score[k] = rh.pend[2 * q];
            if (rh.pend && o.pend_j) o.pend_j[k] = (uint32_t)rh.pend[2 * q + 1];
        }
        if (o.end_i) o.end_i[k] = res[q].end_i;
        if (o.end_j) o.end_j[k] = res[q].end_j;
    }
    return PWA_OK;
}

// The stages in call order; `stats` is the context's slot of the calling family (linear or gotoh), zeroed once the request is valid
int align_batch_impl(pwa_ctx* ctx, const AlignRequest& rq, AlignStats& stats) try {
    int rc = validate_align(ctx, rq);
    if (rc != PWA_OK) return rc;
    HIPC(ctx, hipSetDevice(ctx->device));
    stats = AlignStats{};
    AlignClock clock{ctx->knobs.debug};
    AlignArena arena;
    if ((rc = build_align_arena(ctx, rq, clock, arena)) != PWA_OK) return rc;
    const TbPlan plan = make_tb_plan(rq, ctx->knobs, arena.coded, ctx->score_band);
    // what is free once the arena is up decides the ranges; the workspaces are taken after that
    size_t free_b = 0, total_b = 0;
    HIPC(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = std::max<uint64_t>((uint64_t)(free_b * 0.8), 64ull << 20);
    const RangeTarget target = range_target(rq, plan, budget);
    clock.mark("plan: memory + range size");
    const RangePlan rp = plan_ranges(rq, plan, target, budget, free_b);
    if (rp.err != PWA_OK) return fail(ctx, rp.err, rp.msg);
    clock.mark("plan: ranges + launches");
    AlignWorkspaces ws;
    if ((rc = take_align_workspaces(ctx, rq, plan, rp, ws)) != PWA_OK) return rc;
    clock.mark("band / ops allocation");
    if (clock.on) std::fprintf(stderr, "[pwa] bands at %p (codes, %.2f GB) %p (scores)\n", ws.band.get(), (double)rp.band_cap / 1e9, ws.sband.get());
    RangeHost rh;
    for (const Range& rg : rp.ranges) {
        if ((rc = init_range_results(ctx, rq, arena, ws, rg, rh)) != PWA_OK) return rc;
        clock.mark("range results init");
        for (const Launch& L : rg.launches)
            if ((rc = run_launch(ctx, rq, arena, plan, ws, rg, L, rh, stats, clock)) != PWA_OK) return rc;
        if (rq.want_str()) {
            if ((rc = format_range_strings(ctx, rq, arena, ws, rg, rh)) != PWA_OK) return rc;
            clock.mark("strings (device) + copy back");
        }
        if ((rc = scatter_range(ctx, rq, ws, rg, rh, stats, clock)) != PWA_OK) return rc;
        clock.mark("scatter to caller buffers");
    }
    if (clock.on) std::fprintf(stderr, "[pwa] %s: %llu pairs in %zu range(s): fills %.3f ms, walks %.3f ms (device), %.2f GB of band written\n",
                               rq.want_ops() ? "align_batch" : rq.want_str() ? "align_batch_cigar" : rq.scores_only() ? "scores_banded" : "overlaps", (unsigned long long)rq.n_pairs,
                               rp.ranges.size(), stats.fill_ms, stats.tb_ms, (double)stats.band_bytes / 1e9);
    if (rq.want_str()) {
        const StrOut& str = rq.out.str;
        if (clock.on) std::fprintf(stderr, "[pwa] strings: count + scan %.3f ms, write %.3f ms (device); %llu B of CIGAR, %llu B of MD:Z\n", rh.fmt_ms[0],
                                   rh.fmt_ms[1], (unsigned long long)rh.str_at[0], (unsigned long long)rh.str_at[1]);
        str.cigar_off[rq.n_pairs] = rh.str_at[0];
        str.mdz_off[rq.n_pairs] = rh.str_at[1];
        if (str.needed) {
            str.needed[0] = rh.str_at[0];
            str.needed[1] = rh.str_at[1];
        }
        if (rh.str_at[0] > str.cigar_cap || rh.str_at[1] > str.mdz_cap) return fail(ctx, PWA_E_CAPACITY, "CIGAR / MD:Z strings exceed the buffers");
    }
    return PWA_OK;
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
} catch (...) {
    return fail(ctx, PWA_E_HIP, "unexpected C++ exception");   // nothing may propagate across the C ABI
}
}  // namespace

// pwa_selftest_host: TbPlan + range_target + plan_ranges on random length lists with made-up free-memory figures, against what any plan
// must satisfy (not against a second copy of the planner).  0, or the number of the failing check (they continue the sort checks').
int pwa::selftest_align_plan(uint64_t x, int check) {
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int round = 0; round < 48; ++round) {   // every combination of the four switches under each output mode
        const bool gotoh = round & 1, small = round & 2, sband = round & 4, gapped = round & 8;
        const uint32_t n_seq = 400, n_pairs = 1500 + (uint32_t)(rnd() % 1500);
        std::vector<uint64_t> off(n_seq + 1, 0), ops_off(n_pairs);
        for (uint32_t s = 0; s < n_seq; ++s) {   // first half patterns (all three classes, some empty), second half texts (some empty)
            const uint64_t r = rnd() % 16, pat = r == 0 ? 0 : r < 9 ? 1 + rnd() % 256 : (r < 14 || gotoh) ? 257 + rnd() % 768 : 1025 + rnd() % 4000;
            off[s + 1] = off[s] + (s < n_seq / 2 ? pat : r == 0 ? 0 : 1 + rnd() % 3000);
        }
        std::vector<uint32_t> pa(n_pairs), pb(n_pairs);
        const GotohSpec gs{-2, -1};
        AlignRequest rq{PWA_MODE_NW + round % 3, 1, -1, gotoh ? -2 : -1, gotoh ? &gs : nullptr, nullptr, nullptr, off.data(), n_seq, pa.data(), pb.data(), n_pairs, {}};
        rq.out.mode = (AlignOutMode)(round / 16);
        if (rq.out.mode == OUT_OVERLAP && rq.semi()) rq.mode = PWA_MODE_NW;
        rq.out.ops_off = ops_off.data();
        for (uint64_t k = 0, at = 0; k < n_pairs; ++k) {
            pa[k] = (uint32_t)(rnd() % (n_seq / 2));
            pb[k] = n_seq / 2 + (uint32_t)(rnd() % (n_seq / 2));
            ops_off[k] = at += (gapped && rnd() % 8 == 0) ? 1 + rnd() % 5 : 0;
            at += rq.slen(pa[k]) + rq.slen(pb[k]);
        }
        Knobs kn;
        if (small) kn.range_bytes = 3u << 20;
        const uint64_t free_b = (rnd() & 1) ? 200ull << 30 : 1ull << 30, budget = std::max<uint64_t>((uint64_t)(free_b * 0.8), 64ull << 20);
        const TbPlan plan = make_tb_plan(rq, kn, !gotoh, sband);
        const RangeTarget tg = range_target(rq, plan, budget);
        const RangePlan rp = plan_ranges(rq, plan, tg, budget, free_b);
        if (plan.band_mult() != (sband && !gotoh ? 5u : 1u)) return check + 1;
        // 1: the ranges partition the list in order (and a small PWA_RANGE_BYTES does cut it)
        if (rp.err != PWA_OK || rp.ranges.empty() || rp.ranges[0].k0 != 0 || rp.ranges.back().k1 != n_pairs || (small && rp.ranges.size() < 2)) return check + 1;
        for (size_t r = 0; r < rp.ranges.size(); ++r) {
            const Range& rg = rp.ranges[r];
            const uint64_t k0 = rg.k0, nc = rg.k1 - rg.k0;
            if (rg.k1 <= k0 || (r && k0 != rp.ranges[r - 1].k1)) return check + 1;
            auto len_n = [&](uint64_t q) { return rq.slen(pa[k0 + q]); };
            auto len_m = [&](uint64_t q) { return rq.slen(pb[k0 + q]); };
            // 2: every live pair in exactly one launch, of its class; pairs with an empty side in none
            std::vector<uint32_t> times(nc, 0);
            std::vector<std::pair<uint64_t, uint64_t>> bands;   // [first, second) of every pair and dummy
            for (const Launch& L : rg.launches) {
                const size_t np = L.q.size(), ppw = L.cls.mini ? (size_t)(64 / L.cls.w) : 1;
                if (L.bo.size() != np || np == 0) return check + 2;
                for (size_t p = 0; p < np; ++p) {
                    if (L.q[p] >= nc || !(L.cls == plan.class_of(len_n(L.q[p])))) return check + 2;
                    ++times[L.q[p]];
                    // 3: a mini launch runs its pairs by falling text length, each band sized for its task's first text; dummies complete the last task
                    if (L.cls.mini && (L.mt.size() != np || (p && len_m(L.q[p]) > len_m(L.q[p - 1])) || L.mt[p] != len_m(L.q[p / ppw * ppw]))) return check + 3;
                    bands.emplace_back(L.bo[p], L.bo[p] + plan.band_of(L.cls, len_n(L.q[p]), L.cls.mini ? L.mt[p] : len_m(L.q[p])));
                }
                if (L.n_dummy >= ppw || (np + L.n_dummy) % ppw) return check + 3;
                for (uint32_t d = 0; d < L.n_dummy; ++d) bands.emplace_back(L.dummy_bo[d], L.dummy_bo[d] + plan.band_of(L.cls, 0, L.mt[np - 1]));
            }
            // 4: bands start on multiples of 256, do not overlap and end inside the range's band
            std::sort(bands.begin(), bands.end());
            for (size_t i = 0; i < bands.size(); ++i)
                if (bands[i].first % 256 || bands[i].second > rg.band || (i && bands[i].first < bands[i - 1].second)) return check + 4;
            // 5: the sums a range is closed by (its first live pair is in whatever the targets say), and the workspaces sized from them
            uint64_t est = 0, op_bytes = 0, opsb = 0, strb = 0, live = 0;
            bool tiled = rq.want_ops();
            for (uint64_t q = 0; q < nc; ++q) {
                const uint64_t n = len_n(q), m = len_m(q);
                if (times[q] != ((n && m) ? 1u : 0u)) return check + 2;
                if (n && m) est += align_up(plan.band_of(plan.class_of(n), n, m), 256), ++live;
                op_bytes += n + m;
                opsb += align_up(n + m + 1, 16);
                if (rq.want_str()) strb += str_bound(n + m);
                if (q + 1 < nc && ops_off[k0 + q + 1] != ops_off[k0 + q] + n + m) tiled = false;
            }
            if (nc > 1 && (est * plan.band_mult() + op_bytes > tg.chunk_target || live > std::max<uint64_t>(tg.pairs_target, 1) || strb > 0xffffffffull)) return check + 5;
            if (rg.opsb != opsb || rg.strb != strb || rp.band_cap < rg.band || rp.nc_cap < nc || rp.ops_cap_b < opsb || rp.str_cap < strb) return check + 5;
            // 6: tiled / span against the caller's op offsets
            if (rg.tiled != tiled || rg.span != (rq.want_ops() ? op_bytes : 0) || (tiled && rp.ops_cap_b < rg.span + 16)) return check + 6;
        }
    }
    return 0;
}

// What an affine-gap entry point adds to its request (whose gap is gap_open): the call's table, band arrays and xdrop where it has
// them, and the context's stats slot it reports into
struct AffineSpec {
    int gap_extend;
    AlignStats* stats;
    bool subst = false, banded = false, ext = false;
    const uint8_t* code = nullptr;   // subst
    int n_sym = 0;
    const int32_t* submat = nullptr;
    const int32_t *band_lo = nullptr, *band_hi = nullptr;   // banded: one (lo, hi) per pair
    int xdrop = 0;                                          // ext
    AffineSpec& table(const uint8_t* c, int n, const int32_t* m) { return subst = true, code = c, n_sym = n, submat = m, *this; }
    AffineSpec& band(const int32_t* lo, const int32_t* hi) { return banded = true, band_lo = lo, band_hi = hi, *this; }
    AffineSpec& extend(int x) { return ext = true, xdrop = x, *this; }
};

// The affine-gap entry points' own checks, in the order every one of them has had them -- gap signs, mode, the table, the band arrays
// (validate_align checks every pair's band) --, then the spec structs hang on the request.  A table is checked, copied and uploaded
// for the call, once (every range of a PWA_RANGE_BYTES-cut list launches with it; the device copy goes back to the context's buffer
// list when the call returns), after the request has been validated: nothing is allocated for a request that is refused.
static int affine_batch(pwa_ctx* ctx, AlignRequest rq, const AffineSpec& sp) try {
    if (rq.gap > 0 || sp.gap_extend > 0)
        return fail(ctx, PWA_E_INVALID, sp.subst ? "gap penalties must be <= 0 (gap_open + L * gap_extend)" : "gotoh gap penalties must be <= 0 (gap_open + L * gap_extend)");
    if (rq.mode != PWA_MODE_NW && rq.mode != PWA_MODE_SW && rq.mode != PWA_MODE_SG) return fail(ctx, PWA_E_INVALID, "unknown mode");
    SubstTable tab;
    int rc = sp.subst ? subst_prepare(ctx, sp.code, sp.n_sym, sp.submat, tab) : PWA_OK;
    if (rc != PWA_OK) return rc;
    if (sp.banded && rq.n_pairs && (!sp.band_lo || !sp.band_hi)) return fail(ctx, PWA_E_INVALID, "null input");
    const GotohSpec gs{rq.gap, sp.gap_extend};
    SubstSpec ss{{nullptr, tab.n_sym, tab.stride}, tab.max_abs};
    const BandSpec bs{sp.band_lo, sp.band_hi};
    const ExtSpec es{sp.xdrop};
    rq.gt = &gs;
    if (sp.subst) rq.sb = &ss;
    if (sp.banded) rq.bd = &bs;
    if (sp.ext) rq.ext = &es;
    if (sp.subst) {
        if ((rc = validate_align(ctx, rq)) != PWA_OK) return rc;   // (align_batch_impl checks again)
        HIPC(ctx, hipSetDevice(ctx->device));
        if ((rc = subst_upload(ctx, tab)) != PWA_OK) return rc;
        ss.tab.tab = tab.dev.as<uint32_t>();
    }
    return align_batch_impl(ctx, rq, *sp.stats);
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
}

// a stats slot of the context into a call's (optional) outputs; `count`: its band bytes, or the cells / rows of the banded score and EXT calls
static int put_stats(const pwa_ctx* ctx, AlignStats pwa_ctx::*slot, float* fill_ms, float* walk_ms, uint64_t* count, uint64_t AlignStats::*what = &AlignStats::band_bytes) {
    if (!ctx) return PWA_E_INVALID;
    const AlignStats& st = ctx->*slot;
    if (fill_ms) *fill_ms = st.fill_ms;
    if (walk_ms) *walk_ms = st.tb_ms;
    if (count) *count = st.*what;
    return PWA_OK;
}

extern "C" {

int pwa_align_batch(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, const uint8_t* seq_bytes,
                    const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                    uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops,
                    uint64_t* end_cells, uint64_t* start_cells) {
    if (!ctx) return PWA_E_INVALID;
    if (!ops) return fail(ctx, PWA_E_INVALID, "null input");
    return align_batch_impl(ctx, request(mode, match, mismatch, gap, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                         out_ops(score_out, end_cells, start_cells, ops, ops_off, n_ops)), ctx->align_stats);
}

int pwa_align_batch_cigar(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, const uint8_t* seq_bytes, const uint64_t* seq_off,
                          uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                          uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells,
                          uint64_t* start_cells, uint64_t needed[2]) {
    if (!ctx) return PWA_E_INVALID;
    return align_batch_impl(ctx, request(mode, match, mismatch, gap, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                         out_strings(score_out, end_cells, start_cells, {cigar, mdz, cigar_cap, mdz_cap, cigar_off, mdz_off, needed})), ctx->align_stats);
}

// affine gaps on the gotoh mini-stripe kernels
int pwa_align_gotoh_batch(pwa_ctx* ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                          const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                          int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells, uint64_t* start_cells) {
    if (!ctx) return PWA_E_INVALID;
    if (!ops) return fail(ctx, PWA_E_INVALID, "null input");
    return affine_batch(ctx, request(mode, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_ops(score_out, end_cells, start_cells, ops, ops_off, n_ops)),
                        AffineSpec{gap_extend, &ctx->gotoh_stats});
}

int pwa_align_gotoh_batch_cigar(pwa_ctx* ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                                const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                                int32_t* score_out, char* cigar, uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap,
                                uint64_t* mdz_off, uint64_t* end_cells, uint64_t* start_cells, uint64_t needed[2]) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(mode, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_strings(score_out, end_cells, start_cells, {cigar, mdz, cigar_cap, mdz_cap, cigar_off, mdz_off, needed})),
                        AffineSpec{gap_extend, &ctx->gotoh_stats});
}

int pwa_align_gotoh_last_stats(const pwa_ctx* ctx, float* fill_ms, float* walk_ms, uint64_t* band_bytes) {
    return put_stats(ctx, &pwa_ctx::gotoh_stats, fill_ms, walk_ms, band_bytes);
}

// ... inside a diagonal band per pair
int pwa_align_banded_batch(pwa_ctx* ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                           const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                           int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells, uint64_t* start_cells,
                           const int32_t* band_lo, const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    if (!ops) return fail(ctx, PWA_E_INVALID, "null input");
    return affine_batch(ctx, request(mode, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out_ops(score_out, end_cells, start_cells, ops, ops_off, n_ops)),
                        AffineSpec{gap_extend, &ctx->banded_stats}.band(band_lo, band_hi));
}

int pwa_align_banded_batch_cigar(pwa_ctx* ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                                 const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                                 int32_t* score_out, char* cigar, uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap,
                                 uint64_t* mdz_off, uint64_t* end_cells, uint64_t* start_cells, uint64_t needed[2], const int32_t* band_lo,
                                 const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(mode, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_strings(score_out, end_cells, start_cells, {cigar, mdz, cigar_cap, mdz_cap, cigar_off, mdz_off, needed})),
                        AffineSpec{gap_extend, &ctx->banded_stats}.band(band_lo, band_hi));
}

int pwa_align_banded_last_stats(const pwa_ctx* ctx, float* fill_ms, float* walk_ms, uint64_t* band_bytes) {
    return put_stats(ctx, &pwa_ctx::banded_stats, fill_ms, walk_ms, band_bytes);
}

// the scores-only form: the same request with nothing to hand back but scores and end cells (OUT_SCORES: no band, no walk)
int pwa_scores_banded(pwa_ctx* ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                      uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint32_t* end_i_out,
                      uint32_t* end_j_out, const int32_t* band_lo, const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(mode, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out_scores(score_out, end_i_out, end_j_out)),
                        AffineSpec{gap_extend, &ctx->banded_scores_stats}.band(band_lo, band_hi));
}

int pwa_scores_banded_last_stats(const pwa_ctx* ctx, float* fill_ms, uint64_t* in_band_cells) {
    return put_stats(ctx, &pwa_ctx::banded_scores_stats, fill_ms, nullptr, in_band_cells, &AlignStats::cells);
}

// the EXT entry points: the banded calls over NW's matrix with the call's xdrop; they report into their own slot
int pwa_extend_banded_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, int xdrop, const uint8_t* seq_bytes,
                            const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                            int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells, uint32_t* rows_out,
                            const int32_t* band_lo, const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    if (!ops) return fail(ctx, PWA_E_INVALID, "null input");
    return affine_batch(ctx, request(PWA_MODE_NW, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_ops(score_out, end_cells, nullptr, ops, ops_off, n_ops).ext(rows_out)),
                        AffineSpec{gap_extend, &ctx->ext_stats}.band(band_lo, band_hi).extend(xdrop));
}

int pwa_extend_banded_batch_cigar(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, int xdrop, const uint8_t* seq_bytes,
                                  const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                                  int32_t* score_out, char* cigar, uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap,
                                  uint64_t* mdz_off, uint64_t* end_cells, uint32_t* rows_out, uint64_t needed[2], const int32_t* band_lo,
                                  const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(PWA_MODE_NW, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_strings(score_out, end_cells, nullptr, {cigar, mdz, cigar_cap, mdz_cap, cigar_off, mdz_off, needed}).ext(rows_out)),
                        AffineSpec{gap_extend, &ctx->ext_stats}.band(band_lo, band_hi).extend(xdrop));
}

int pwa_scores_extend_banded(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, int xdrop, const uint8_t* seq_bytes,
                             const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                             int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out, uint32_t* rows_out, const int32_t* band_lo,
                             const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(PWA_MODE_NW, match, mismatch, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out_scores(score_out, end_i_out, end_j_out).ext(rows_out)),
                        AffineSpec{gap_extend, &ctx->ext_stats}.band(band_lo, band_hi).extend(xdrop));
}

// their substitution-matrix forms, which also hand back the pattern-end result
int pwa_extend_banded_subst_batch(pwa_ctx* ctx, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend, int xdrop,
                                  const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                                  uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells,
                                  uint32_t* rows_out, int32_t* pend_score_out, uint32_t* pend_j_out, const int32_t* band_lo, const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    if (!ops) return fail(ctx, PWA_E_INVALID, "null input");
    return affine_batch(ctx, request(PWA_MODE_NW, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_ops(score_out, end_cells, nullptr, ops, ops_off, n_ops).ext(rows_out, pend_score_out, pend_j_out)),
                        AffineSpec{gap_extend, &ctx->ext_stats}.table(code, n_sym, submat).band(band_lo, band_hi).extend(xdrop));
}

int pwa_extend_banded_subst_batch_cigar(pwa_ctx* ctx, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend, int xdrop,
                                        const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a,
                                        const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar, uint64_t cigar_cap,
                                        uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells, uint32_t* rows_out,
                                        int32_t* pend_score_out, uint32_t* pend_j_out, uint64_t needed[2], const int32_t* band_lo,
                                        const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(PWA_MODE_NW, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_strings(score_out, end_cells, nullptr, {cigar, mdz, cigar_cap, mdz_cap, cigar_off, mdz_off, needed}).ext(rows_out, pend_score_out, pend_j_out)),
                        AffineSpec{gap_extend, &ctx->ext_stats}.table(code, n_sym, submat).band(band_lo, band_hi).extend(xdrop));
}

int pwa_scores_extend_banded_subst(pwa_ctx* ctx, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend, int xdrop,
                                   const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                                   uint64_t n_pairs, int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out, uint32_t* rows_out,
                                   int32_t* pend_score_out, uint32_t* pend_j_out, const int32_t* band_lo, const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(PWA_MODE_NW, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_scores(score_out, end_i_out, end_j_out).ext(rows_out, pend_score_out, pend_j_out)),
                        AffineSpec{gap_extend, &ctx->ext_stats}.table(code, n_sym, submat).band(band_lo, band_hi).extend(xdrop));
}

int pwa_extend_banded_last_stats(const pwa_ctx* ctx, float* fill_ms, float* walk_ms, uint64_t* rows_considered) {
    return put_stats(ctx, &pwa_ctx::ext_stats, fill_ms, walk_ms, rows_considered, &AlignStats::cells);
}

// the gotoh classes with the diagonal score from the caller's table
int pwa_align_subst_batch(pwa_ctx* ctx, int mode, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend,
                          const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                          uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells,
                          uint64_t* start_cells) {
    if (!ctx) return PWA_E_INVALID;
    if (!ops) return fail(ctx, PWA_E_INVALID, "null input");
    return affine_batch(ctx, request(mode, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out_ops(score_out, end_cells, start_cells, ops, ops_off, n_ops)),
                        AffineSpec{gap_extend, &ctx->subst_stats}.table(code, n_sym, submat));
}

int pwa_align_subst_batch_cigar(pwa_ctx* ctx, int mode, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend,
                                const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a,
                                const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar, uint64_t cigar_cap,
                                uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells,
                                uint64_t* start_cells, uint64_t needed[2]) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(mode, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_strings(score_out, end_cells, start_cells, {cigar, mdz, cigar_cap, mdz_cap, cigar_off, mdz_off, needed})),
                        AffineSpec{gap_extend, &ctx->subst_stats}.table(code, n_sym, submat));
}

// the banded forms; they report where the banded calls report
int pwa_align_banded_subst_batch(pwa_ctx* ctx, int mode, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend,
                                 const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                                 uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells,
                                 uint64_t* start_cells, const int32_t* band_lo, const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    if (!ops) return fail(ctx, PWA_E_INVALID, "null input");
    return affine_batch(ctx, request(mode, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out_ops(score_out, end_cells, start_cells, ops, ops_off, n_ops)),
                        AffineSpec{gap_extend, &ctx->banded_stats}.table(code, n_sym, submat).band(band_lo, band_hi));
}

int pwa_align_banded_subst_batch_cigar(pwa_ctx* ctx, int mode, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend,
                                       const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a,
                                       const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar, uint64_t cigar_cap,
                                       uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells,
                                       uint64_t* start_cells, uint64_t needed[2], const int32_t* band_lo, const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(mode, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                                     out_strings(score_out, end_cells, start_cells, {cigar, mdz, cigar_cap, mdz_cap, cigar_off, mdz_off, needed})),
                        AffineSpec{gap_extend, &ctx->banded_stats}.table(code, n_sym, submat).band(band_lo, band_hi));
}

int pwa_scores_banded_subst(pwa_ctx* ctx, int mode, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend,
                            const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                            uint64_t n_pairs, int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out, const int32_t* band_lo,
                            const int32_t* band_hi) {
    if (!ctx) return PWA_E_INVALID;
    return affine_batch(ctx, request(mode, 0, 0, gap_open, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out_scores(score_out, end_i_out, end_j_out)),
                        AffineSpec{gap_extend, &ctx->banded_scores_stats}.table(code, n_sym, submat).band(band_lo, band_hi));
}

int pwa_align_subst_last_stats(const pwa_ctx* ctx, float* fill_ms, float* walk_ms, uint64_t* band_bytes) {
    return put_stats(ctx, &pwa_ctx::subst_stats, fill_ms, walk_ms, band_bytes);
}

int pwa_overlaps(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, const uint8_t* seq_bytes, const uint64_t* seq_off,
                 uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out,
                 int32_t* overlap_out) {
    if (!ctx) return PWA_E_INVALID;
    if (!overlap_out) return fail(ctx, PWA_E_INVALID, "null input");
    AlignOut out;
    out.mode = OUT_OVERLAP, out.score = score_out, out.overlap = overlap_out;
    return align_batch_impl(ctx, request(mode, match, mismatch, gap, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, out), ctx->align_stats);
}

int pwa_align(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, const uint8_t* pattern, uint64_t n,
              const uint8_t* text, uint64_t m, int32_t* score, uint8_t* ops, uint64_t ops_cap, uint64_t* n_ops,
              uint64_t end_cell[2], uint64_t start_cell[2]) try {
    if (!ctx) return PWA_E_INVALID;
    if (!score || !ops || !n_ops || (n && !pattern) || (m && !text)) return fail(ctx, PWA_E_INVALID, "null input");
    if (ops_cap < n + m) return fail(ctx, PWA_E_CAPACITY, "ops_cap must be at least n + m");
    std::vector<uint8_t> bytes(n + m);
    if (n) std::memcpy(bytes.data(), pattern, n);
    if (m) std::memcpy(bytes.data() + n, text, m);
    const uint64_t off[3] = {0, n, n + m};
    const uint32_t a = 0, b = 1;
    const uint64_t ooff = 0;
    return pwa_align_batch(ctx, mode, match, mismatch, gap, bytes.data(), off, 2, &a, &b, 1, score, ops, &ooff, n_ops,
                           end_cell, start_cell);
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
} catch (...) {
    return fail(ctx, PWA_E_HIP, "unexpected C++ exception");   // nothing may propagate across the C ABI
}

int pwa_align_matrices(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, const uint8_t* pattern, uint64_t n,
                       const uint8_t* text, uint64_t m, int32_t* dp_out, char* tb_out) try {
    if (!ctx) return PWA_E_INVALID;
    if (mode != PWA_MODE_NW && mode != PWA_MODE_SW && mode != PWA_MODE_SG) return fail(ctx, PWA_E_INVALID, "unknown mode");
    if ((n && !pattern) || (m && !text) || (!dp_out && !tb_out)) return fail(ctx, PWA_E_INVALID, "null input");
    if (n > 0x7fffffc0ull || m > 0x7fffffc0ull) return fail(ctx, PWA_E_CAPACITY, "sequence longer than 2^31");
    const bool keyed = tb_range_ok(n + m, match, mismatch, gap, mode == PWA_MODE_SW ? 26 : 28) && !ctx->knobs.no_keyed_tb;
    const bool local = mode == PWA_MODE_SW, semi = mode == PWA_MODE_SG;
    const uint64_t W = m + 1;
    // row 0 and column 0 exactly as the reference initialises them (hw2.cpp:119-136 / 193-194)
    for (uint64_t i = 0; i <= n; ++i) {
        if (dp_out) dp_out[i * W] = local ? 0 : wrap_mul((int64_t)i, gap);
        if (tb_out) tb_out[i * W] = (!local && i > 0) ? 'u' : ' ';
    }
    for (uint64_t j = 0; j <= m; ++j) {
        if (dp_out) dp_out[j] = local || semi ? 0 : wrap_mul((int64_t)j, gap);   // (semi-global: row 0 is free)
        if (tb_out) tb_out[j] = (!local && !semi && j > 0) ? 'l' : ' ';
    }
    if (n == 0 || m == 0) return PWA_OK;
    HIPC(ctx, hipSetDevice(ctx->device));
    // patterns of up to 256 rows over an alphabet of <= 7 symbols: the mini-stripe engine, as pwa_align_batch would pick it (so that
    // the whole-matrix comparison covers that engine's cells too); everything else: the stripe engine on raw bytes
    uint8_t code_of[256];
    bool seen[256] = {false};
    for (uint64_t o = 0; o < n; ++o) seen[pattern[o]] = true;
    for (uint64_t o = 0; o < m; ++o) seen[text[o]] = true;
    const bool coded = code_alphabet(seen, code_of, match, mismatch, gap, ctx->knobs);
    int mini_rl = 0, wide_rl = 0;   // wide: one pair per wave (PWA_TB_ENGINE=2 here: a single pair would normally take pipelined stripes)
    if (mini_eligible(ctx->knobs, coded, keyed, local, n + m, match, mismatch, gap)) {
        mini_rl = mini_rl_for(n);
        if (!mini_rl && n <= 1024 && ctx->knobs.tb_engine == 2) wide_rl = wide_rl_for(n);
    }
    const PairGeom geom = mini_rl ? PairGeom{mini_rl, 1} : wide_rl ? PairGeom{wide_rl, 1} : choose_geom(ctx->knobs, n, keyed, true);
    const uint64_t kRL = (uint64_t)geom.rl;
    const uint64_t band = mini_rl ? (uint64_t)mini_band_steps(m) * 16 * kRL : tb_band_bytes(n, m, geom.rl);   // (wide: one 64 RL-row stripe)
    DevBuf d_pat, d_txt, d_band, d_sband, d_res;
    HIPC(ctx, d_pat.alloc(ctx, n + 64));
    HIPC(ctx, d_txt.alloc(ctx, m + 64));
    HIPC(ctx, d_band.alloc(ctx, (mini_rl ? 4 : 1) * band + 32768));
    HIPC(ctx, d_sband.alloc(ctx, (mini_rl ? 4 : 1) * band * sizeof(int32_t)));
    HIPC(ctx, d_res.alloc(ctx, sizeof(PairResult)));
    if (mini_rl || wide_rl) {
        std::vector<uint8_t> cp(n), ct(m);
        for (uint64_t o = 0; o < n; ++o) cp[o] = code_of[pattern[o]];
        for (uint64_t o = 0; o < m; ++o) ct[o] = code_of[text[o]];
        HIPC(ctx, upload_via_bounce(ctx, d_pat.p, cp.data(), n));
        HIPC(ctx, upload_via_bounce(ctx, d_txt.p, ct.data(), m));
    } else {
        HIPC(ctx, hipMemcpy(d_pat.p, pattern, n, hipMemcpyHostToDevice));
        HIPC(ctx, hipMemcpy(d_txt.p, text, m, hipMemcpyHostToDevice));
    }
    HIPC(ctx, hipMemset(d_res.p, 0, sizeof(PairResult)));
    std::vector<PairDesc> pd(1);
    std::memset(&pd[0], 0, sizeof(PairDesc));
    pd[0].pat = d_pat.as<uint8_t>();
    pd[0].txt = d_txt.as<uint8_t>();
    pd[0].n = (int32_t)n;
    pd[0].m = (int32_t)m;
    pd[0].tb = d_band.as<uint8_t>();
    pd[0].sband = d_sband.as<int32_t>();
    pd[0].res = d_res.as<PairResult>();
    PairLaunch pl;
    PairForm form{PF_STRIPE_FILL, mode, BAND_TB_SCORES, WALK_NONE, keyed ? CELLS_KEYED : CELLS_PLAIN, geom.rl, geom.w};   // raw bytes; only the bands are read
    if (mini_rl || wide_rl) form.family = PF_MINI_FILL, form.cells = CELLS_CODED, form.w = mini_rl ? 16 : 64;
    for (int d = 1; mini_rl && d < 4; ++d) {   // three empty patterns fill the wave; their padding goes behind the pair's bands
        PairDesc e = pd[0];
        e.n = 0;
        e.tb = d_band.as<uint8_t>() + (uint64_t)d * band;
        e.sband = d_sband.as<int32_t>() + (uint64_t)d * band;
        pd.push_back(e);
    }
    int rc = form.mini() ? pl.build_mini(ctx, pd, 1, form, match, mismatch, gap) : pl.build(ctx, pd, form, match, mismatch, gap);
    if (rc != PWA_OK) return rc;
    rc = pl.launch(ctx, ctx->stream, nullptr);
    if (rc != PWA_OK) return rc;
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    rc = pl.check(ctx);
    if (rc != PWA_OK) return rc;
    std::vector<uint8_t> hb(tb_out ? band : 0);
    std::vector<int32_t> hs(dp_out ? band : 0);
    if (tb_out) HIPC(ctx, hipMemcpy(hb.data(), d_band.p, band, hipMemcpyDeviceToHost));
    if (dp_out) HIPC(ctx, hipMemcpy(hs.data(), d_sband.p, band * sizeof(int32_t), hipMemcpyDeviceToHost));
    // band codes are tie-break priorities (pair_fill.hip.h): global up 0, left 1, diag 2; local left 0, up 1, diag 2, floor 3
    static const char kCodeNW[4] = {'u', 'l', 'd', 'd'}, kCodeSW[4] = {'l', 'u', 'd', '0'};   // hw2.cpp:145-153 / 214-222
    const char* const kCode = local ? kCodeSW : kCodeNW;
    const uint64_t T = band_steps(m);
    const uint64_t PA = kRL >= 16 ? 16 : (kRL >= 8 ? 8 : 4), PB = kRL - PA;   // BandGeo<LN, RL> of the mini-stripe kernels
    const uint64_t LN = mini_rl ? 16 : 64, Q4 = kRL & ~(uint64_t)3, W4 = kRL & 3;
    for (uint64_t i = 1; i <= n; ++i) {
        const uint64_t q = i - 1;
        for (uint64_t j = 1; j <= m; ++j) {
            uint64_t idx, sidx;   // skewed bands -> row-major matrix
            if (mini_rl || wide_rl) {
                const uint64_t k = q / kRL, r = q % kRL, t = j - 1 + k;
                idx = t * LN * kRL + (r < PA ? k * PA + r : LN * PA + k * PB + (r - PA));
                sidx = t * LN * kRL + (r < Q4 ? (r >> 2) * (LN * 4) + k * 4 + (r & 3) : Q4 * LN + k * W4 + (r & 3));   // BandGeo::sband_off
            } else {
                const uint64_t st = q / (64 * kRL), k = (q % (64 * kRL)) / kRL, r = q % kRL;
                idx = sidx = ((st * T + (j - 1 + k)) * 64 + k) * kRL + r;
            }
            if (tb_out) tb_out[i * W + j] = kCode[hb[idx] & 3];
            if (dp_out) dp_out[i * W + j] = hs[sidx];
        }
    }
    return PWA_OK;
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
} catch (...) {
    return fail(ctx, PWA_E_HIP, "unexpected C++ exception");   // nothing may propagate across the C ABI
}

int pwa_align_last_stats(const pwa_ctx* ctx, float* fill_ms, float* traceback_ms, uint64_t* band_bytes) {
    return put_stats(ctx, &pwa_ctx::align_stats, fill_ms, traceback_ms, band_bytes);
}

}  // extern "C"
