// pwalign.hip -- score batches: pwa_*batch_create (the strip / stripe / mini-stripe scheduler of a pair list), pwa_batch_run ..
// pwa_batch_destroy, and the one-shot calls over lists of any size (pwa_scores, pwa_distances, pwa_scores_affine, pwa_scores_gotoh, pwa_scores_subst).  The rest of the
// C ABI of include/pwalign.h: pwalign_ctx.hip (contexts, memory), pwalign_affine_tb.hip, pwalign_align.hip.  gfx950 only; no CPU path.
#include "pwalign_internal.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <numeric>

using namespace pwa;

// ------------------------------------------------------------------------------------ batch
struct pwa_batch {
    pwa_ctx* ctx = nullptr;
    int mode = 0;
    uint64_t n_pairs = 0;
    uint64_t cells = 0, padded_cells = 0;
    bool want_end = false;
    // engine 1: register-strip kernels
    bool use_strips = false;        // some pairs run on the register-strip kernels
    bool use_pairs = false;         // some (or, with end cells / scorings the strips cannot pad for, all) pairs run on the stripe engine
    const BatchKernelEntry* kern = nullptr;
    BatchParams bp{};
    bool affine = false, nwdist = false, lanes = false;
    bool gotoh = false;             // affine-gap (gotoh) scores: batch_gotoh_kernel strips, or the band-less gotoh mini-stripe fills in `mini`
    SubstTable subst;               // pwa_subst_batch_create: the batch's own copy of the caller's table, host and device (n_sym = 0: none)
    void* strip_fn = nullptr;         // the strip kernel this batch launches (strip_kernel_fn)
    bool cell16 = false;            // the strips run two pairs per lane in packed f16 cells (batch_scores.hip.h, CELL16)
    bool prof16 = false;            // ... in their profile form: one pattern per wave task (batch_scores.hip.h, PROF16)
    bool prof16_int = false;        // ... with the integer-coded row step (H as an integer per half; prof16_int_admitted)
    int32_t aff_go = 0, aff_ge = 0, aff_neg = 0;
    uint32_t grid = 0;
    DevBuf arena, tasks, slot_poff, slot_plen, slot_out, slot_toff, slot_tlen, lane_text, hand, queue, scores;
    // engine 2: wavefront kernels without traceback band (exact end cells, any scoring)
    PairLaunch pl;
    std::vector<std::unique_ptr<PairLaunch>> mini;   // engine 3: mini-stripe launches without a band, one per row class (short patterns routed off the strips)
    DevBuf pair_res;
    uint64_t n_live = 0;            // pairs that reach a kernel (n > 0 and m > 0)
    std::vector<uint32_t> live_idx; // pairs off the strips: pair index of result slot q (stripe engine's pairs first, then the mini launches')
    std::vector<int32_t> host_scores;   // trivial pairs resolved on the host
    std::vector<uint32_t> host_end_i, host_end_j;
    std::string kernel_name;
    int32_t* ext_scores = nullptr;      // caller-owned device score vector (pwa_batch_set_d_scores)
    static constexpr int kRing = 64;          // event pairs of the most recent runs
    hipEvent_t ev0[kRing] = {}, ev1[kRing] = {};
    uint64_t n_runs = 0;
    bool ran = false;
};

namespace {

// Packed f16 strip cells (batch_scores.hip.h, CELL16): VALU per lane row and column, both pairs together -- perm, pk_add,
// pk_maximum3, pk_add clamp, 1/2 pk_maximum3 for the running best, + the hand-off share ([gpu] PMC on C3: 4.56)
constexpr double kCell16Vpr = 4.6;
// The profile form (PROF16): 3.5 VALU per lane row -- indexed pk_add clamp, pk_maximum3, pk_add, 1/2 pk_maximum3 -- + the f16 row's
// v_mov and the per-block profile ([gpu] tools/valu_issue.hip: 6.43 against CELL16's 7.62 cycles per cell at two waves per SIMD;
// its integer-coded row 6.00 in the same table).  The integer row has had no v_mov since r06; the figure was fitted before that and
// has not been re-fitted, so both rows are still priced alike.
constexpr double kProf16Vpr = 3.8;
constexpr int kProf16R = 152;   // the rows of its single strip (batch_scores16p_kernel<152>): the admission limit
// ... and the rows a task of an n-row pattern runs: the kernel skips the pad rows past n rounded up to a pair of rows.  Skipped rows
// are priced as nothing, which is a little low: per 8-column block a skipped pair of the integer row still issues 9 VALU (of a pair's
// 56), 2 scalar instructions and a taken branch, a skipped f16 row 3 scalar instructions, a taken branch and its v_mov.  For 100-row
// patterns that is 26 pairs, ~230 VALU against ~2800 of the rows that run (about 8 %); DESIGN.md r06 has the measured times.
constexpr uint64_t prof16_rows(uint64_t n) { return n <= 2 ? 2 : (n + 1) / 2 * 2; }
// f16 bit pattern of k * 2^-11 for |k| <= 1023: a normal number (exponent k's leading bit + 4), exact
uint32_t f16_bits_scaled(int k) {
    if (k == 0) return 0;
    const uint32_t sign = k < 0 ? 0x8000u : 0u, a = (uint32_t)std::abs(k);
    int e = 0;
    while ((a >> (e + 1)) != 0) ++e;
    return sign | ((uint32_t)(e + 4) << 10) | ((a - (1u << e)) << (10 - e));
}

// ---------------------------------------------------------------------------- batch: create
enum { KIND_LINEAR = 0, KIND_AFFINE = 1, KIND_NWDIST = 2, KIND_GOTOH = 3, KIND_SUBST = 4 };   // KIND_SUBST: gotoh under a substitution table
constexpr uint64_t kGotohMiniMaxN = 1024;   // patterns of the band-less gotoh fills: 16 lanes x kMiniRL rows, then 64 lanes x 8 | 16 rows

// The caller's sequences, pair list and scoring, as the stages of batch_create_impl see them
struct BatchInput {
    const uint8_t* seq_bytes;
    const uint64_t* seq_off;
    uint32_t n_seq;
    const uint32_t* pair_a;
    const uint32_t* pair_b;
    uint64_t n_pairs;
    int kind, match, mismatch, gap, gap_extend;
    bool local, want_end;
    bool semi;   // PWA_MODE_SG: every pair runs off the strips (band-less mini-stripe / stripe fills + the end-cell walk)
    bool affine() const { return kind == KIND_AFFINE; }
    bool nwdist() const { return kind == KIND_NWDIST; }
    const SubstTable* subst;   // KIND_SUBST: the checked table (match / mismatch unused), else null
    bool gotoh() const { return kind == KIND_GOTOH || kind == KIND_SUBST; }   // gap = gap_open, beside gap_extend; any mode, end cells allowed
    uint64_t len(uint32_t s) const { return seq_off[s + 1] - seq_off[s]; }
};

// PWA_DEBUG: host-side time between the phases of a batch's creation
struct CreateClock {
    pwa_ctx* ctx;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!ctx->knobs.debug) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[pwa] create: %-24s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
        if (ctx->knobs.probe) {   // how long does a kernel submission take at this point?
            hipLaunchKernelGGL(pwa_nop_kernel, dim3(1), dim3(64), 0, ctx->stream, (int*)nullptr);
            (void)hipStreamSynchronize(ctx->stream);
            const auto t2 = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[pwa]     probe after it: nop kernel + sync %8.3f ms\n", std::chrono::duration<double, std::milli>(t2 - now).count());
            t_last = t2;
        }
    }
};

struct LivePairs {
    std::vector<uint32_t> live;   // the pairs that reach a kernel (n > 0 and m > 0), ascending
    uint64_t max_n = 0, max_m = 0;
    bool any_trivial_score = false;
};

// One pass over the pair list: index check, and pairs with an empty side never reach a kernel (hw2.cpp: loops 138/205 do not
// run) -- they are resolved here, into b's host scores and end cells
int scan_pairs(pwa_ctx* ctx, pwa_batch* b, const BatchInput& in, LivePairs& lp) {
    b->host_scores.assign(in.n_pairs, 0);
    if (b->want_end) {
        b->host_end_i.assign(in.n_pairs, 0);
        b->host_end_j.assign(in.n_pairs, 0);
    }
    lp.live.resize(in.n_pairs);
    uint64_t n_live = 0;
    const int64_t gotoh_gaps = (int64_t)std::llabs((long long)in.gap) + std::llabs((long long)in.gap_extend);
    const int64_t gotoh_mx = in.subst ? std::max(in.subst->max_abs, gotoh_gaps) : max_abs({in.match, in.mismatch, gotoh_gaps});
    for (uint64_t k = 0; k < in.n_pairs; ++k) {
        if (in.pair_a[k] >= in.n_seq || in.pair_b[k] >= in.n_seq) return fail(ctx, PWA_E_INVALID, "pair index out of range");
        const uint64_t n = in.len(in.pair_a[k]), m = in.len(in.pair_b[k]);
        if (in.subst && (m > 0x7fffffc0ull || (long double)(n + m + 2) * (long double)gotoh_mx >= (long double)(1u << 28)))
            return fail(ctx, PWA_E_CAPACITY, "substitution-matrix scores out of range: (n + m + 2) * max(max |submat|, |gap_open| + |gap_extend|) must stay below 2^28");
        if (in.gotoh() && (m > 0x7fffffc0ull || (long double)(n + m + 2) * (long double)gotoh_mx >= (long double)(1u << 28)))
            return fail(ctx, PWA_E_CAPACITY, "gotoh scores out of range: (n + m + 2) * max(|match|, |mismatch|, |gap_open| + |gap_extend|) must stay below 2^28");
        if (n == 0 || m == 0) {
            if (in.gotoh()) {   // one gap of the whole other side: gap_open + L * gap_extend (SG: only the pattern's rows cost)
                const uint64_t L = in.local ? 0 : in.semi ? (m == 0 ? n : 0) : n + m;
                b->host_scores[k] = L == 0 ? 0 : (int32_t)((uint32_t)in.gap + (uint32_t)wrap_mul((int64_t)L, in.gap_extend));
            } else if (in.nwdist()) {   // hw4.cpp:21-28 + 146-152: an all-gap alignment, every column counts
                b->host_scores[k] = (int32_t)(n + m);
            } else if (in.affine()) {   // hw3.cpp:39-52: V[0][0] = 0, F[n][0] = Go + Ge(n-1), E[0][m] = Go + Ge(m-1)
                b->host_scores[k] = (n + m == 0) ? 0 : (int32_t)((uint32_t)in.gap + (uint32_t)wrap_mul((int64_t)(n + m - 1), in.gap_extend));
            } else if (in.semi) {
                b->host_scores[k] = wrap_mul((int64_t)n, in.gap);   // dp[n][0]; an empty pattern ends at (0, 0) with score 0
            } else if (!in.local) b->host_scores[k] = wrap_mul((int64_t)(n + m), in.gap);   // dp[n][0] / dp[0][m], hw2.cpp:125-136
            lp.any_trivial_score = lp.any_trivial_score || b->host_scores[k] != 0;
            if (b->want_end && !in.local) {
                b->host_end_i[k] = (uint32_t)n;
                b->host_end_j[k] = in.semi ? 0u : (uint32_t)m;
            }
            continue;
        }
        if (n > 0x7fffffc0ull || m > 0x7fffffc0ull) return fail(ctx, PWA_E_CAPACITY, "sequence longer than 2^31");
        lp.live[n_live++] = (uint32_t)k;
        b->cells += n * m;
        lp.max_n = std::max(lp.max_n, n);
        lp.max_m = std::max(lp.max_m, m);
    }
    lp.live.resize(n_live);
    return PWA_OK;
}

struct Alphabet {
    bool present[256];       // text symbols
    bool pattern_has[256];   // pattern symbols
    int code_of[256];        // -1: not a text symbol
    int n_alpha = 0;
    int absent_byte = -1;    // the smallest byte no text holds
    int text_pad_byte = -1;  // raw-byte (SC_CMP) form; the coded (SC_PERM) form uses code 6 when the alphabet leaves it free
};

Alphabet scan_alphabet(const BatchInput& in, const std::vector<uint8_t>& is_text) {
    Alphabet al;
    scan_bytes(in.seq_bytes, in.seq_off, in.n_seq, is_text, al.present, 8ull << 20);
    // LANES kernels also pad TEXTS (columns past a lane's own text): that symbol must match no pattern symbol and
    // must differ from the pattern pad, or padded rows would "match" padded columns.
    {
        std::vector<uint8_t> is_pat(in.n_seq, 0);
        for (uint64_t k = 0; k < in.n_pairs; ++k) is_pat[in.pair_a[k]] = 1;
        scan_bytes(in.seq_bytes, in.seq_off, in.n_seq, is_pat, al.pattern_has, 8ull << 20);
    }
    // codes: the text symbols that patterns use first, then the text-only ones (an N in the texts does not push a pattern symbol
    // past code 3, which the packed f16 cells need); symbols compare by equality only, so any order gives the same scores
    for (int v = 0; v < 256; ++v) {
        al.code_of[v] = -1;
        if (!al.present[v] && al.absent_byte < 0) al.absent_byte = v;
    }
    for (int pass = 0; pass < 2; ++pass)
        for (int v = 0; v < 256; ++v)
            if (al.present[v] && al.pattern_has[v] == (pass == 0)) al.code_of[v] = al.n_alpha++;
    for (int v = 255; v >= 0 && al.text_pad_byte < 0; --v)
        if (!al.pattern_has[v] && v != al.absent_byte) al.text_pad_byte = v;
    return al;
}

bool fits8(int v) { return v >= -128 && v <= 127; }

// How a batch's cells are stored and scored
struct CellForm {
    bool strips = false;              // the strip kernels can serve the list
    int kmode = BM_NW, score_path = SC_CMP;
    int tab_match = 0, tab_mismatch = 0;
    int32_t aff_go = 0, aff_ge = 0, aff_neg = 0;
    bool coded = false;               // the arena holds codes, not bytes
    bool mini_scores = false, mini_gap0 = false;
};

int choose_cell_form(pwa_ctx* ctx, const BatchInput& in, const LivePairs& lp, const Alphabet& al, CellForm& f) {
    const int match = in.match, mismatch = in.mismatch, gap = in.gap, gap_extend = in.gap_extend;
    const bool local = in.local, affine = in.affine(), nwdist = in.nwdist(), gotoh = in.gotoh();
    const uint64_t max_n = lp.max_n, max_m = lp.max_m;
    // ---- engine choice.  The strip engine pads short patterns with rows that match nothing; for SW
    // those rows can only hold values <= real rows if mismatch <= 0 and gap <= 0.
    // (semi-global: no strip form yet -- every pair takes the route of a pass with end cells)
    // (gotoh lists follow the linear rule, as a rule: NW and SW without end cells on the strips, gap terms are <= 0 there)
    // (a substitution table: always the band-less mini form -- the strips score by byte compare or a two-value table)
    f.strips = affine || nwdist || (!in.subst && !in.want_end && !in.semi && (!local || (mismatch <= 0 && gap <= 0)));
    f.kmode = local ? BM_SW : BM_NW;
    f.tab_match = match;
    f.tab_mismatch = mismatch;
    if (nwdist) {
        f.kmode = BM_DIST;
        f.tab_match = match - gap;       // the rows store H + gap: the diagonal consumer takes the gap back out
        f.tab_mismatch = mismatch - gap;
        if (al.n_alpha <= 7 && fits8(f.tab_match) && fits8(f.tab_mismatch)) f.score_path = SC_PERM;
        if (f.score_path == SC_CMP && al.absent_byte < 0)
            return fail(ctx, PWA_E_INVALID, "distance pass: the texts use all 256 byte values, no padding symbol left");
        // packed (H, dist) keys: dist in 12 bits, H in the 18 above (batch_nwdist.hip.h)
        if (max_n + max_m <= 4000 && (int64_t)(max_n + max_m + 2) * max_abs({match, mismatch, gap}) < 65536 && !ctx->knobs.no_packed_dist) {
            f.kmode = BM_DISTP;
            f.tab_match = match;       // the packed kernel takes hw4's own three scores
            f.tab_mismatch = mismatch;
        }
    } else if (affine) {
        // Ge(i+j)-shifted form when every value stays far inside int32 (the sentinels are -2^29 there)
        const bool shift_ok = (int64_t)(max_n + max_m + 4) * max_abs({match, mismatch, gap, gap_extend}) * 4 < (1ll << 27);
        f.kmode = shift_ok ? BM_AFFS : BM_AFF;
        f.aff_go = gap;
        f.aff_ge = gap_extend;
        f.aff_neg = shift_ok ? -(1 << 29) : std::numeric_limits<int32_t>::min() / 2;   // hw3.cpp:16
        if (shift_ok) {
            f.tab_match = match - 2 * gap_extend;
            f.tab_mismatch = mismatch - 2 * gap_extend;
        }
        if (al.n_alpha <= 7 && fits8(f.tab_match) && fits8(f.tab_mismatch)) f.score_path = SC_PERM;
        if (f.score_path == SC_CMP && al.absent_byte < 0)
            return fail(ctx, PWA_E_INVALID, "affine pass: the texts use all 256 byte values, no padding symbol left");
    } else if (gotoh) {
        if (f.strips) {
            // NW in ge (i + j)-shifted coordinates when every value stays far inside int32, as the hw3 form above; SW keeps the zero floor
            const bool shift_ok = !local && (int64_t)(max_n + max_m + 4) * max_abs({match, mismatch, gap, gap_extend}) * 4 < (1ll << 27);
            f.kmode = local ? BM_GSW : shift_ok ? BM_GNWS : BM_GNW;
            f.aff_go = gap;
            f.aff_ge = gap_extend;
            if (shift_ok) {
                f.tab_match = match - 2 * gap_extend;
                f.tab_mismatch = mismatch - 2 * gap_extend;
            }
            if (al.n_alpha <= 7 && fits8(f.tab_match) && fits8(f.tab_mismatch)) f.score_path = SC_PERM;
            if (f.score_path == SC_CMP && al.absent_byte < 0) f.strips = false;   // no byte left to pad with
        }
        // everything else: the band-less gotoh mini-stripe fills, on raw bytes, with their shape limit
        if (in.subst && max_n > kGotohMiniMaxN) return fail(ctx, PWA_E_CAPACITY, "substitution-matrix scores take patterns of at most 1024 symbols");
        if (!f.strips && max_n > kGotohMiniMaxN)
            return fail(ctx, PWA_E_CAPACITY, "gotoh scores off the strip kernels (semi-global, end cells, SW with mismatch > 0, texts with all 256 byte values) take patterns of at most 1024 symbols");
    } else if (f.strips) {
        if (!local) {
            // gap-shifted NW: G = H - g(i+j) needs every |value| to stay far inside int32
            const int64_t s_match = (int64_t)match - 2 * (int64_t)gap, s_mis = (int64_t)mismatch - 2 * (int64_t)gap;
            if ((int64_t)(max_n + max_m + 4) * max_abs({match, mismatch, gap}) * 4 < (1ll << 30) && fits8((int)s_match) && fits8((int)s_mis)) {
                f.kmode = BM_NWG;
                f.tab_match = (int)s_match;
                f.tab_mismatch = (int)s_mis;
            }
        }
        // (an alphabet of more than 7 symbols takes the compare path, which works in G space too)
        if (al.n_alpha <= 7 && fits8(f.tab_match) && fits8(f.tab_mismatch)) f.score_path = SC_PERM;
        if (f.score_path == SC_CMP && al.absent_byte < 0) f.strips = false;   // no byte left to pad with
    }
    // (a scores pass that wants end cells runs wholly off the strips: its arena is coded whenever the alphabet allows, for the mini-stripe
    // kernels -- the stripe engine's compare form is the same on codes, a pattern-only symbol is code 7 and equals no text code)
    const bool code_for_end_cells = (in.want_end || in.semi) && !affine && !nwdist && !gotoh && al.n_alpha <= 7 && ctx->knobs.tb_engine != 0;
    f.coded = (f.strips && f.score_path == SC_PERM) || code_for_end_cells;
    // Short patterns that a scores pass routes away from the strips run on the mini-stripe engine WITHOUT a band (mini_fill.hip.h,
    // BAND = false: four pairs per wave) where it applies: coded arena, keyed cells in range, table constants in a byte.
    if (f.coded && !affine && !nwdist && !gotoh && ctx->knobs.tb_engine != 0 && tb_range_ok(max_n + max_m, match, mismatch, gap, local ? 26 : 28)) {
        f.mini_scores = diag_keys_fit(match, mismatch, gap);
        f.mini_gap0 = f.mini_scores && !local && !in.semi && gap0_ok(max_n + max_m, match, mismatch, gap);
    }
    return PWA_OK;
}

// Device arena: every used sequence, 16-byte aligned, as symbols of the chosen coding; aoff[s]: where sequence s starts
int upload_arena(pwa_ctx* ctx, pwa_batch* b, const BatchInput& in, const std::vector<uint8_t>& is_used, uint64_t max_n, const CellForm& f,
                 const Alphabet& al, std::vector<uint64_t>& aoff) {
    aoff.assign(in.n_seq, 0);
    uint64_t arena_bytes = 0;
    for (uint32_t s = 0; s < in.n_seq; ++s)
        if (is_used[s]) {
            aoff[s] = arena_bytes;
            arena_bytes += align_up(in.len(s) + 1, 16);
        }
    arena_bytes += 512;   // slack: strips and text words are over-read, never over-used
    // (a strip task loads its lanes' pattern words for every strip of its LONGEST pattern and masks them after the load: a short pattern
    // is read up to that length past its start -- past the end of the arena when it lies last, which faulted on the device)
    if (f.strips) arena_bytes += align_up(max_n, 16);
    if (arena_bytes >= 0xffffffffull) return fail(ctx, PWA_E_CAPACITY, "sequence arena exceeds 4 GiB");
    uint8_t code8[256];
    for (int v = 0; v < 256; ++v) code8[v] = (uint8_t)(al.code_of[v] >= 0 ? al.code_of[v] : 7);
    HIPC(ctx, b->arena.alloc(ctx, arena_bytes));
    HIPC(ctx, build_arena(ctx, b->arena.p, arena_bytes, in.seq_bytes, in.seq_off, in.n_seq, is_used, aoff, f.coded ? code8 : nullptr,
                          !al.present[0] && !al.pattern_has[0]));
    return PWA_OK;
}

struct HostTask {
    uint32_t text, first, count;
    uint64_t maxlen;   // longest pattern of the task
    uint64_t m;        // text length (LANES: the longest text of the task)
};

// up to lanes_per_task patterns of one text per wave task
std::vector<HostTask> group_by_text(const BatchInput& in, const std::vector<uint32_t>& order, size_t lanes_per_task) {
    std::vector<HostTask> g;
    for (size_t p = 0; p < order.size();) {
        size_t q = p;
        while (q < order.size() && q - p < lanes_per_task && in.pair_b[order[q]] == in.pair_b[order[p]]) ++q;
        g.push_back({in.pair_b[order[p]], (uint32_t)p, (uint32_t)(q - p), in.len(in.pair_a[order[p]]), in.len(in.pair_b[order[p]])});
        p = q;
    }
    return g;
}

struct StripTasks {
    std::vector<uint32_t> order;   // pair indices, task by task
    std::vector<HostTask> ht;
    bool lanes = false;            // every lane its own text (LANES kernels)
};

// ---- wave tasks: pairs grouped by text, patterns sorted by length, 64 per wave
StripTasks plan_strip_tasks(pwa_ctx* ctx, const BatchInput& in, const std::vector<uint32_t>& live, const CellForm& f, const Alphabet& al) {
    StripTasks st;
    std::vector<uint32_t>& order = st.order;
    order = live;   // ascending pair index: the stable sorts below keep it as the last key
    {
        // text ascending, pattern length descending.  Stable counting sorts, least significant key first: two linear passes
        // per key, and the length pass is skipped when every pattern has the same length (a million-pair cross product:
        // ~3 ms [gpu box] against 14 ms for the 64-bit radix sort, which stays as the fallback for huge key ranges)
        uint64_t lmin = ~0ull, lmax = 0;
        for (const uint32_t k : order) {
            const uint64_t l = in.len(in.pair_a[k]);
            lmin = std::min(lmin, l);
            lmax = std::max(lmax, l);
        }
        // (the histograms have n_seq + 1 and lmax - lmin + 1 entries whatever the list's size: a short list over a large
        // FASTA index, or with one outlier length, is cheaper through the radix sort)
        if (lmax - lmin < (1u << 22) && in.n_seq <= (1u << 24) && (uint64_t)in.n_seq <= 4 * (uint64_t)order.size() + 65536 &&
            lmax - lmin <= 4 * (uint64_t)order.size() + 65536) {
            std::vector<uint32_t> tmp;
            if (lmax != lmin) counting_sort(order, tmp, (size_t)(lmax - lmin + 1), [&](uint32_t k) { return (size_t)(lmax - in.len(in.pair_a[k])); });
            counting_sort(order, tmp, (size_t)in.n_seq, [&](uint32_t k) { return (size_t)in.pair_b[k]; });
        } else {
            std::vector<uint64_t> key(order.size());   // text ascending, pattern length descending (lengths < 2^31)
            for (size_t o = 0; o < order.size(); ++o)
                key[o] = ((uint64_t)in.pair_b[order[o]] << 32) | (uint64_t)(0x7fffffffu - (uint32_t)in.len(in.pair_a[order[o]]));
            radix_sort_by_key(key, order);
        }
    }
    st.ht = group_by_text(in, order, 64);
    // ---- lists whose pairs share few texts (the reference's own loop pairs pattern i with reference i,
    // hw2.cpp:328-338) would leave most lanes of a text-grouped wave empty: give every lane its own text
    // instead (LANES kernels, local alignment only).  Pairs are sorted so that a wave's 64 pairs need about
    // the same number of strips and columns; a wave runs max(strips) x max(columns) of its lanes.
    bool kernels_have_lanes = false;
    size_t n_kernels = 0;
    const BatchKernelEntry* const kernels = batch_kernel_table(&n_kernels);
    for (size_t ki = 0; ki < n_kernels; ++ki) kernels_have_lanes |= (kernels[ki].fn_lanes != nullptr && kernels[ki].score == f.score_path);
    const bool text_pad_ok = f.score_path == SC_PERM ? al.n_alpha <= 6 : al.text_pad_byte >= 0;
    const bool underfilled = st.ht.size() * 64 > order.size() * 3 / 2 + 64;
    st.lanes = f.kmode == BM_SW && !in.affine() && !in.nwdist() && kernels_have_lanes && text_pad_ok && underfilled;
    // global alignment: right-aligned texts, front-padded with a code the table scores like a gap (batch_scores.hip.h).
    // Needs the gap-shifted form, a coded alphabet with codes 4..7 free, every pattern symbol inside it (a
    // pattern-only symbol shares code 7 with the pad rows), g <= 0 and -g in a table byte.
    bool patterns_inside = true;
    for (int v = 0; v < 256; ++v) patterns_inside = patterns_inside && (!al.pattern_has[v] || al.present[v]);
    const bool lanes_nw = f.kmode == BM_NWG && !in.affine() && !in.nwdist() && f.score_path == SC_PERM && al.n_alpha <= 4 && patterns_inside &&
                          in.gap <= 0 && fits8(-in.gap) && underfilled;
    st.lanes = st.lanes || lanes_nw;
    if (ctx->knobs.force_lanes >= 0) st.lanes = st.lanes && ctx->knobs.force_lanes != 0;   // experiments only
    if (st.lanes) {
        order = live;
        std::vector<uint64_t> key(order.size());   // nominal strips descending, then text length descending
        for (size_t o = 0; o < order.size(); ++o) {
            const uint64_t strips = (in.len(in.pair_a[order[o]]) + 75) / 76;
            key[o] = ((0x7fffffffull - strips) << 32) | (uint64_t)(0x7fffffffu - (uint32_t)in.len(in.pair_b[order[o]]));
        }
        radix_sort_by_key(key, order);
        st.ht.clear();
        for (size_t p = 0; p < order.size(); p += 64) {
            const size_t q = std::min(order.size(), p + 64);
            uint64_t mn = 0, mm = 0;
            for (size_t o = p; o < q; ++o) {
                mn = std::max(mn, in.len(in.pair_a[order[o]]));
                mm = std::max(mm, in.len(in.pair_b[order[o]]));
            }
            st.ht.push_back({in.pair_b[order[p]], (uint32_t)p, (uint32_t)(q - p), mn, mm});
        }
    }
    return st;
}

struct StripHeight {
    int R = 0, mode = 0;      // R = 0: no kernel instantiation
    long double cost = -1;
};

// ---- strip height: least padded work, ties to the taller strip.  c16: the packed f16 form (two pairs per lane, 128-slot tasks),
// priced per lane row at kCell16Vpr VALU for both pairs
StripHeight choose_strip_height(const std::vector<HostTask>& tl, const CellForm& f, bool lanes, bool c16, const Knobs& knobs) {
    StripHeight best;
    best.mode = f.kmode;
    size_t n_kernels = 0;
    const BatchKernelEntry* const kernels = batch_kernel_table(&n_kernels);
    const int force = knobs.force_r, force_mode = knobs.force_mode;   // experiments only
    for (size_t ki = 0; ki < n_kernels; ++ki) {
        const BatchKernelEntry& e = kernels[ki];
        // SW has two forms: BM_SW (R registers per lane, 5.0 VALU per cell) and BM_SWS (2R registers, 4.06)
        const bool mode_ok = e.mode == f.kmode || (f.kmode == BM_SW && e.mode == BM_SWS);
        if (!mode_ok || e.score != f.score_path) continue;
        if (lanes && !e.fn_lanes) continue;
        if (c16 && !e.fn_cell16) continue;
        const int R = e.R;
        if (force && force != R) continue;
        if (force_mode >= 0 && force_mode != e.mode) continue;
        long double w = c16 ? (long double)kCell16Vpr : e.mode == BM_SWS ? 4.06L : (e.mode == BM_SW ? 5.02L : 1.0L);   // VALU per lane row
        // affine strips of more than 40 rows run 2 instead of 3 waves per SIMD: [gpu] all pairs of 1024 x 1000 take
        // 93.2 ms at R = 52 against 89.2 ms at R = 32 for the same padded cells
        // (the gotoh strips hold three values per row like them and share affine_waves_per_simd: the same height table)
        if ((e.mode == BM_AFF || e.mode == BM_AFFS || e.mode == BM_GNW || e.mode == BM_GNWS || e.mode == BM_GSW) && R > 40) w *= 1.045L;
        // evaluated cells + the strip hand-off priced at ~2 cells per column and strip boundary ([gpu]: the
        // 1000-row affine pass is equally fast at R = 32 and 52 but moves 37 % fewer HBM bytes at 52)
        long double cost = 0;
        for (const auto& t : tl) {
            const uint64_t strips = (t.maxlen + R - 1) / R;
            cost += (long double)(strips * R + 2 * (strips - 1)) * (long double)t.m * 64.0L;
        }
        cost *= w;
        if (best.cost < 0 || cost < best.cost || (cost == best.cost && R > best.R)) {
            best.cost = cost;
            best.R = R;
            best.mode = e.mode;
        }
    }
    return best;
}

// ---- packed f16 cells (batch_scores.hip.h, CELL16): local scores over a coded arena whose pattern symbols all have codes 0..3,
// pad rules of the int32 strips (mismatch, gap <= 0), scores in a byte, and every value k * 2^-11 with |k| <= 2047 exact in f16:
// H <= longest pattern * max(match, 0) bounds all of them.  Everything else keeps the int32 kernels, bit for bit.
bool cell16_admitted(const Knobs& knobs, const BatchInput& in, const CellForm& f, const Alphabet& al, bool lanes, uint64_t max_n) {
    bool pats_low = true;
    for (int v = 0; v < 256; ++v) pats_low = pats_low && (!al.pattern_has[v] || (al.present[v] && al.code_of[v] <= 3));
    return in.local && f.kmode == BM_SW && !in.affine() && !in.nwdist() && f.score_path == SC_PERM && !lanes && pats_low &&
           in.mismatch <= 0 && in.gap <= 0 && max_abs({in.match, in.mismatch, in.gap}) <= 127 && (int64_t)max_n * std::max(in.match, 0) <= 2047 &&
           knobs.cell16 != 0 && (knobs.force_mode < 0 || knobs.force_mode == BM_SWS);
}

// ---- the profile form of the packed cells (PROF16): CELL16's admission, patterns of at most kProf16R rows, and every code of the
// arena in 0..3 (its profile tables have four text codes; 12 is the text pad).  Pairs are grouped by pattern, 128 to a wave task,
// texts longest first so that a task's columns are about its lanes' own.
bool prof16_admitted(const Knobs& knobs, const Alphabet& al, uint64_t max_n) {
    bool codes_low = true;
    for (int v = 0; v < 256; ++v) codes_low = codes_low && (!al.present[v] || al.code_of[v] <= 3);
    return knobs.prof16 != 0 && codes_low && max_n <= (uint64_t)kProf16R;
}

// ---- PROF16's integer-coded row: H >= 0 stored as an integer per half and s' = s - gap added with one 32-bit add, which needs every
// s' >= 0 (mismatch <= match is not assumed).  Everything else is PROF16's own admission: H <= 2047 and s' <= 254 keep a half below
// 2^16 (no carry into the other pair) and below 0x7c00 (ordered like its f16 reading).  Priced like the f16 row (kProf16Vpr): the
// same 3.5 instructions per lane row, and no routing decision sits near enough to move.
bool prof16_int_admitted(const Knobs& knobs, const BatchInput& in) {
    return knobs.prof16_int != 0 && in.mismatch - in.gap >= 0 && in.match - in.gap >= 0;
}

std::vector<HostTask> group_by_pattern(const BatchInput& in, std::vector<uint32_t>& order) {
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        if (in.pair_a[x] != in.pair_a[y]) return in.pair_a[x] < in.pair_a[y];
        return in.len(in.pair_b[x]) > in.len(in.pair_b[y]);
    });
    std::vector<HostTask> g;
    for (size_t p = 0; p < order.size();) {
        size_t q = p;
        while (q < order.size() && q - p < 128 && in.pair_a[order[q]] == in.pair_a[order[p]]) ++q;
        g.push_back({in.pair_a[order[p]], (uint32_t)p, (uint32_t)(q - p), in.len(in.pair_a[order[p]]), in.len(in.pair_b[order[p]])});
        p = q;
    }
    return g;
}

long double prof16_cost(const std::vector<HostTask>& tl) {   // in choose_strip_height's units
    long double cost = 0;
    for (const auto& t : tl) cost += (long double)prof16_rows(t.maxlen) * (long double)((t.m + 7) / 8 * 8) * 64.0L;
    return cost * (long double)kProf16Vpr;
}

// Whether the cost-based split below applies.  Linear scores always.  hw4 distances take it when the batch is in the two-value form
// (some n + m > 4000, or PWA_NO_PACKED_DIST): coded arena, keys H * 4 + prio inside int32 (pair_dist.hip.h).  Packed-form lists, other
// byte alphabets and larger scores stay on the strips.  hw3 affine scores likewise: coded arena, every real value inside +-2^28 so that
// the -2^29 sentinels never win (pair_affine.hip.h).  Raw-byte alphabets and scorings large enough for the reference's own
// wrap-around to matter stay on the strips.
bool route_eligible(const BatchInput& in, const CellForm& f, uint64_t max_n, uint64_t max_m) {
    if (in.gotoh()) return false;   // routing is a rule for them (choose_cell_form); work-aware routing: DESIGN.md §9
    if (in.nwdist())
        return f.kmode == BM_DIST && f.score_path == SC_PERM && (int64_t)(max_n + max_m + 2) * max_abs({in.match, in.mismatch, in.gap, 1}) < (1ll << 28);
    if (in.affine())
        return f.score_path == SC_PERM &&
               (int64_t)(max_n + max_m + 2) * max_abs({in.match, in.mismatch, std::llabs((long long)in.gap) + std::llabs((long long)in.gap_extend), 1}) < (1ll << 28);
    return true;
}

// Route estimates of a pass kind: the strips' VALU per cell; and the stripe engine's, in the units of the estimate (stripes of
// choose_geom's geometry): ns per stripe step and SIMD with the chip full, us of pipeline lag per stripe, ns per step of a pair alone
struct RouteCost {
    double valu_per_cell, step_ns, lag_us, lone_step_ns;
};

RouteCost route_cost(const BatchInput& in, const CellForm& f, bool cell16, int strip_mode) {
    // the distance fill (pair_dist.hip.h), [gpu] profiles/hw4_long_route_probe.txt: 496 pairs 10k x 10k 29.9 ms; one pair 10k x 10k
    // 2.66 ms, 20k x 20k 5.29 ms
    if (in.nwdist()) return {10.75, 80.0, 13.0, 162.0};
    // the affine score fill (pair_affine.hip.h), [gpu] profiles/hw3_long_route_probe.txt: 496 pairs 10k x 10k 23.4 ms; one pair
    // 10k x 10k 1.62 ms, 20k x 20k 3.21 ms; affine strips: 5.6 VALU per cell, PMC of profiles/r03_hw3_rocprof_summary.md
    if (in.affine()) return {5.6, 62.0, 8.0, 99.0};
    // linear scores: the keyed chunk without a band (coded arena, keys in range) or the plain step ([gpu] r03_route_probe.txt: one
    // 10k x 10k pair 1.26 / 1.01 ms, 64 pairs 3.45 / 2.05 ms)
    const double vpc = cell16 ? kCell16Vpr : (strip_mode == BM_SWS ? 4.06 : strip_mode == BM_SW ? 5.02 : strip_mode == BM_NWG ? 2.53 : 4.5) + (f.score_path == SC_CMP ? 2.0 : 0.0);
    if (f.mini_scores) return {vpc, in.local ? 70.0 : 42.0, 9.0, in.local ? 55.0 : 30.0};
    return {vpc, in.local ? 105.0 : 75.0, 9.0, 100.0};
}

// ---- work-aware routing (r03).  The strip engine is the cheaper one per cell (lane = pair, 2.5 - 5 VALU per cell) but a wave
// task is one wave running strips x columns on its own: a list of few long pairs -- ONE 10k x 10k pair is 105 strips x 2500
// column blocks x 1560 instructions on one lane of one wave, [gpu] 779 ms against 1.67 ms on the stripe engine -- or of few
// wave tasks (4096 pairs 150 x 10k = 64 tasks: 11.6 ms against 4.3 ms) leaves the chip idle.  The stripe engine spreads a
// pair over ceil(n / (64 RL)) waves that sweep anti-diagonals (~100 ns per step of 64 RL cells per SIMD).  Both costs are
// estimated from the task list with constants measured on the GPU (profiles/r03_route_probe.txt), tasks are moved to the
// stripe engine in two candidate orders (largest strip task first; cheapest-to-move per unit of strip work first) and
// the split with the smallest estimated total -- the two launches run one after the other on the run's stream -- wins.
// Pairs are independent (hw2.cpp:328-338) and both engines are exact, so a split changes no result.
// Returns the tasks (indices into st.ht) to move to the stripe engine.
std::vector<uint32_t> tasks_to_move(const pwa_ctx* ctx, const BatchInput& in, const StripTasks& st, int R, uint64_t task_lanes,
                                    const RouteCost& rc, bool mini_scores) {
    const std::vector<HostTask>& ht = st.ht;
    const size_t nt0 = ht.size();
    constexpr double kLoneNs = 1.9, kSimdNs = 1.63;                                 // ns per wave instruction: one wave alone / a SIMD with two
    const double kSimds = 4.0 * ctx->num_cu;
    std::vector<double> I(nt0), S(nt0), L(nt0);   // strip instructions / stripe-side work (ns x SIMD) / longest single-pair latency (us) of a task
    double I_total = 0, I_max = 0;
    uint64_t filled = 0;
    for (size_t t = 0; t < nt0; ++t) {
        const uint64_t strips = (ht[t].maxlen + R - 1) / R;
        I[t] = (double)strips * (double)((ht[t].m + 3) / 4) * (4.0 * R * rc.valu_per_cell);
        I_total += I[t];
        I_max = std::max(I_max, I[t]);
        filled += ht[t].count;
    }
    // nothing to route when the strips' waves are many, full, and none of them dominates: per cell the strips are the cheapest engine
    // by 2x and more, so no task can gain by leaving (and the per-pair estimates below cost ~3 ms for a million pairs)
    const bool strips_fit = (double)nt0 >= 4 * kSimds && filled * 10 >= (uint64_t)nt0 * task_lanes * 9 && I_max * kLoneNs * 4 < I_total / kSimds * kSimdNs &&
                            ctx->knobs.scores_route < 0;
    for (size_t t = 0; t < nt0 && !strips_fit; ++t) {
        double steps = 0, lat = 0;
        for (uint32_t l = 0; l < ht[t].count; ++l) {
            const uint32_t k = st.order[ht[t].first + l];
            const uint64_t n = in.len(in.pair_a[k]), m = in.len(in.pair_b[k]);
            if (const int mrl = mini_scores ? mini_rl_for(n) : 0) {   // mini-stripe engine, no band: a quarter of a wave, (17 + 5 | 7.3 RL) instructions per step
                const double mstep = (17.0 + (in.local ? 7.3 : 5.0) * mrl) * 1.37;   // [gpu] 92 ns per step for RL = 10, global (tools/probes/mini_mix.hip)
                steps += (double)(m + 15) * mstep / 4.0 / 1.5;                    // (two waves per SIMD: ~1.9 x one wave's throughput)
                lat = std::max(lat, (double)(m + 15) * mstep * 1e-3);
                continue;
            }
            const PairGeom g = choose_geom(ctx->knobs, n);
            const double stripes = (double)((n + 64 * g.rl - 1) / (64 * g.rl));
            steps += stripes * (double)(m + 63) * rc.step_ns;
            lat = std::max(lat, stripes * rc.lag_us + (double)(m + 63) * rc.lone_step_ns * 1e-3);
        }
        S[t] = steps;
        L[t] = lat;
    }
    auto evaluate = [&](const std::vector<uint32_t>& ord, size_t& best_k) -> double {
        // tasks ord[0 .. k-1] move; suffix maxima of I over the tasks that stay
        std::vector<double> sufmax(nt0 + 1, 0.0);
        for (size_t k = nt0; k-- > 0;) sufmax[k] = std::max(sufmax[k + 1], I[ord[k]]);
        double best_t = -1, moved_I = 0, moved_S = 0, moved_L = 0;
        for (size_t k = 0; k <= nt0; ++k) {
            const double ts = std::max(sufmax[k] * kLoneNs, (I_total - moved_I) / kSimds * kSimdNs) * 1e-3;              // us
            const double tp = k ? std::max(moved_L, moved_S / kSimds * 1e-3) + 15.0 : 0.0;                                 // us (+ two more launches)
            const double tt = ts + tp;
            if (best_t < 0 || tt < best_t) {
                best_t = tt;
                best_k = k;
            }
            if (k < nt0) {
                moved_I += I[ord[k]];
                moved_S += S[ord[k]];
                moved_L = std::max(moved_L, L[ord[k]]);
            }
        }
        return best_t;
    };
    std::vector<uint32_t> ordA(nt0), ordB(nt0);
    std::iota(ordA.begin(), ordA.end(), 0u);
    ordB = ordA;
    if (!strips_fit) {
        std::stable_sort(ordA.begin(), ordA.end(), [&](uint32_t x, uint32_t y) { return I[x] > I[y]; });
        std::stable_sort(ordB.begin(), ordB.end(), [&](uint32_t x, uint32_t y) { return S[x] * I[y] < S[y] * I[x]; });   // S / I ascending
    }
    size_t kA = 0, kB = 0;
    const double tA = strips_fit ? 0.0 : evaluate(ordA, kA), tB = strips_fit ? 0.0 : evaluate(ordB, kB);
    std::vector<uint32_t>& ord = tA <= tB ? ordA : ordB;
    size_t kmove = strips_fit ? 0 : (tA <= tB ? kA : kB);
    if (ctx->knobs.scores_route == 1) kmove = nt0;   // tests: everything (eligible) on the stripe engine
    if (ctx->knobs.debug) std::fprintf(stderr, "[pwa] route: %zu of %zu wave tasks to the stripe engine (estimates: all on strips %.1f us, split %.1f us)\n",
                                       kmove, nt0, std::max(*std::max_element(I.begin(), I.end()) * kLoneNs, I_total / kSimds * kSimdNs) * 1e-3, std::min(tA, tB));
    ord.resize(kmove);
    return std::move(ord);
}

// Takes the moved tasks out of st.ht; returns their pairs, ascending
std::vector<uint32_t> split_tasks(StripTasks& st, const std::vector<uint32_t>& move) {
    std::vector<uint8_t> moved(st.ht.size(), 0);
    for (const uint32_t t : move) moved[t] = 1;
    std::vector<HostTask> keep;
    std::vector<uint32_t> pair_list;
    for (size_t t = 0; t < st.ht.size(); ++t) {
        if (!moved[t]) {
            keep.push_back(st.ht[t]);
            continue;
        }
        for (uint32_t l = 0; l < st.ht[t].count; ++l) pair_list.push_back(st.order[st.ht[t].first + l]);
    }
    st.ht.swap(keep);
    std::sort(pair_list.begin(), pair_list.end());
    return pair_list;
}

// The strip kernel a batch launches, chosen once: the occupancy query and pwa_batch_run both take this one
void* strip_kernel_fn(const BatchKernelEntry& e, const BatchInput& in, bool cell16, bool lanes, bool single) {
    if (in.nwdist()) return reinterpret_cast<void*>(e.dfn);
    if (in.affine() || in.gotoh()) return reinterpret_cast<void*>(e.afn);
    const batch_kernel_t fn = cell16  ? (single ? e.fn_cell16_single : e.fn_cell16)
                              : lanes ? (single ? e.fn_lanes_single : e.fn_lanes)
                                      : (single && e.fn_single ? e.fn_single : e.fn);
    return reinterpret_cast<void*>(fn);
}

// Right-aligned, front-padded (code 4) text rows of a LANES global batch: task t, lane l at t_base + l * M_t, M_t = 4 * ceil(max m / 4)
int upload_lane_rows(pwa_ctx* ctx, pwa_batch* b, const BatchInput& in, const Alphabet& al, const StripTasks& st, BatchTask* tasks, uint32_t* stoff) {
    const std::vector<HostTask>& ht = st.ht;
    const size_t nt = ht.size();
    uint64_t total = 0;
    std::vector<uint64_t> tbase(nt);
    for (size_t t = 0; t < nt; ++t) {
        tbase[t] = total;
        total += 64ull * ((ht[t].m + 3) / 4 * 4);
    }
    if (total + 64 >= (ctx->knobs.lane_rows_limit ? ctx->knobs.lane_rows_limit : 0xffffffffull))
        return fail(ctx, PWA_E_CAPACITY, "per-lane text rows exceed 4 GiB");   // (one-shot calls halve the run and retry)
    // The rows are built straight in the context's two page-locked arena buffers, in pieces of whole tasks (~32 MiB), by several host
    // threads, while the previous piece is on its way (copy stream) -- like build_arena.  (Until r03: one thread, byte by byte into a
    // heap buffer, then through the bounce buffer: 156 ms of a 159 ms call for 131 072 pairs 150 x 2000.)
    HIPC(ctx, b->lane_text.alloc(ctx, total + 64));
    uint8_t code8[256];
    for (int v = 0; v < 256; ++v) code8[v] = (uint8_t)al.code_of[v];
    constexpr uint64_t kPiece = 32ull << 20;
    auto task_end = [&](size_t t) { return t + 1 < nt ? tbase[t + 1] : total + 64; };   // (the slack after the last task is pad as well)
    int piece = 0;
    for (size_t t0 = 0; t0 < nt; ++piece) {
        size_t t1 = t0 + 1;
        while (t1 < nt && task_end(t1) - tbase[t0] <= kPiece) ++t1;
        const uint64_t base = tbase[t0], bytes = task_end(t1 - 1) - base;
        PinnedBuf& pb = ctx->pin[pwa_ctx::PIN_ARENA + (piece & 1)];
        if (piece >= 2) HIPC(ctx, hipEventSynchronize(ctx->copy_ev[piece & 1]));   // the copy that last read this buffer
        HIPC(ctx, pb.reserve(bytes));
        uint8_t* const host = pb.as<uint8_t>();
        const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>({16, bytes / (1ull << 20) + 1, std::max(1u, std::thread::hardware_concurrency()), (uint64_t)(t1 - t0)}));
        auto work = [&](int th) {
            const size_t a = t0 + (t1 - t0) * (size_t)th / (size_t)T, z = t0 + (t1 - t0) * (size_t)(th + 1) / (size_t)T;
            for (size_t t = a; t < z; ++t) {
                const uint64_t M = (ht[t].m + 3) / 4 * 4;
                std::memset(host + (tbase[t] - base), 4, task_end(t) - tbase[t]);
                tasks[t].text_len = (uint32_t)M;
                for (uint32_t l = 0; l < ht[t].count; ++l) {
                    const uint32_t k = st.order[ht[t].first + l];
                    const uint8_t* src = in.seq_bytes + in.seq_off[in.pair_b[k]];
                    const uint64_t len = in.len(in.pair_b[k]);
                    uint8_t* dst = host + (tbase[t] - base) + (uint64_t)l * M + (M - len);
                    for (uint64_t o = 0; o < len; ++o) dst[o] = code8[src[o]];
                    stoff[t * 64 + l] = (uint32_t)(tbase[t] + (uint64_t)l * M);
                }
            }
        };
        std::vector<std::thread> pool;
        for (int th = 1; th < T; ++th) pool.emplace_back(work, th);
        work(0);
        for (auto& x : pool) x.join();
        HIPC(ctx, hipMemcpyAsync(b->lane_text.as<uint8_t>() + base, host, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
        HIPC(ctx, hipEventRecord(ctx->copy_ev[piece & 1], ctx->copy_stream));
        t0 = t1;
    }
    HIPC(ctx, hipStreamSynchronize(ctx->copy_stream));
    return PWA_OK;
}

// The strips that stay: slot arrays, lane text rows, the kernel, the hand-off workspace and BatchParams
int setup_strips(pwa_ctx* ctx, pwa_batch* b, const BatchInput& in, const CellForm& f, const Alphabet& al, const std::vector<uint64_t>& aoff,
                 StripTasks& st, const StripHeight& h, uint64_t max_m, CreateClock& clock) {
    std::vector<HostTask>& ht = st.ht;
    const int kmode = h.mode, R = h.R;
    const uint64_t kTaskLanes = b->cell16 ? 128 : 64;   // lane slots per wave task
    const bool own_texts = b->lanes || b->prof16;   // per-slot text arrays
    for (const auto& t : ht)
        b->padded_cells += b->prof16 ? prof16_rows(t.maxlen) * ((t.m + 7) / 8 * 8) * kTaskLanes
                                     : (t.maxlen + R - 1) / R * R * (b->lanes ? (t.m + 3) / 4 * 4 : t.m) * kTaskLanes;
    b->kern = find_batch_kernel(R, kmode, f.score_path);
    if (!b->kern) return fail(ctx, PWA_E_INVALID, "internal: no kernel instantiation");
    b->kernel_name = b->kern->name;
    std::sort(ht.begin(), ht.end(), [&](const HostTask& x, const HostTask& y) {   // longest first
        const uint64_t cx = b->prof16 ? x.m : (x.maxlen + R - 1) / R * x.m, cy = b->prof16 ? y.m : (y.maxlen + R - 1) / R * y.m;
        if (cx != cy) return cx > cy;
        return x.first < y.first;
    });
    const size_t nt = ht.size();
    // task list and lane slots are built in page-locked buffers of the context and uploaded from there (see PinnedBuf)
    HIPC(ctx, ctx->pin[pwa_ctx::PIN_TASKS].reserve(nt * sizeof(BatchTask)));
    for (int q = 0; q < (own_texts ? 5 : 3); ++q) HIPC(ctx, ctx->pin[pwa_ctx::PIN_SLOT0 + q].reserve(nt * kTaskLanes * sizeof(uint32_t)));
    BatchTask* const tasks = ctx->pin[pwa_ctx::PIN_TASKS].as<BatchTask>();
    uint32_t* const spoff = ctx->pin[pwa_ctx::PIN_SLOT0].as<uint32_t>();
    uint32_t* const splen = ctx->pin[pwa_ctx::PIN_SLOT1].as<uint32_t>();
    uint32_t* const sout = ctx->pin[pwa_ctx::PIN_SLOT2].as<uint32_t>();
    uint32_t* const stoff = own_texts ? ctx->pin[pwa_ctx::PIN_SLOT3].as<uint32_t>() : nullptr;   // empty lanes: no text, no pattern
    uint32_t* const stlen = own_texts ? ctx->pin[pwa_ctx::PIN_SLOT4].as<uint32_t>() : nullptr;
    std::memset(tasks, 0, nt * sizeof(BatchTask));
    std::memset(spoff, 0, nt * kTaskLanes * sizeof(uint32_t));
    std::memset(splen, 0, nt * kTaskLanes * sizeof(uint32_t));
    std::memset(sout, 0xff, nt * kTaskLanes * sizeof(uint32_t));
    if (own_texts) {
        std::memset(stoff, 0, nt * kTaskLanes * sizeof(uint32_t));
        std::memset(stlen, 0, nt * kTaskLanes * sizeof(uint32_t));
    }
    uint32_t max_strips = 1;
    {   // (a million slots through three indirections each: on a few threads for long task lists)
        const int T = (int)std::max<size_t>(1, std::min<size_t>({8, std::max(1u, std::thread::hardware_concurrency()), nt >> 11}));
        std::vector<uint32_t> part_max((size_t)T, 1);
        auto work = [&](int th) {
            const size_t a = nt * (size_t)th / (size_t)T, z = nt * (size_t)(th + 1) / (size_t)T;
            for (size_t t = a; t < z; ++t) {
                tasks[t].text_off = (uint32_t)aoff[ht[t].text];
                tasks[t].text_len = (uint32_t)ht[t].m;
                tasks[t].slot0 = (uint32_t)(t * kTaskLanes);
                tasks[t].n_strips = (uint32_t)((ht[t].maxlen + R - 1) / R);
                part_max[(size_t)th] = std::max(part_max[(size_t)th], tasks[t].n_strips);
                if (b->prof16) {   // PROF16's task: the pattern's arena offset and length, the longest text
                    tasks[t].n_strips = (uint32_t)ht[t].maxlen;
                    part_max[(size_t)th] = 1;
                }
                for (uint32_t l = 0; l < ht[t].count; ++l) {
                    const uint32_t k = st.order[ht[t].first + l];
                    spoff[t * kTaskLanes + l] = (uint32_t)aoff[in.pair_a[k]];
                    splen[t * kTaskLanes + l] = (uint32_t)in.len(in.pair_a[k]);
                    sout[t * kTaskLanes + l] = k;
                    if (own_texts) {
                        stoff[t * kTaskLanes + l] = (uint32_t)aoff[in.pair_b[k]];
                        stlen[t * kTaskLanes + l] = (uint32_t)in.len(in.pair_b[k]);
                    }
                }
                // PROF16: an empty slot streams the task's shortest text (its last: group_by_pattern), so that the kernel's unmasked
                // loads, which go by the shortest text of all 128 slots, stay inside a text in every lane
                for (uint32_t l = ht[t].count; b->prof16 && ht[t].count > 0 && l < kTaskLanes; ++l) {
                    stoff[t * kTaskLanes + l] = stoff[t * kTaskLanes + ht[t].count - 1];
                    stlen[t * kTaskLanes + l] = stlen[t * kTaskLanes + ht[t].count - 1];
                }
            }
        };
        std::vector<std::thread> pool;
        for (int th = 1; th < T; ++th) pool.emplace_back(work, th);
        work(0);
        for (auto& x : pool) x.join();
        for (int th = 0; th < T; ++th) max_strips = std::max(max_strips, part_max[(size_t)th]);
    }
    if (b->lanes && kmode == BM_NWG) {
        const int rc = upload_lane_rows(ctx, b, in, al, st, tasks, stoff);
        if (rc != PWA_OK) return rc;
    }
    if (own_texts) {
        HIPC(ctx, b->slot_toff.alloc(ctx, nt * kTaskLanes * 4));
        HIPC(ctx, hipMemcpy(b->slot_toff.p, stoff, nt * kTaskLanes * 4, hipMemcpyHostToDevice));
        HIPC(ctx, b->slot_tlen.alloc(ctx, nt * kTaskLanes * 4));
        HIPC(ctx, hipMemcpy(b->slot_tlen.p, stlen, nt * kTaskLanes * 4, hipMemcpyHostToDevice));
    }
    clock.mark("choose R + slot arrays");
    HIPC(ctx, b->tasks.alloc(ctx, nt * sizeof(BatchTask)));
    HIPC(ctx, hipMemcpy(b->tasks.p, tasks, nt * sizeof(BatchTask), hipMemcpyHostToDevice));
    HIPC(ctx, b->slot_poff.alloc(ctx, nt * kTaskLanes * 4));
    HIPC(ctx, hipMemcpy(b->slot_poff.p, spoff, nt * kTaskLanes * 4, hipMemcpyHostToDevice));
    HIPC(ctx, b->slot_plen.alloc(ctx, nt * kTaskLanes * 4));
    HIPC(ctx, hipMemcpy(b->slot_plen.p, splen, nt * kTaskLanes * 4, hipMemcpyHostToDevice));
    HIPC(ctx, b->slot_out.alloc(ctx, nt * kTaskLanes * 4));
    HIPC(ctx, hipMemcpy(b->slot_out.p, sout, nt * kTaskLanes * 4, hipMemcpyHostToDevice));

    if (b->lanes) b->kernel_name = std::string(b->kernel_name).insert(b->kernel_name.size() - 1, ",LANES");
    b->strip_fn = strip_kernel_fn(*b->kern, in, b->cell16, b->lanes, max_strips == 1);
    if (b->prof16) b->strip_fn = reinterpret_cast<void*>(b->prof16_int ? b->kern->fn_prof16_int : b->kern->fn_prof16);   // (the reported name stays the CELL16 entry's)
    int per_cu = 0;
    HIPC(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, b->strip_fn, 64, 0));
    per_cu = std::max(1, std::min(per_cu, 32));
    b->grid = (uint32_t)std::min<uint64_t>(nt, (uint64_t)ctx->num_cu * per_cu);
    // int32 per half: one (affine: two) int4 per lane per 4-column block
    const int hand_vals = (in.affine() || in.gotoh() || (in.nwdist() && kmode != BM_DISTP)) ? 2 : 1;   // int4 per lane per 4-column block
    const uint64_t half = (max_strips > 1 ? ((max_m + 3) / 4 + 1) * 256 : 256) * hand_vals;
    // Strip s reads the half written by strip s-1 and writes the other one.  With at most two strips per task
    // the second half is only ever the parked dummy block (stride 0), so it is one block long: for C3 that
    // turns a 10.5 GB workspace (0.24 s of hipMalloc, profiles/r01_malloc_probe.txt) into 5.2 GB (0.3 ms).
    const uint64_t block_ints = 256 * hand_vals;
    const uint64_t second = max_strips > 2 ? half : block_ints;
    {   // very long texts: fewer workgroups rather than a workspace that does not fit (tasks come off a queue,
        // any grid is correct)
        size_t free_b = 0, total_b = 0;
        HIPC(ctx, hipMemGetInfo(&free_b, &total_b));
        const uint64_t per_wg = (half + second) * sizeof(int32_t);
        const uint64_t fit = std::max<uint64_t>(1, (uint64_t)(free_b * 0.6) / per_wg);
        b->grid = (uint32_t)std::min<uint64_t>(b->grid, fit);
        b->grid = (b->grid + 3u) & ~3u;   // whole four-wave workgroups (pwa_batch_run): every wave has a hand-off region of its own
    }
    HIPC(ctx, b->hand.alloc_hand(ctx, (size_t)b->grid * (half + second) * sizeof(int32_t)));   // (the one an earlier batch of this context left behind, if it is big enough)

    clock.mark("uploads + workspace");
    BatchParams& P = b->bp;
    P.arena = b->arena.as<uint8_t>();
    P.tasks = b->tasks.as<BatchTask>();
    P.slot_poff = b->slot_poff.as<uint32_t>();
    P.slot_plen = b->slot_plen.as<uint32_t>();
    P.slot_out = b->slot_out.as<uint32_t>();
    P.scores = b->scores.as<int32_t>();
    P.hand = b->hand.as<int32_t>();
    P.hand_stride = half + second;
    P.hand_half = (uint32_t)half;
    P.queue = b->queue.as<uint32_t>();
    P.n_tasks = (uint32_t)nt;
    P.match = f.tab_match;
    P.mismatch = f.tab_mismatch;
    P.gap = in.gap;
    const uint32_t bm = (uint8_t)(int8_t)f.tab_match, bx = (uint8_t)(int8_t)f.tab_mismatch;
    P.tab_lo = bm | (bx << 8) | (bx << 16) | (bx << 24);   // selector 0 -> match
    P.tab_hi = bx * 0x01010101u;                           // selectors 4..7 -> mismatch
    const uint32_t pad = (f.score_path == SC_PERM) ? 7u : (uint32_t)al.absent_byte;
    P.pad_word = pad * 0x01010101u;
    P.tpad_word = ((f.score_path == SC_PERM) ? 6u : (uint32_t)std::max(al.text_pad_byte, 0)) * 0x01010101u;
    P.lane_text = b->lane_text.as<uint8_t>();
    if (b->lanes && kmode == BM_NWG) P.tab_hi = (uint32_t)(uint8_t)(int8_t)(-in.gap) * 0x01010101u;   // selectors 4..7: front pad = a gap column
    if (b->cell16) {   // f16 bit patterns of s * 2^-11 (exact: |s| <= 127)
        const uint32_t m16 = f16_bits_scaled(in.match), x16 = f16_bits_scaled(in.mismatch), g16 = f16_bits_scaled(in.gap);
        P.lo16_base = (x16 & 0xffu) * 0x01010101u;
        P.lo16_diff = (m16 ^ x16) & 0xffu;
        P.hi16_base = (x16 >> 8) * 0x01010101u;
        P.hi16_diff = ((m16 ^ x16) >> 8) & 0xffu;
        P.gap16x2 = g16 | (g16 << 16);
        if (b->prof16 && !b->prof16_int) {   // the profile form's tables hold s' = s - g (|s'| <= 254: exact)
            const uint32_t mp = f16_bits_scaled(in.match - in.gap), xp = f16_bits_scaled(in.mismatch - in.gap);
            P.lo16_base = (xp & 0xffu) * 0x01010101u;
            P.lo16_diff = (mp ^ xp) & 0xffu;
            P.hi16_base = (xp >> 8) * 0x01010101u;
            P.hi16_diff = ((mp ^ xp) >> 8) & 0xffu;
        } else if (b->prof16) {   // its integer row: the bytes s' = s - g (0..254) themselves, and gamma = -g in both halves
            const uint32_t mp = (uint32_t)(in.match - in.gap), xp = (uint32_t)(in.mismatch - in.gap), gamma = (uint32_t)(-in.gap);
            P.lo16_base = xp * 0x01010101u;
            P.lo16_diff = mp ^ xp;
            P.hi16_base = P.hi16_diff = 0;
            P.gap16x2 = gamma | (gamma << 16);
        }
    }
    P.slot_toff = b->slot_toff.as<uint32_t>();
    P.slot_tlen = b->slot_tlen.as<uint32_t>();
    return PWA_OK;
}

// ---- the pairs that do not run on strips: short patterns over a coded arena on the mini-stripe engine (no band, four pairs per
// wave, one launch per row class), everything else on the stripe engine (no band: exact first-maximum end cells, any scoring)
int setup_off_strips(pwa_ctx* ctx, pwa_batch* b, const BatchInput& in, const CellForm& f, const std::vector<uint64_t>& aoff,
                     const std::vector<uint32_t>& pairs) {
    const int match = in.match, mismatch = in.mismatch, gap = in.gap;
    const bool local = in.local, mini_gap0 = f.mini_gap0;
    std::vector<uint32_t> plist;
    std::vector<std::pair<int, std::vector<uint32_t>>> mini_lists;   // (rows per lane, pairs)
    for (const uint32_t k : pairs) {
        const int mrl = f.mini_scores ? mini_rl_for(in.len(in.pair_a[k])) : 0;
        if (!mrl) {
            plist.push_back(k);
            continue;
        }
        size_t c = 0;
        while (c < mini_lists.size() && mini_lists[c].first != mrl) ++c;
        if (c == mini_lists.size()) mini_lists.emplace_back(mrl, std::vector<uint32_t>());
        mini_lists[c].second.push_back(k);
    }
    const size_t nl = pairs.size();
    HIPC(ctx, b->pair_res.alloc(ctx, nl * sizeof(PairResult)));
    HIPC(ctx, hipMemset(b->pair_res.p, 0, nl * sizeof(PairResult)));
    size_t q_next = 0;
    auto describe = [&](uint32_t k, size_t q) {
        PairDesc d;
        std::memset(&d, 0, sizeof d);
        d.pat = b->arena.as<uint8_t>() + aoff[in.pair_a[k]];
        d.txt = b->arena.as<uint8_t>() + aoff[in.pair_b[k]];
        d.n = (int32_t)in.len(in.pair_a[k]);
        d.m = (int32_t)in.len(in.pair_b[k]);
        d.res = b->pair_res.as<PairResult>() + q;
        d.out_index = k;
        return d;
    };
    std::string names;
    if (!plist.empty()) {
        b->use_pairs = true;
        b->live_idx = plist;
        std::vector<PairDesc> pd;
        pd.reserve(plist.size());
        uint64_t pe_max_n = 0;
        for (const uint32_t k : plist) pe_max_n = std::max(pe_max_n, in.len(in.pair_a[k]));
        PairGeom geom = choose_geom(ctx->knobs, pe_max_n);
        {   // RL = 2 buys a pair more waves in flight -- which a list that fills the chip anyway does not need: [gpu, r03] SW scores of
            // 10k x 10k pairs, RL = 2 / RL = 4: 8 pairs 1.73 / 1.79 ms, 64 pairs 5.35 / 4.93 ms, 256 pairs 17.3 / 12.8 ms
            uint64_t stripes2 = 0;
            for (const uint32_t k : plist) stripes2 += (in.len(in.pair_a[k]) + 127) / 128;
            if (geom.rl == 2 && geom.w == 4 && !ctx->knobs.force_rl && stripes2 >= 2048) geom.rl = 4;
        }
        // a coded arena with keys in range (what the band-less mini kernels ask for as well): the keyed chunk without a band -- table
        // scoring, one v_max3 per cell, global fills gap-shifted -- instead of the plain compare-and-select step: [gpu, r03] SW scores of
        // 64 pairs 10k x 10k 4.8 -> 3.45 ms, NW 4.06 -> 2.05 ms; one pair 1.67 -> 1.26 / 1.55 -> 1.01 ms
        const bool keyed_scores = !in.nwdist() && f.mini_scores && !ctx->knobs.no_keyed_tb && !ctx->knobs.no_pair_table;
        const bool gap0_scores = keyed_scores && mini_gap0 && !ctx->knobs.no_gap_shift;   // (never semi-global: mini_gap0 is false)
        for (const uint32_t k : plist) {
            PairDesc d = describe(k, q_next++);
            d.score_bias = gap0_scores ? wrap_mul((int64_t)(in.len(in.pair_a[k]) + in.len(in.pair_b[k])), gap) : 0;
            pd.push_back(d);
            b->padded_cells += (in.len(in.pair_a[k]) + 64 * geom.rl - 1) / (64 * geom.rl) * (64 * geom.rl) * in.len(in.pair_b[k]);
        }
        PairForm form{PF_STRIPE_FILL, b->mode, BAND_NONE, WALK_NONE, gap0_scores ? CELLS_GAP0 : keyed_scores ? CELLS_CODED : CELLS_PLAIN, geom.rl, geom.w};
        if (in.nwdist() || in.affine()) form.family = in.nwdist() ? PF_STRIPE_DIST : PF_STRIPE_AFFINE, form.mode = PWA_MODE_NW;   // (affine: go travels as the gap, ge beside it)
        const int rc = b->pl.build(ctx, pd, form, gap0_scores ? match - 2 * gap : match, gap0_scores ? mismatch - 2 * gap : mismatch, gap0_scores ? 0 : gap,
                                   in.affine() ? in.gap_extend : 0);
        if (rc != PWA_OK) return rc;
        b->pl.G.scores_out = b->scores.as<int32_t>();   // the device score vector is complete after run()
        names = in.nwdist()   ? std::string("pair_dist_kernel<RL=") + std::to_string(geom.rl) + ",NW,DIST,no-band>"
                : in.affine() ? std::string("pair_affine_kernel<RL=") + std::to_string(geom.rl) + ",AFF,no-band>"
                              : std::string("pair_fill_kernel<RL=") + std::to_string(geom.rl) + (local ? ",SW" : in.semi ? ",SG" : (gap0_scores ? ",NW,GAP0" : ",NW")) + (keyed_scores ? ",keyed,no-band>" : ",no-traceback>");
    }
    for (auto& cls : mini_lists) {
        const int rl = cls.first;
        std::vector<uint32_t>& lst = cls.second;
        sort_by_length_desc(lst, [&](uint32_t x) { return in.len(in.pair_b[x]); });   // a wave's four texts about equally long
        std::vector<PairDesc> pd;
        pd.reserve(lst.size() + 3);
        for (const uint32_t k : lst) {
            PairDesc d = describe(k, q_next++);
            b->live_idx.push_back(k);
            d.score_bias = mini_gap0 ? wrap_mul((int64_t)(in.len(in.pair_a[k]) + in.len(in.pair_b[k])), gap) : 0;
            pd.push_back(d);
            b->padded_cells += (uint64_t)(16 * rl) * in.len(in.pair_b[k]);
        }
        const uint32_t n_real = (uint32_t)pd.size();
        while (pd.size() % 4) {   // empty patterns fill the last wave (their results go nowhere: no row of theirs is row n)
            PairDesc d = pd[n_real - 1];
            d.n = 0;
            pd.push_back(d);
        }
        b->mini.emplace_back(new PairLaunch());
        PairLaunch& ml = *b->mini.back();
        ml.mem = PairLaunch::MEM_FREE_LIST;
        const PairForm form{PF_MINI_FILL, b->mode, BAND_NONE, WALK_NONE, mini_gap0 ? CELLS_GAP0 : CELLS_CODED, rl, 16};
        const int rc = ml.build_mini(ctx, pd, n_real, form, mini_gap0 ? match - 2 * gap : match, mini_gap0 ? mismatch - 2 * gap : mismatch, mini_gap0 ? 0 : gap);
        if (rc != PWA_OK) return rc;
        ml.G.scores_out = b->scores.as<int32_t>();
        names += std::string(names.empty() ? "" : " + ") + "mini_fill_kernel<RL=" + std::to_string(rl) + (local ? ",SW" : in.semi ? ",SG" : (mini_gap0 ? ",NW,GAP0" : ",NW")) + ",no-band>";
    }
    b->kernel_name = b->use_strips ? b->kernel_name + " + " + names : names;   // (the strip kernel first: bench.py prices its instruction mix)
    return PWA_OK;
}

// ---- gotoh pairs off the strips (every SG list, every list with end cells, SW with mismatch > 0, no pad byte): the band-less form of
// the gotoh mini-stripe fill (gotoh_fill.hip.h, gotoh_scores_kernel), one launch per row class -- 16 lanes per pair up to 256 rows,
// one pair per wave up to 1024.  The fill itself writes PairResult and the device score vector: no walk follows.
int setup_gotoh_mini(pwa_ctx* ctx, pwa_batch* b, const BatchInput& in, const std::vector<uint64_t>& aoff, const std::vector<uint32_t>& pairs) {
    struct Cls {
        int rl, ln;
        std::vector<uint32_t> lst;
    };
    std::vector<Cls> classes;
    for (const uint32_t k : pairs) {
        const uint64_t n = in.len(in.pair_a[k]);
        const int ln = n <= 256 ? 16 : 64, rl = n <= 256 ? mini_rl_for(n) : n <= 512 ? 8 : 16;
        size_t c = 0;
        while (c < classes.size() && (classes[c].rl != rl || classes[c].ln != ln)) ++c;
        if (c == classes.size()) classes.push_back({rl, ln, {}});
        classes[c].lst.push_back(k);
    }
    HIPC(ctx, b->pair_res.alloc(ctx, pairs.size() * sizeof(PairResult)));
    HIPC(ctx, hipMemset(b->pair_res.p, 0, pairs.size() * sizeof(PairResult)));
    static const char* const kModeName[3] = {"NW", "SW", "SG"};
    size_t q_next = 0;
    std::string names;
    for (Cls& cls : classes) {
        sort_by_length_desc(cls.lst, [&](uint32_t x) { return in.len(in.pair_b[x]); });   // a wave's four texts about equally long
        const size_t ppw = (size_t)(64 / cls.ln);
        std::vector<PairDesc> pd;
        pd.reserve(cls.lst.size() + 3);
        for (const uint32_t k : cls.lst) {
            PairDesc d;
            std::memset(&d, 0, sizeof d);
            d.pat = b->arena.as<uint8_t>() + aoff[in.pair_a[k]];
            d.txt = b->arena.as<uint8_t>() + aoff[in.pair_b[k]];
            d.n = (int32_t)in.len(in.pair_a[k]);
            d.m = (int32_t)in.len(in.pair_b[k]);
            d.res = b->pair_res.as<PairResult>() + q_next++;
            d.out_index = k;
            b->live_idx.push_back(k);
            pd.push_back(d);
            b->padded_cells += (uint64_t)(cls.ln * cls.rl) * in.len(in.pair_b[k]);
        }
        const uint32_t n_real = (uint32_t)pd.size();
        while (pd.size() % ppw) {   // empty patterns fill the last wave (no row of theirs is row n, no cell of theirs a maximum: nothing is written)
            PairDesc d = pd[n_real - 1];
            d.n = 0;
            pd.push_back(d);
        }
        b->mini.emplace_back(new PairLaunch());
        PairLaunch& ml = *b->mini.back();
        ml.mem = PairLaunch::MEM_FREE_LIST;
        PairForm form{in.subst ? PF_MINI_SUBST : PF_MINI_GOTOH, b->mode, BAND_NONE, WALK_NONE, CELLS_KEYED, cls.rl, cls.ln};
        if (in.subst) form.subst = SubstRef{b->subst.dev.as<uint32_t>(), b->subst.n_sym, b->subst.stride};
        const int rc = ml.build_mini(ctx, pd, n_real, form, in.match, in.mismatch, in.gap);
        if (rc != PWA_OK) return rc;
        ml.G.gap_extend = in.gap_extend;
        ml.G.scores_out = b->scores.as<int32_t>();
        names += std::string(names.empty() ? "" : " + ") + (in.subst ? "subst_scores_kernel<RL=" : "gotoh_scores_kernel<RL=") + std::to_string(cls.rl) + ",LN=" + std::to_string(cls.ln) + "," +
                 kModeName[b->mode] + ",no-band>";
    }
    b->kernel_name = names;
    return PWA_OK;
}

int batch_create_impl(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, int kind, int gap_extend,
                      const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a,
                      const uint32_t* pair_b, uint64_t n_pairs, int want_end_cells, pwa_batch** out, SubstTable* subst = nullptr) try {
    if (!ctx || !out) return PWA_E_INVALID;
    *out = nullptr;
    const bool affine = kind == KIND_AFFINE, nwdist = kind == KIND_NWDIST, gotoh = kind == KIND_GOTOH || kind == KIND_SUBST;
    if ((kind == KIND_SUBST) != (subst != nullptr)) return fail(ctx, PWA_E_INVALID, "internal: substitution table");
    if ((affine || nwdist) && want_end_cells) return fail(ctx, PWA_E_INVALID, "end cells are not defined for this pass");
    if (mode != PWA_MODE_NW && mode != PWA_MODE_SW && (mode != PWA_MODE_SG || affine || nwdist)) return fail(ctx, PWA_E_INVALID, "unknown mode");
    if (gotoh && (gap > 0 || gap_extend > 0)) return fail(ctx, PWA_E_INVALID, "gotoh gap penalties must be <= 0 (gap_open + L * gap_extend)");
    if (!seq_off || (n_pairs && (!pair_a || !pair_b))) return fail(ctx, PWA_E_INVALID, "null input");
    if (n_seq && !seq_bytes && seq_off[n_seq] != 0) return fail(ctx, PWA_E_INVALID, "null seq_bytes");
    if (n_pairs >= 0xffffffffull) return fail(ctx, PWA_E_CAPACITY, "more than 2^32-2 pairs in one batch");
    for (uint32_t s = 0; s < n_seq; ++s)
        if (seq_off[s + 1] < seq_off[s]) return fail(ctx, PWA_E_INVALID, "seq_off not monotone");
    HIPC(ctx, hipSetDevice(ctx->device));
    CreateClock clock{ctx};
    BatchInput in{seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, kind, match, mismatch, gap, gap_extend,
                  mode == PWA_MODE_SW, want_end_cells != 0, mode == PWA_MODE_SG, nullptr};

    pwa_batch* b = new (std::nothrow) pwa_batch();
    if (!b) return fail(ctx, PWA_E_NOMEM, "host allocation");
    struct Guard {
        pwa_batch* b;
        ~Guard() { if (b) pwa_batch_destroy(b); }
    } guard{b};
    b->ctx = ctx;
    for (DevBuf* d : {&b->arena, &b->tasks, &b->slot_poff, &b->slot_plen, &b->slot_out, &b->slot_toff, &b->slot_tlen, &b->lane_text, &b->hand, &b->queue,
                      &b->scores, &b->pair_res})
        d->pool = ctx;   // released buffers are kept for the next batch of this context
    b->pl.mem = PairLaunch::MEM_FREE_LIST;   // (and those of its launches)
    b->mode = mode;
    b->n_pairs = n_pairs;
    b->want_end = in.want_end;
    b->affine = affine;
    b->nwdist = nwdist;
    b->gotoh = gotoh;
    if (subst) {   // the batch keeps the table: the caller's arrays are free after this call
        b->subst.blob.swap(subst->blob);
        b->subst.n_sym = subst->n_sym;
        b->subst.stride = subst->stride;
        b->subst.max_abs = subst->max_abs;
        in.subst = &b->subst;
    }

    LivePairs lp;
    int rc = scan_pairs(ctx, b, in, lp);
    if (rc != PWA_OK) return rc;
    b->n_live = lp.live.size();
    HIPC(ctx, b->scores.alloc(ctx, std::max<uint64_t>(n_pairs, 1) * sizeof(int32_t)));
    if (lp.any_trivial_score) HIPC(ctx, upload_via_bounce(ctx, b->scores.p, b->host_scores.data(), n_pairs * sizeof(int32_t)));
    else {   // (on the copy stream and waited for: a run may be enqueued on any stream afterwards -- and the context's own stream may be
             // busy with the previous batch's run, which preparing this one must not wait for)
        HIPC(ctx, hipMemsetAsync(b->scores.p, 0, std::max<uint64_t>(n_pairs, 1) * sizeof(int32_t), ctx->copy_stream));
        HIPC(ctx, hipStreamSynchronize(ctx->copy_stream));
    }
    HIPC(ctx, b->queue.alloc(ctx, 64));   // (the event ring of the runs is created run by run: pwa_batch_run)
    if (lp.live.empty()) {
        b->kernel_name = "none";
        guard.b = nullptr;
        *out = b;
        return PWA_OK;
    }

    // ---- which sequences play which role; the alphabet, the cell form, the arena
    std::vector<uint8_t> is_text(n_seq, 0), is_used(n_seq, 0);
    for (uint32_t k : lp.live) {
        is_text[pair_b[k]] = 1;
        is_used[pair_a[k]] = is_used[pair_b[k]] = 1;
    }
    if (subst && (rc = subst_upload(ctx, b->subst)) != PWA_OK) return rc;
    const Alphabet al = scan_alphabet(in, is_text);
    CellForm form;
    if ((rc = choose_cell_form(ctx, in, lp, al, form)) != PWA_OK) return rc;
    b->use_strips = form.strips;
    b->aff_go = form.aff_go;
    b->aff_ge = form.aff_ge;
    b->aff_neg = form.aff_neg;
    std::vector<uint64_t> aoff;
    if ((rc = upload_arena(ctx, b, in, is_used, lp.max_n, form, al, aoff)) != PWA_OK) return rc;
    clock.mark("validate + arena upload");

    b->padded_cells = 0;
    std::vector<uint32_t> off_strips;   // the pairs that run off the strips (all of them when the strips cannot serve the list)
    if (!b->use_strips) off_strips = lp.live;
    if (b->use_strips) {
        StripTasks st = plan_strip_tasks(ctx, in, lp.live, form, al);
        b->lanes = st.lanes;
        clock.mark("sort + group pairs");
        StripHeight h = choose_strip_height(st.ht, form, st.lanes, false, ctx->knobs);
        if (h.R == 0) return fail(ctx, PWA_E_INVALID, "internal: no kernel instantiation");
        if (cell16_admitted(ctx->knobs, in, form, al, st.lanes, lp.max_n)) {
            std::vector<HostTask> ht16 = group_by_text(in, st.order, 128);
            const StripHeight h16 = choose_strip_height(ht16, form, st.lanes, true, ctx->knobs);
            if (h16.R != 0 && (ctx->knobs.cell16 == 1 || h16.cost < h.cost)) {
                b->cell16 = true;
                st.ht.swap(ht16);
                h = h16;
            }
        }
        if (route_eligible(in, form, lp.max_n, lp.max_m) && ctx->knobs.scores_route != 0) {
            const std::vector<uint32_t> move = tasks_to_move(ctx, in, st, h.R, b->cell16 ? 128 : 64, route_cost(in, form, b->cell16, h.mode), form.mini_scores);
            if (!move.empty()) {
                off_strips = split_tasks(st, move);
                if (!st.ht.empty()) h = choose_strip_height(st.ht, form, st.lanes, b->cell16, ctx->knobs);   // the strips that stay may prefer another height
            }
        }
        if (b->cell16 && !st.ht.empty() && prof16_admitted(ctx->knobs, al, lp.max_n)) {   // the strips that stay, one pattern per task
            std::vector<uint32_t> porder;
            for (const auto& t : st.ht)
                for (uint32_t l = 0; l < t.count; ++l) porder.push_back(st.order[t.first + l]);
            std::vector<HostTask> htp = group_by_pattern(in, porder);
            if (ctx->knobs.prof16 == 1 || prof16_cost(htp) < h.cost) {
                b->prof16 = true;
                b->prof16_int = prof16_int_admitted(ctx->knobs, in);
                st.order.swap(porder);
                st.ht.swap(htp);
            }
        }
        if (st.ht.empty()) b->use_strips = false;
        if (b->use_strips && (rc = setup_strips(ctx, b, in, form, al, aoff, st, h, lp.max_m, clock)) != PWA_OK) return rc;
    }
    if (!off_strips.empty() && (rc = gotoh ? setup_gotoh_mini(ctx, b, in, aoff, off_strips) : setup_off_strips(ctx, b, in, form, aoff, off_strips)) != PWA_OK) return rc;
    if (ctx->knobs.debug) {
        clock.mark("engine setup");
        HIPC(ctx, hipDeviceSynchronize());
        clock.mark("hipDeviceSynchronize");
        hipLaunchKernelGGL(pwa_nop_kernel, dim3(1), dim3(64), 0, ctx->stream, (int*)nullptr);
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
        clock.mark("nop kernel + sync");
        hipLaunchKernelGGL(pwa_nop_kernel, dim3(1), dim3(64), 0, ctx->stream, (int*)nullptr);
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
        clock.mark("nop kernel + sync again");
    }
    guard.b = nullptr;
    *out = b;
    return PWA_OK;
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
} catch (...) {
    return fail(ctx, PWA_E_HIP, "unexpected C++ exception");   // nothing may propagate across the C ABI
}

// The strip engine addresses its sequence arena with 32-bit offsets (4 GiB per batch object).  The one-shot entry points
// take pair lists of any size: the list is cut into runs of consecutive pairs whose sequences fit one arena, each run is
// one batch object, results land in the caller's vectors at the run's offset (pairs are independent, hw2.cpp:328-338).
uint64_t arena_limit(const pwa_ctx* ctx) {
    if (ctx->knobs.arena_limit) return ctx->knobs.arena_limit;   // tests
    return 0xffffffffull - (1ull << 20);
}
// r03 (overlap H2D with compute): the runs are PIPELINED -- while the kernels of run k execute, run k + 1 is validated,
// scheduled, coded and uploaded (copy stream, page-locked pieces) and its kernels are queued behind; the host then collects run k.
// Destroyed runs hand their device buffers to the context's free list (no hipFree: it would wait for the run in flight).
// Cutting a list that FITS one arena into several runs, so that the first kernels start before all of the input is on the device, was
// built and measured (PWA_PIPE_RUNS=6) and is not the default: [gpu] hw2_amd -l on 262 144 pairs 150 x 2000 (569 MB): scores pass 89 ms in
// one run, 137 ms in six -- the kernels of that input take 9 ms, the rest is host work per run (alphabet scans, sorts, uploads with their
// synchronisations), which six runs pay six times; 4.5 GB (two arenas): 357 ms in two pipelined runs, 493 ms in six
// (profiles/r03_cli_scale.txt).
template <class Create>
int scores_in_arena_chunks(pwa_ctx* ctx, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                           uint64_t n_pairs, int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out, Create&& create) try {
    if (!seq_off || (n_pairs && (!pair_a || !pair_b))) return fail(ctx, PWA_E_INVALID, "null input");
    uint64_t limit = arena_limit(ctx);
    std::vector<uint64_t> stamp(n_seq, 0);
    uint64_t chunk = 0;
    if (!ctx->knobs.arena_limit && ctx->knobs.pipe_runs > 1) {   // experiment: cut a list that fits one arena into PWA_PIPE_RUNS runs
        ++chunk;
        uint64_t total = 512;
        for (uint64_t k = 0; k < n_pairs; ++k)
            for (const uint32_t sidx : {pair_a[k], pair_b[k]}) {
                if (sidx >= n_seq) return fail(ctx, PWA_E_INVALID, "pair index out of range");
                if (stamp[sidx] != chunk) total += align_up(seq_off[sidx + 1] - seq_off[sidx] + 1, 16);
                stamp[sidx] = chunk;
            }
        limit = std::min<uint64_t>(limit, std::max<uint64_t>(1ull << 20, total / (uint64_t)ctx->knobs.pipe_runs + (1ull << 20)));
    }
    struct InFlight {
        pwa_batch* b = nullptr;
        uint64_t k0 = 0;
    } prev;
    auto collect = [&](InFlight& f) -> int {   // wait for the run's own event, copy its results out, recycle its buffers
        if (!f.b) return PWA_OK;
        const int rc = pwa_batch_fetch(f.b, score_out + f.k0, end_i_out ? end_i_out + f.k0 : nullptr, end_j_out ? end_j_out + f.k0 : nullptr);
        pwa_batch_destroy(f.b);
        f.b = nullptr;
        return rc;
    };
    uint64_t k0 = 0, n_runs = 0;
    int rc = PWA_OK;
    const auto t_begin = std::chrono::steady_clock::now();
    while (k0 < n_pairs && rc == PWA_OK) {
        ++chunk;
        ++n_runs;
        uint64_t k1 = k0, bytes = 512;
        for (; k1 < n_pairs; ++k1) {
            uint64_t add = 0;
            for (const uint32_t sidx : {pair_a[k1], pair_b[k1]}) {
                if (sidx >= n_seq) {
                    (void)collect(prev);
                    return fail(ctx, PWA_E_INVALID, "pair index out of range");
                }
                if (stamp[sidx] != chunk) add += align_up(seq_off[sidx + 1] - seq_off[sidx] + 1, 16);
            }
            if (pair_a[k1] == pair_b[k1] && stamp[pair_a[k1]] != chunk) add /= 2;
            if (bytes + add > limit && k1 > k0) break;
            bytes += add;
            stamp[pair_a[k1]] = stamp[pair_b[k1]] = chunk;
        }
        pwa_batch* b = nullptr;
        rc = create(pair_a + k0, pair_b + k0, k1 - k0, &b);   // host work + uploads: overlaps the kernels of the previous run
        // the arena estimate above is not the only 32-bit limit inside a batch object (per-lane text rows of the LANES form, slot
        // arrays): a run that is refused for its size is halved until it fits -- pairs are independent (hw2.cpp:328-338)
        while (rc == PWA_E_CAPACITY && k1 - k0 > 1) {
            k1 = k0 + (k1 - k0) / 2;
            rc = create(pair_a + k0, pair_b + k0, k1 - k0, &b);
        }
        if (rc == PWA_OK) rc = pwa_batch_run(b, nullptr);      // queued behind the previous run on the context's stream
        const int rc_prev = collect(prev);                      // ... whose results are copied out meanwhile
        if (rc == PWA_OK) {
            prev.b = b;
            prev.k0 = k0;
            rc = rc_prev;
            if (ctx->knobs.no_pipeline && rc == PWA_OK) rc = collect(prev);   // A/B: every run is collected before the next one is prepared
        } else if (b) {
            pwa_batch_destroy(b);
        }
        k0 = k1;
    }
    const int rc_last = collect(prev);
    if (ctx->knobs.debug)
        std::fprintf(stderr, "[pwa] scores pass: %llu pairs in %llu pipelined run(s) of <= %llu MB of sequences, %.3f ms in all\n", (unsigned long long)n_pairs,
                     (unsigned long long)n_runs, (unsigned long long)(limit >> 20), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    return rc != PWA_OK ? rc : rc_last;
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
}

}  // namespace

extern "C" {

int pwa_batch_create(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, const uint8_t* seq_bytes,
                     const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                     uint64_t n_pairs, int want_end_cells, pwa_batch** out) {
    return batch_create_impl(ctx, mode, match, mismatch, gap, KIND_LINEAR, 0, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                             want_end_cells, out);
}

int pwa_affine_batch_create(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                            const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                            uint64_t n_pairs, pwa_batch** out) {
    return batch_create_impl(ctx, PWA_MODE_NW, match, mismatch, gap_open, KIND_AFFINE, gap_extend, seq_bytes, seq_off, n_seq, pair_a,
                             pair_b, n_pairs, 0, out);
}

int pwa_nwdist_batch_create(pwa_ctx* ctx, int match, int mismatch, int gap, const uint8_t* seq_bytes, const uint64_t* seq_off,
                            uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, pwa_batch** out) {
    return batch_create_impl(ctx, PWA_MODE_NW, match, mismatch, gap, KIND_NWDIST, 0, seq_bytes, seq_off, n_seq, pair_a, pair_b,
                             n_pairs, 0, out);
}

int pwa_gotoh_batch_create(pwa_ctx* ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                           const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                           int want_end_cells, pwa_batch** out) {
    return batch_create_impl(ctx, mode, match, mismatch, gap_open, KIND_GOTOH, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                             want_end_cells, out);
}

int pwa_subst_batch_create(pwa_ctx* ctx, int mode, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend,
                           const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                           uint64_t n_pairs, int want_end_cells, pwa_batch** out) try {
    if (!ctx || !out) return PWA_E_INVALID;
    *out = nullptr;
    SubstTable tab;
    const int rc = subst_prepare(ctx, code, n_sym, submat, tab);
    if (rc != PWA_OK) return rc;
    return batch_create_impl(ctx, mode, 0, 0, gap_open, KIND_SUBST, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, want_end_cells, out,
                             &tab);
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
}

int pwa_batch_run(pwa_batch* b, void* stream_v) {
    if (!b) return PWA_E_INVALID;
    pwa_ctx* ctx = b->ctx;
    HIPC(ctx, hipSetDevice(ctx->device));   // the caller's thread may have another device current
    hipStream_t st = stream_v ? static_cast<hipStream_t>(stream_v) : ctx->stream;
    const int slot = (int)(b->n_runs % pwa_batch::kRing);
    if (!b->ev0[slot] || !b->ev1[slot]) {   // both or neither: a half-created pair is torn down and created again
        if (b->ev0[slot]) (void)hipEventDestroy(b->ev0[slot]);
        if (b->ev1[slot]) (void)hipEventDestroy(b->ev1[slot]);
        b->ev0[slot] = b->ev1[slot] = nullptr;
        HIPC(ctx, hipEventCreate(&b->ev0[slot]));
        HIPC(ctx, hipEventCreate(&b->ev1[slot]));
    }
    HIPC(ctx, hipEventRecord(b->ev0[slot], st));
    if (b->n_live) {
        if (b->use_strips) {
            HIPC(ctx, hipMemsetAsync(b->queue.p, 0, 16, st));
            if (b->nwdist) {
                NwDistParams dp;
                dp.b = b->bp;
                dp.tab2_lo = 0x000000ffu;   // selector 0 (symbols equal) -> -1, every other selector -> 0
                dp.tab2_hi = 0u;
                dp.scores2 = nullptr;
                hipLaunchKernelGGL(reinterpret_cast<nwdist_kernel_t>(b->strip_fn), dim3(b->grid), dim3(64), 0, st, dp);
            } else if (b->affine || b->gotoh) {   // (the gotoh strips take go and ge the same way; neg is hw3's alone)
                AffineParams ap;
                ap.b = b->bp;
                ap.go = b->aff_go;
                ap.ge = b->aff_ge;
                ap.neg = b->aff_neg;
                hipLaunchKernelGGL(reinterpret_cast<affine_kernel_t>(b->strip_fn), dim3(b->grid), dim3(64), 0, st, ap);
            } else {
                // b->grid waves as workgroups of four, with an LDS request that admits exactly their share per CU: a balanced
                // placement whatever ran before (batch_scores.hip.h)
                const uint32_t n_wg = (b->grid + 3) / 4, per_cu = (n_wg + (uint32_t)ctx->num_cu - 1) / (uint32_t)ctx->num_cu;
                static const uint32_t kPadKiB[6] = {0, 96, 64, 48, 36, 30};
                const size_t pad_lds = per_cu <= 5 ? (size_t)kPadKiB[per_cu] * 1024 : 0;
                HIPC(ctx, hipFuncSetAttribute(b->strip_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad_lds));
                hipLaunchKernelGGL(reinterpret_cast<batch_kernel_t>(b->strip_fn), dim3(n_wg), dim3(256), pad_lds, st, b->bp);
            }
            HIPC(ctx, hipGetLastError());
        }
        // the stripe launch of a split batch is often a few long pairs -- tens of waves bound by their own pipeline latency -- so the
        // mini-stripe launches run NEXT to it, on the context's auxiliary stream, forked after the strips and joined before the end
        const bool fork = b->use_pairs && !b->mini.empty();
        hipStream_t ms = fork ? ctx->aux_stream : st;
        if (fork) {
            HIPC(ctx, hipEventRecord(ctx->aux_ev[0], st));
            HIPC(ctx, hipStreamWaitEvent(ms, ctx->aux_ev[0], 0));
        }
        if (b->use_pairs) {
            const int rc = b->pl.launch(ctx, st, nullptr);
            if (rc != PWA_OK) return rc;
        }
        for (auto& ml : b->mini) {
            const int rc = ml->launch(ctx, ms, nullptr);
            if (rc != PWA_OK) return rc;
        }
        if (fork) {
            HIPC(ctx, hipEventRecord(ctx->aux_ev[1], ms));
            HIPC(ctx, hipStreamWaitEvent(st, ctx->aux_ev[1], 0));
        }
    }
    HIPC(ctx, hipEventRecord(b->ev1[slot], st));
    ++b->n_runs;
    b->ran = true;
    return PWA_OK;
}

int32_t* pwa_batch_d_scores(pwa_batch* b) {
    if (!b) return nullptr;
    return b->ext_scores ? b->ext_scores : b->scores.as<int32_t>();
}

int pwa_batch_set_d_scores(pwa_batch* b, int32_t* d_scores) {
    if (!b || !d_scores) return PWA_E_INVALID;
    pwa_ctx* ctx = b->ctx;
    HIPC(ctx, hipSetDevice(ctx->device));
    // carry over what is already there (pairs with an empty side are resolved at create time)
    HIPC(ctx, hipMemcpy(d_scores, pwa_batch_d_scores(b), b->n_pairs * sizeof(int32_t), hipMemcpyDeviceToDevice));
    b->ext_scores = d_scores;
    b->bp.scores = d_scores;
    b->pl.G.scores_out = d_scores;
    for (auto& ml : b->mini) ml->G.scores_out = d_scores;
    return PWA_OK;
}

int pwa_batch_last_ms(pwa_batch* b, float* ms) {
    if (!b || !ms || !b->ran) return PWA_E_INVALID;
    HIPC(b->ctx, hipSetDevice(b->ctx->device));
    const int slot = (int)((b->n_runs - 1) % pwa_batch::kRing);
    HIPC(b->ctx, hipEventSynchronize(b->ev1[slot]));
    HIPC(b->ctx, hipEventElapsedTime(ms, b->ev0[slot], b->ev1[slot]));
    return PWA_OK;
}

int pwa_batch_run_times(pwa_batch* b, float* ms_out, int cap, int* n_out) {
    if (!b || !ms_out || !n_out || cap < 0) return PWA_E_INVALID;
    HIPC(b->ctx, hipSetDevice(b->ctx->device));
    const uint64_t have = std::min<uint64_t>(b->n_runs, pwa_batch::kRing);
    const int n = (int)std::min<uint64_t>(have, (uint64_t)cap);
    for (int k = 0; k < n; ++k) {   // oldest of the last n first
        const int slot = (int)((b->n_runs - n + k) % pwa_batch::kRing);
        HIPC(b->ctx, hipEventSynchronize(b->ev1[slot]));
        HIPC(b->ctx, hipEventElapsedTime(&ms_out[k], b->ev0[slot], b->ev1[slot]));
    }
    *n_out = n;
    return PWA_OK;
}

int pwa_batch_info(const pwa_batch* b, uint64_t* cells, uint64_t* padded_cells, uint64_t* n_tasks,
                   const char** kernel_name) {
    if (!b) return PWA_E_INVALID;
    if (cells) *cells = b->cells;
    if (padded_cells) *padded_cells = b->padded_cells;
    if (n_tasks) {
        *n_tasks = (b->use_strips ? b->bp.n_tasks : 0) + (b->use_pairs ? (uint64_t)b->pl.G.n_pairs : 0);
        for (const auto& ml : b->mini) *n_tasks += ml->G.n_tasks;
    }
    if (kernel_name) *kernel_name = b->kernel_name.c_str();
    return PWA_OK;
}

int pwa_batch_profile_form(const pwa_batch* b) {
    if (!b) return PWA_E_INVALID;
    return b->use_strips && b->prof16 ? 1 : 0;
}

int pwa_batch_profile_int(const pwa_batch* b) {
    if (!b) return PWA_E_INVALID;
    return b->use_strips && b->prof16 && b->prof16_int ? 1 : 0;
}

int pwa_profile_plan(uint32_t min_text_len, uint32_t max_text_len, uint32_t* interior_blocks, uint32_t* blocks) {
    if (!interior_blocks || !blocks || min_text_len > max_text_len || max_text_len > 0x7fffffffu) return PWA_E_INVALID;
    *blocks = (max_text_len + 7) / 8;
    *interior_blocks = std::min<uint32_t>((uint32_t)prof16_interior_blocks((int)min_text_len), *blocks);
    return PWA_OK;
}

int pwa_strip_table(uint32_t index, const char** name, int* rows, int* mode, int* score_path, uint32_t* variants, uint32_t* count) {
    size_t n = 0;
    const BatchKernelEntry* const t = batch_kernel_table(&n);
    if (count) *count = (uint32_t)n;
    if (index >= n) return PWA_E_INVALID;
    const BatchKernelEntry& e = t[index];
    if (name) *name = e.name;
    if (rows) *rows = e.R;
    if (mode) *mode = e.mode;
    if (score_path) *score_path = e.score;
    if (variants)
        *variants = (e.fn_single ? PWA_STRIP_SINGLE : 0u) | (e.fn_lanes ? PWA_STRIP_LANES : 0u) | (e.fn_lanes_single ? PWA_STRIP_LANES_SINGLE : 0u) |
                    (e.fn_cell16 ? PWA_STRIP_CELL16 : 0u) | (e.fn_cell16_single ? PWA_STRIP_CELL16_SINGLE : 0u) | (e.fn_prof16 ? PWA_STRIP_PROF16 : 0u) |
                    (e.fn_prof16_int ? PWA_STRIP_PROF16_INT : 0u);
    return PWA_OK;
}

int pwa_batch_cell_bits(const pwa_batch* b) {
    if (!b) return PWA_E_INVALID;
    return b->use_strips ? (b->cell16 ? 16 : 32) : 0;
}

int pwa_batch_fetch(pwa_batch* b, int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out) try {
    if (!b || !score_out) return PWA_E_INVALID;
    pwa_ctx* ctx = b->ctx;
    if ((end_i_out || end_j_out) && !b->want_end) return fail(ctx, PWA_E_INVALID, "batch was created without end cells");
    if (!b->ran) return fail(ctx, PWA_E_INVALID, "pwa_batch_run has not been called");
    HIPC(ctx, hipSetDevice(ctx->device));
    HIPC(ctx, hipEventSynchronize(b->ev1[(b->n_runs - 1) % pwa_batch::kRing]));
    if (b->use_pairs) {   // the bounded spins of the stripe pipeline: a workgroup that gave up says so here
        const int rc = b->pl.check(ctx);
        if (rc != PWA_OK) return rc;
    }
    if (!b->want_end || b->n_live == 0) {   // both engines write their pairs' scores into the device score vector
        HIPC(ctx, hipMemcpy(score_out, pwa_batch_d_scores(b), b->n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (b->want_end) {   // only reachable with no live pairs
            if (end_i_out) std::memcpy(end_i_out, b->host_end_i.data(), b->n_pairs * 4);
            if (end_j_out) std::memcpy(end_j_out, b->host_end_j.data(), b->n_pairs * 4);
        }
        return PWA_OK;
    }
    std::vector<PairResult> res(b->n_live);   // end cells asked for: every live pair ran off the strips (stripe or mini-stripe engine)
    HIPC(ctx, hipMemcpy(res.data(), b->pair_res.p, b->n_live * sizeof(PairResult), hipMemcpyDeviceToHost));
    std::memcpy(score_out, b->host_scores.data(), b->n_pairs * sizeof(int32_t));
    if (b->want_end) {
        if (end_i_out) std::memcpy(end_i_out, b->host_end_i.data(), b->n_pairs * 4);
        if (end_j_out) std::memcpy(end_j_out, b->host_end_j.data(), b->n_pairs * 4);
    }
    for (uint64_t q = 0; q < b->n_live; ++q) {
        const uint32_t k = b->live_idx[q];
        score_out[k] = res[q].score;
        if (end_i_out) end_i_out[k] = res[q].end_i;
        if (end_j_out) end_j_out[k] = res[q].end_j;
    }
    return PWA_OK;
} catch (const std::bad_alloc&) {
    return fail(b ? b->ctx : nullptr, PWA_E_NOMEM, "host allocation failed");
} catch (...) {
    return fail(b ? b->ctx : nullptr, PWA_E_HIP, "unexpected C++ exception");   // nothing may propagate across the C ABI
}

void pwa_batch_destroy(pwa_batch* b) {
    if (!b) return;
    if (b->ctx) (void)hipSetDevice(b->ctx->device);
    // the device buffers go back to the context's free list, not to hipFree (which would wait for the whole device): wait here for
    // this batch's own last run, so that the next batch cannot be handed memory a kernel is still using
    if (b->ran && b->n_runs) {
        const int slot = (int)((b->n_runs - 1) % pwa_batch::kRing);
        if (b->ev1[slot]) (void)hipEventSynchronize(b->ev1[slot]);
    }
    for (int e = 0; e < pwa_batch::kRing; ++e) {
        if (b->ev0[e]) (void)hipEventDestroy(b->ev0[e]);
        if (b->ev1[e]) (void)hipEventDestroy(b->ev1[e]);
    }
    b->hand.park_hand();   // the hand-off workspace stays the context's parked one if it is the larger one (DevMem::park_hand)
    delete b;
}

int pwa_scores(pwa_ctx* ctx, int mode, int match, int mismatch, int gap, const uint8_t* seq_bytes,
               const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
               uint64_t n_pairs, int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out) {
    if (!ctx || !score_out) return PWA_E_INVALID;
    return scores_in_arena_chunks(ctx, seq_off, n_seq, pair_a, pair_b, n_pairs, score_out, end_i_out, end_j_out,
                                  [&](const uint32_t* a, const uint32_t* b, uint64_t n, pwa_batch** out) {
                                      return pwa_batch_create(ctx, mode, match, mismatch, gap, seq_bytes, seq_off, n_seq, a, b, n,
                                                              (end_i_out || end_j_out) ? 1 : 0, out);
                                  });
}

int pwa_distances(pwa_ctx* ctx, int match, int mismatch, int gap, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                  const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* dist_out) {
    if (!ctx || !dist_out) return PWA_E_INVALID;
    return scores_in_arena_chunks(ctx, seq_off, n_seq, pair_a, pair_b, n_pairs, dist_out, nullptr, nullptr,
                                  [&](const uint32_t* a, const uint32_t* b, uint64_t n, pwa_batch** out) {
                                      return pwa_nwdist_batch_create(ctx, match, mismatch, gap, seq_bytes, seq_off, n_seq, a, b, n, out);
                                  });
}

int pwa_scores_affine(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                      const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                      int32_t* score_out) {
    if (!ctx || !score_out) return PWA_E_INVALID;
    return scores_in_arena_chunks(ctx, seq_off, n_seq, pair_a, pair_b, n_pairs, score_out, nullptr, nullptr,
                                  [&](const uint32_t* a, const uint32_t* b, uint64_t n, pwa_batch** out) {
                                      return pwa_affine_batch_create(ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq,
                                                                     a, b, n, out);
                                  });
}

int pwa_scores_gotoh(pwa_ctx* ctx, int mode, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                     const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                     int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out) {
    if (!ctx || !score_out) return PWA_E_INVALID;
    return scores_in_arena_chunks(ctx, seq_off, n_seq, pair_a, pair_b, n_pairs, score_out, end_i_out, end_j_out,
                                  [&](const uint32_t* a, const uint32_t* b, uint64_t n, pwa_batch** out) {
                                      return pwa_gotoh_batch_create(ctx, mode, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq,
                                                                    a, b, n, (end_i_out || end_j_out) ? 1 : 0, out);
                                  });
}

int pwa_scores_subst(pwa_ctx* ctx, int mode, const uint8_t* code, int n_sym, const int32_t* submat, int gap_open, int gap_extend,
                     const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                     uint64_t n_pairs, int32_t* score_out, uint32_t* end_i_out, uint32_t* end_j_out) {
    if (!ctx || !score_out) return PWA_E_INVALID;
    {   // (an empty list creates no batch: the table and the gaps are checked all the same)
        SubstTable tab;
        const int rc = subst_prepare(ctx, code, n_sym, submat, tab);
        if (rc != PWA_OK) return rc;
        if (gap_open > 0 || gap_extend > 0) return fail(ctx, PWA_E_INVALID, "gotoh gap penalties must be <= 0 (gap_open + L * gap_extend)");
    }
    return scores_in_arena_chunks(ctx, seq_off, n_seq, pair_a, pair_b, n_pairs, score_out, end_i_out, end_j_out,
                                  [&](const uint32_t* a, const uint32_t* b, uint64_t n, pwa_batch** out) {
                                      return pwa_subst_batch_create(ctx, mode, code, n_sym, submat, gap_open, gap_extend, seq_bytes, seq_off, n_seq,
                                                                    a, b, n, (end_i_out || end_j_out) ? 1 : 0, out);
                                  });
}

}  // extern "C"
