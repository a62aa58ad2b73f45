// pwalign_affine_tb.hip -- hw3's affine-gap alignments of a pair list (pwa_align_affine_batch): 32-row strip wave tasks
// (batch_affine_tb.hip.h) and, for few long pairs, the stripe engine (pair_affine_tb.hip.h).
#include "pwalign_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

#include "batch_affine_tb.hip.h"

using namespace pwa;

namespace {

constexpr int kAffStripRows = 32, kAffStripBlocks = kAffStripRows / 4;   // rows of a strip (batch_affine_tb_kernel), its 4-row blocks

// What pwa_align_affine_batch was called with: scoring, sequences, pair list and the caller's result buffers
struct AffTbRequest {
    int match, mismatch, gap_open, gap_extend;
    const uint8_t* seq_bytes;
    const uint64_t* seq_off;
    uint32_t n_seq;
    const uint32_t *pair_a, *pair_b;
    uint64_t n_pairs;
    int32_t* score_out;
    uint8_t* ops;
    const uint64_t* ops_off;
    uint64_t* n_ops;
    uint64_t slen(uint32_t s) const { return seq_off[s + 1] - seq_off[s]; }
};

// A wave task of the affine alignment strips (batch_affine_tb_kernel): `count` pairs order[first ..] sharing string1 (m columns),
// their string2 over `strips` 32-row strips, the task's code band tb_dwords
struct AffTbTask {
    uint32_t first, count;
    uint64_t strips, m, tb_dwords;
};

// The pairs that reach a kernel (both sides non-empty), ascending, and the longest string1 / string2 among them
struct AffLive {
    std::vector<uint32_t> live;
    uint64_t max_m = 0, max_n2 = 0;
};

// The raw-byte device arena: sequence s at aoff[s]; pad_byte occurs in no string1
struct AffArena {
    DevBuf arena;
    std::vector<uint64_t> aoff;
    int pad_byte = -1;
};

// Device results of the whole call (scores and strip op counts by pair index, op lists at dev_ops_off[k]), the strips' queue word and
// hand-off halves, and the host's op counts
struct AffResults {
    DevBuf d_scores, d_ops, d_nops, d_queue, d_hand;
    std::vector<uint64_t> dev_ops_off;
    uint64_t ops_total = 0;
    uint64_t half = 0;        // int32 per hand-off half
    uint32_t grid_cap = 0;    // most workgroups of a strip launch
    std::vector<uint32_t> h_nops;
};

int validate_affine(pwa_ctx* ctx, const AffTbRequest& rq) {
    if (!rq.seq_off || !rq.score_out || !rq.ops || !rq.ops_off || !rq.n_ops || (rq.n_pairs && (!rq.pair_a || !rq.pair_b)))
        return fail(ctx, PWA_E_INVALID, "null input");
    if (rq.n_seq && !rq.seq_bytes && rq.seq_off[rq.n_seq] != 0) return fail(ctx, PWA_E_INVALID, "null seq_bytes");
    return check_pair_list(ctx, rq.pair_a, rq.pair_b, rq.n_pairs, rq.n_seq);
}

// ---- pairs with an empty side: the reference's boundary walk (hw3.cpp:42-53, 105-131) -- all 'D' or all 'I' -- written to the
// caller's buffers here; the others are listed in lp
int resolve_empty_pairs(pwa_ctx* ctx, const AffTbRequest& rq, AffLive& lp) {
    for (uint64_t k = 0; k < rq.n_pairs; ++k) {
        const uint64_t n1 = rq.slen(rq.pair_a[k]), n2 = rq.slen(rq.pair_b[k]);
        if (n1 > 0x3fffffffull || n2 > 0x3fffffffull) return fail(ctx, PWA_E_CAPACITY, "sequence longer than 2^30");
        if (n1 == 0 || n2 == 0) {
            rq.score_out[k] = (n1 + n2 == 0) ? 0 : (int32_t)((uint32_t)rq.gap_open + (uint32_t)wrap_mul((int64_t)(n1 + n2 - 1), rq.gap_extend));
            std::memset(rq.ops + rq.ops_off[k], n1 ? 'D' : 'I', n1 + n2);
            rq.n_ops[k] = n1 + n2;
            continue;
        }
        lp.live.push_back((uint32_t)k);
        lp.max_m = std::max(lp.max_m, n1);
        lp.max_n2 = std::max(lp.max_n2, n2);
    }
    return PWA_OK;
}

// ---- arena: raw bytes; pad byte = one that no string1 (text) contains
int build_raw_arena(pwa_ctx* ctx, const AffTbRequest& rq, const std::vector<uint32_t>& live, AffArena& ar) {
    std::vector<uint8_t> is_used(rq.n_seq, 0);
    bool in_text[256] = {false};
    for (uint32_t k : live) {
        is_used[rq.pair_a[k]] = is_used[rq.pair_b[k]] = 1;
    }
    {
        std::vector<uint8_t> is_text(rq.n_seq, 0);
        for (uint32_t k : live) is_text[rq.pair_a[k]] = 1;
        for (uint32_t s = 0; s < rq.n_seq; ++s)
            if (is_text[s])
                for (uint64_t o = rq.seq_off[s]; o < rq.seq_off[s + 1]; ++o) in_text[rq.seq_bytes[o]] = true;
    }
    for (int v = 255; v >= 0 && ar.pad_byte < 0; --v)
        if (!in_text[v]) ar.pad_byte = v;
    if (ar.pad_byte < 0) return fail(ctx, PWA_E_CAPACITY, "the first sequences of the pairs use all 256 byte values: no padding symbol left");
    const uint64_t arena_bytes = layout_arena(rq.seq_off, rq.n_seq, is_used, 512, ar.aoff);
    if (arena_bytes >= 0xffffffffull) return fail(ctx, PWA_E_CAPACITY, "sequence arena exceeds 4 GiB");
    std::vector<uint8_t> host_arena(arena_bytes, 0);
    for (uint32_t s = 0; s < rq.n_seq; ++s)
        if (is_used[s] && rq.slen(s)) std::memcpy(host_arena.data() + ar.aoff[s], rq.seq_bytes + rq.seq_off[s], rq.slen(s));
    HIPC(ctx, ar.arena.alloc(ctx, arena_bytes));
    HIPC(ctx, upload_via_bounce(ctx, ar.arena.p, host_arena.data(), arena_bytes));
    return PWA_OK;
}

// ---- wave tasks: pairs grouped by string1, string2 sorted by length (descending), 64 per wave
std::vector<AffTbTask> group_wave_tasks(const AffTbRequest& rq, const std::vector<uint32_t>& live, std::vector<uint32_t>& order) {
    order = live;
    {
        std::vector<uint64_t> key(order.size());
        for (size_t o = 0; o < order.size(); ++o)
            key[o] = ((uint64_t)rq.pair_a[order[o]] << 32) | (uint64_t)(0x7fffffffu - (uint32_t)rq.slen(rq.pair_b[order[o]]));
        radix_sort_by_key(key, order);
    }
    std::vector<AffTbTask> ht;
    for (size_t p = 0; p < order.size();) {
        size_t q = p;
        while (q < order.size() && q - p < 64 && rq.pair_a[order[q]] == rq.pair_a[order[p]]) ++q;
        const uint64_t strips = (rq.slen(rq.pair_b[order[p]]) + kAffStripRows - 1) / kAffStripRows, m = rq.slen(rq.pair_a[order[p]]);
        ht.push_back({(uint32_t)p, (uint32_t)(q - p), strips, m, strips * m * kAffStripBlocks * 64});
        p = q;
    }
    return ht;
}

// ---- pwa_align_affine_batch: which strip wave tasks move to the stripe engine (pair_affine_tb.hip.h).  A strip wave task is one
// wave running strips x m columns of 32 rows on its own: [gpu] the 15 center pairs of 16 x 10 kb are ONE task, 313 strips x 10 000
// columns in 5.47 s, 55 ns per row and column.  The stripe engine spreads each pair over ceil(n / 256) waves that sweep anti-diagonals,
// then walks every pair with one wave.  As in tasks_to_move, tasks are moved in order of decreasing strip cost and the count with
// the smallest estimated total -- the strip launch and the stripe launches run one after the other -- wins; a task whose strip band
// does not fit the budget moves whatever the estimate (the strips cannot run it at all).  Constants: profiles/hw3_align_route_probe.txt.
std::vector<uint8_t> affine_tb_route(const pwa_ctx* ctx, const AffTbRequest& rq, const std::vector<AffTbTask>& ht,
                                     const std::vector<uint32_t>& order, uint64_t strip_budget_bytes, bool eligible) {
    const size_t nt = ht.size();
    std::vector<uint8_t> move(nt, 0);
    const int route = ctx->knobs.affine_tb_route;
    if (!eligible || route == 0) return move;
    if (route == 1) {
        std::fill(move.begin(), move.end(), 1);
        return move;
    }
    // [gpu] profiles/hw3_align_route_probe.txt: strips 55 ns per row and column of a task (one wave alone); stripe engine, a pair
    // alone: 32.5 us per 256-row stripe + 134 ns per step; chip full (16 x 100 kb): 340 ns per stripe step and SIMD; walks ~50 ns per op
    constexpr double kStripNs = 55.0;
    constexpr double kStepNs = 340.0, kLagUs = 32.5, kLoneStepNs = 134.0, kWalkNsPerOp = 50.0, kLaunchUs = 30.0;
    const double kSimds = 4.0 * ctx->num_cu;
    std::vector<double> I(nt), S(nt), L(nt);   // strip ns / stripe fill ns x SIMD / longest stripe fill + walk (ns) of a task
    std::vector<uint32_t> ord(nt);
    for (size_t t = 0; t < nt; ++t) {
        ord[t] = (uint32_t)t;
        I[t] = (double)ht[t].strips * 32.0 * (double)ht[t].m * kStripNs;
        double steps = 0, lat = 0;
        for (uint32_t l = 0; l < ht[t].count; ++l) {
            const uint32_t k = order[ht[t].first + l];
            const double n = (double)rq.slen(rq.pair_a[k]), m = (double)rq.slen(rq.pair_b[k]), stripes = std::ceil(n / 256.0);
            steps += stripes * (m + 63) * kStepNs;
            lat = std::max(lat, stripes * kLagUs * 1e3 + (m + 63) * kLoneStepNs + (n + m) * kWalkNsPerOp);
        }
        S[t] = steps;
        L[t] = lat;
    }
    // tasks that cannot stay first, then by decreasing strip cost
    auto must = [&](size_t t) { return ht[t].tb_dwords * 4 > strip_budget_bytes; };
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return must(x) != must(y) ? must(x) : I[x] > I[y]; });
    size_t n_must = 0;
    while (n_must < nt && must(ord[n_must])) ++n_must;
    std::vector<double> sufmax(nt + 1, 0.0), sufsum(nt + 1, 0.0);
    for (size_t k = nt; k-- > 0;) {
        sufmax[k] = std::max(sufmax[k + 1], I[ord[k]]);
        sufsum[k] = sufsum[k + 1] + I[ord[k]];
    }
    double best = -1, mS = 0, mL = 0;
    size_t best_k = n_must;
    for (size_t k = 0; k <= nt; ++k) {
        const double ts = std::max(sufmax[k], sufsum[k] / kSimds);                                    // ns
        const double tp = k ? std::max(mL, mS / kSimds) + kLaunchUs * 1e3 : 0.0;
        if (k >= n_must && (best < 0 || ts + tp < best)) {
            best = ts + tp;
            best_k = k;
        }
        if (k < nt) {
            mS += S[ord[k]];
            mL = std::max(mL, L[ord[k]]);
        }
    }
    for (size_t k = 0; k < best_k; ++k) move[ord[k]] = 1;
    if (ctx->knobs.debug)
        std::fprintf(stderr, "[pwa] align_affine route: %zu of %zu wave tasks to the stripe engine (%zu whose strip band exceeds %.2f GB; estimates: "
                             "all on strips %.1f ms, split %.1f ms)\n", best_k, nt, n_must, (double)strip_budget_bytes / 1e9,
                     std::max(sufmax[0], sufsum[0] / kSimds) * 1e-6, best * 1e-6);
    return move;
}

// ---- wave tasks that leave the strips for the stripe engine (pair_affine_tb.hip.h): by estimated cost, and every task whose
// strip band exceeds the budget.  Only lists whose keys stay inside int32 (the kernel's guard, 2^26 on the values) qualify.
// Returns their pairs, ascending; ht keeps the tasks that stay.
std::vector<uint32_t> split_off_stripe_pairs(const pwa_ctx* ctx, const AffTbRequest& rq, const AffLive& lp, const std::vector<uint32_t>& order,
                                             uint64_t strip_budget_bytes, std::vector<AffTbTask>& ht) {
    std::vector<uint32_t> stripe_pairs;
    const bool eligible = (int64_t)(lp.max_m + lp.max_n2 + 2) *
                              max_abs({rq.match, rq.mismatch, std::llabs((long long)rq.gap_open) + std::llabs((long long)rq.gap_extend), 1}) < (1ll << 26);
    const std::vector<uint8_t> move = affine_tb_route(ctx, rq, ht, order, strip_budget_bytes, eligible);
    std::vector<AffTbTask> keep;
    for (size_t t = 0; t < ht.size(); ++t) {
        if (!move[t]) {
            keep.push_back(ht[t]);
            continue;
        }
        for (uint32_t l = 0; l < ht[t].count; ++l) stripe_pairs.push_back(order[ht[t].first + l]);
    }
    ht.swap(keep);
    std::sort(stripe_pairs.begin(), stripe_pairs.end());
    return stripe_pairs;
}

// ---- the call's result buffers, the strips' queue word and (for n_strip_tasks > 0) their hand-off halves
int take_result_buffers(pwa_ctx* ctx, const AffTbRequest& rq, const AffLive& lp, size_t n_strip_tasks, AffResults& rs) {
    HIPC(ctx, rs.d_scores.alloc(ctx, rq.n_pairs * sizeof(int32_t)));
    HIPC(ctx, rs.d_nops.alloc(ctx, rq.n_pairs * sizeof(uint32_t)));
    HIPC(ctx, rs.d_queue.alloc(ctx, 64));
    rs.dev_ops_off.assign(rq.n_pairs, 0);
    for (uint32_t k : lp.live) {
        rs.dev_ops_off[k] = rs.ops_total;
        rs.ops_total += align_up(rq.slen(rq.pair_a[k]) + rq.slen(rq.pair_b[k]) + 1, 16);
    }
    HIPC(ctx, rs.d_ops.alloc(ctx, rs.ops_total));
    rs.half = ((lp.max_m + 3) / 4 + 1) * 192 * 4;   // int32 per half: three int4 per lane per 4-column block
    rs.grid_cap = (uint32_t)std::min<uint64_t>(n_strip_tasks, (uint64_t)ctx->num_cu * 2);
    if (rs.grid_cap) HIPC(ctx, rs.d_hand.alloc(ctx, (size_t)rs.grid_cap * 2 * rs.half * sizeof(int32_t)));
    rs.h_nops.assign(rq.n_pairs, 0);
    return PWA_OK;
}

// ---- pwa_align_affine_batch on the stripe engine: the pairs `pairs` (caller indices, ascending) in consecutive chunks whose bands fit
// the budget (min(0.6 free, 48 GiB), or PWA_RANGE_BYTES), one fill + walk launch per chunk.  Scores go to rs.d_scores[k], op lists to
// rs.d_ops + dev_ops_off[k]; rs.h_nops[k] is filled on the host.  Band, results and launch buffers come from the context's caches.
int affine_tb_on_stripes(pwa_ctx* ctx, const AffTbRequest& rq, const std::vector<uint32_t>& pairs, const AffArena& ar, AffResults& rs,
                         size_t free_b) {
    if (pairs.empty()) return PWA_OK;
    const uint64_t cap = ctx->knobs.range_bytes ? ctx->knobs.range_bytes : std::min<uint64_t>((uint64_t)(free_b * 0.6), 48ull << 30);
    constexpr uint64_t kWalkPad = 32768;   // the walk stages whole 16 KiB windows: one may run past the last band
    auto band = [&](uint32_t k) { return align_up(tb_band_bytes(rq.slen(rq.pair_a[k]), rq.slen(rq.pair_b[k]), 4), 256); };
    std::vector<std::pair<size_t, size_t>> chunks;
    uint64_t band_cap = 0, nc_cap = 0;
    for (size_t p0 = 0; p0 < pairs.size();) {
        size_t p1 = p0;
        uint64_t b = 0;
        while (p1 < pairs.size() && (p1 == p0 || b + band(pairs[p1]) <= cap)) b += band(pairs[p1++]);
        if (b + kWalkPad > (uint64_t)(free_b * 0.97)) return fail(ctx, PWA_E_NOMEM, "traceback band of a single pair exceeds free HBM");
        chunks.emplace_back(p0, p1);
        band_cap = std::max(band_cap, b);
        nc_cap = std::max<uint64_t>(nc_cap, p1 - p0);
        p0 = p1;
    }
    if (ctx->knobs.debug)
        std::fprintf(stderr, "[pwa] align_affine stripes: %zu pairs in %zu chunk(s) of <= %.2f GB of band (cap %.2f GB)\n", pairs.size(), chunks.size(),
                     (double)band_cap / 1e9, (double)cap / 1e9);
    Lease l_band, l_res;
    HIPC(ctx, workspace(ctx, DevMem::BAND, band_cap + kWalkPad, l_band));
    HIPC(ctx, workspace(ctx, DevMem::RES, nc_cap * sizeof(PairResult), l_res));
    PairResult* const d_res = l_res.as<PairResult>();
    for (const auto& ch : chunks) {
        const size_t nc = ch.second - ch.first;
        std::vector<PairDesc> pd(nc);
        uint64_t bo = 0, max_n = 0;
        for (size_t q = 0; q < nc; ++q) {
            const uint32_t k = pairs[ch.first + q];
            PairDesc& d = pd[q];
            std::memset(&d, 0, sizeof d);
            d.pat = ar.arena.as<uint8_t>() + ar.aoff[rq.pair_a[k]];   // rows: string1 (hw3's i), columns: string2 (j)
            d.txt = ar.arena.as<uint8_t>() + ar.aoff[rq.pair_b[k]];
            d.n = (int32_t)rq.slen(rq.pair_a[k]);
            d.m = (int32_t)rq.slen(rq.pair_b[k]);
            d.tb = l_band.as<uint8_t>() + bo;
            d.res = d_res + q;
            d.ops = rs.d_ops.as<uint8_t>() + rs.dev_ops_off[k];
            d.ops_cap = (uint32_t)(d.n + d.m);
            d.out_index = k;
            bo += band(k);
            max_n = std::max<uint64_t>(max_n, (uint64_t)d.n);
            ctx->aff_stats.band_bytes += tb_band_bytes((uint64_t)d.n, (uint64_t)d.m, 4);
        }
        HIPC(ctx, hipMemsetAsync(d_res, 0, nc * sizeof(PairResult), ctx->stream));
        PairLaunch pl;
        pl.mem = PairLaunch::MEM_SLOTS;
        const PairForm form{PF_STRIPE_AFFINE_TB, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_PLAIN, 4, max_n <= 256 ? 1 : 4};
        int rc = pl.build(ctx, pd, form, rq.match, rq.mismatch, rq.gap_open, rq.gap_extend);
        if (rc != PWA_OK) return rc;
        pl.G.scores_out = rs.d_scores.as<int32_t>();
        if (ctx->knobs.debug)
            std::fprintf(stderr, "[pwa] align_affine chunk: pairs %zu .. %zu, W=%d grid=%u tasks=%u band %.2f GB rows %llu B\n", ch.first, ch.second - 1,
                         pl.form.w, pl.grid, pl.G.n_tasks, (double)bo / 1e9, (unsigned long long)pl.row_bytes);
        HIPC(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
        rc = pl.launch(ctx, ctx->stream, ctx->ev[1]);
        if (rc != PWA_OK) return rc;
        HIPC(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
        rc = pl.check(ctx);
        if (rc != PWA_OK) return rc;
        float a = 0, c = 0;
        HIPC(ctx, hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
        HIPC(ctx, hipEventElapsedTime(&c, ctx->ev[1], ctx->ev[2]));
        ctx->aff_stats.fill_ms += a;
        ctx->aff_stats.walk_ms += c;
        std::vector<PairResult> res(nc);
        HIPC(ctx, hipMemcpy(res.data(), d_res, nc * sizeof(PairResult), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < nc; ++q) {
            if (res[q].overflow) return fail(ctx, PWA_E_CAPACITY, "internal: traceback longer than n+m");
            rs.h_nops[pairs[ch.first + q]] = res[q].n_ops;
        }
    }
    ctx->aff_stats.stripe_pairs += pairs.size();
    return PWA_OK;
}

// ---- one chunk of strip wave tasks ht[t0 .. t1) whose code bands (dw dwords in all) fit the budget: the tasks' tables, their
// uploads, the fill and the walk
int run_strip_chunk(pwa_ctx* ctx, const AffTbRequest& rq, const AffArena& ar, const AffResults& rs, const std::vector<uint32_t>& order,
                    const std::vector<AffTbTask>& ht, size_t t0, size_t t1, uint64_t dw) {
    const size_t nt = t1 - t0;
    std::vector<BatchTask> tasks(nt);
    std::vector<uint32_t> spoff(nt * 64, 0), splen(nt * 64, 0), sout(nt * 64, 0xffffffffu);
    std::vector<uint64_t> tboff(nt);
    std::vector<AffineWalkPair> wp;
    uint64_t at = 0;
    for (size_t t = 0; t < nt; ++t) {
        const AffTbTask& h = ht[t0 + t];
        const uint32_t text = rq.pair_a[order[h.first]];
        tasks[t].text_off = (uint32_t)ar.aoff[text];
        tasks[t].text_len = (uint32_t)h.m;
        tasks[t].slot0 = (uint32_t)(t * 64);
        tasks[t].n_strips = (uint32_t)h.strips;
        tboff[t] = at;
        for (uint32_t l = 0; l < h.count; ++l) {
            const uint32_t k = order[h.first + l];
            spoff[t * 64 + l] = (uint32_t)ar.aoff[rq.pair_b[k]];
            splen[t * 64 + l] = (uint32_t)rq.slen(rq.pair_b[k]);
            sout[t * 64 + l] = k;
            wp.push_back({at, rs.dev_ops_off[k], l, (uint32_t)h.m, (uint32_t)rq.slen(rq.pair_b[k]), k});
        }
        at += h.tb_dwords;
    }
    DevBuf d_tb, d_tasks, d_spoff, d_splen, d_sout, d_tboff, d_wp;
    HIPC(ctx, d_tb.alloc(ctx, dw * 4));
    HIPC(ctx, d_tasks.alloc(ctx, nt * sizeof(BatchTask)));
    HIPC(ctx, upload_via_bounce(ctx, d_tasks.p, tasks.data(), nt * sizeof(BatchTask)));
    HIPC(ctx, d_spoff.alloc(ctx, nt * 64 * 4));
    HIPC(ctx, upload_via_bounce(ctx, d_spoff.p, spoff.data(), nt * 64 * 4));
    HIPC(ctx, d_splen.alloc(ctx, nt * 64 * 4));
    HIPC(ctx, upload_via_bounce(ctx, d_splen.p, splen.data(), nt * 64 * 4));
    HIPC(ctx, d_sout.alloc(ctx, nt * 64 * 4));
    HIPC(ctx, upload_via_bounce(ctx, d_sout.p, sout.data(), nt * 64 * 4));
    HIPC(ctx, d_tboff.alloc(ctx, nt * sizeof(uint64_t)));
    HIPC(ctx, upload_via_bounce(ctx, d_tboff.p, tboff.data(), nt * sizeof(uint64_t)));
    HIPC(ctx, d_wp.alloc(ctx, wp.size() * sizeof(AffineWalkPair)));
    HIPC(ctx, upload_via_bounce(ctx, d_wp.p, wp.data(), wp.size() * sizeof(AffineWalkPair)));

    AffineTbParams T;
    std::memset(&T, 0, sizeof T);
    BatchParams& P = T.a.b;
    P.arena = ar.arena.as<uint8_t>();
    P.tasks = d_tasks.as<BatchTask>();
    P.slot_poff = d_spoff.as<uint32_t>();
    P.slot_plen = d_splen.as<uint32_t>();
    P.slot_out = d_sout.as<uint32_t>();
    P.scores = rs.d_scores.as<int32_t>();
    P.hand = rs.d_hand.as<int32_t>();
    P.hand_stride = 2 * rs.half;
    P.hand_half = (uint32_t)rs.half;
    P.queue = rs.d_queue.as<uint32_t>();
    P.n_tasks = (uint32_t)nt;
    P.match = rq.match;
    P.mismatch = rq.mismatch;
    P.gap = rq.gap_open;
    P.pad_word = (uint32_t)ar.pad_byte * 0x01010101u;
    T.a.go = rq.gap_open;
    T.a.ge = rq.gap_extend;
    T.a.neg = std::numeric_limits<int32_t>::min() / 2;   // hw3.cpp:16
    T.tb = d_tb.as<uint32_t>();
    T.task_tb_off = d_tboff.as<uint64_t>();
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nt, rs.grid_cap);
    HIPC(ctx, hipMemsetAsync(rs.d_queue.p, 0, 16, ctx->stream));
    hipLaunchKernelGGL((batch_affine_tb_kernel<kAffStripRows, SC_CMP>), dim3(grid), dim3(64), 0, ctx->stream, T);
    HIPC(ctx, hipGetLastError());
    hipLaunchKernelGGL((affine_walk_kernel<kAffStripRows>), dim3((uint32_t)((wp.size() + 63) / 64)), dim3(64), 0, ctx->stream,
                       d_wp.as<AffineWalkPair>(), (uint32_t)wp.size(), d_tb.as<uint32_t>(), rs.d_ops.as<uint8_t>(),
                       rs.d_nops.as<uint32_t>());
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return PWA_OK;
}

// ---- scores, op counts and op lists of the live pairs into the caller's buffers
int gather_results(pwa_ctx* ctx, const AffTbRequest& rq, const std::vector<uint32_t>& live, const std::vector<uint32_t>& stripe_pairs,
                   AffResults& rs) {
    std::vector<int32_t> h_scores(rq.n_pairs);
    std::vector<uint8_t> h_ops(rs.ops_total);
    HIPC(ctx, hipMemcpy(h_scores.data(), rs.d_scores.p, rq.n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
    {   // the strip walk's counts; the stripe pairs' came back with their results
        std::vector<uint32_t> strip_nops(rq.n_pairs);
        HIPC(ctx, hipMemcpy(strip_nops.data(), rs.d_nops.p, rq.n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::vector<uint8_t> on_stripes(rq.n_pairs, 0);
        for (uint32_t k : stripe_pairs) on_stripes[k] = 1;
        for (uint32_t k : live)
            if (!on_stripes[k]) rs.h_nops[k] = strip_nops[k];
    }
    HIPC(ctx, hipMemcpy(h_ops.data(), rs.d_ops.p, rs.ops_total, hipMemcpyDeviceToHost));
    for (uint32_t k : live) {
        rq.score_out[k] = h_scores[k];
        rq.n_ops[k] = rs.h_nops[k];
        if (rs.h_nops[k] > rq.slen(rq.pair_a[k]) + rq.slen(rq.pair_b[k])) return fail(ctx, PWA_E_CAPACITY, "internal: traceback longer than n+m");
        std::memcpy(rq.ops + rq.ops_off[k], h_ops.data() + rs.dev_ops_off[k], rs.h_nops[k]);
    }
    return PWA_OK;
}

}  // namespace

extern "C" {

// hw3.cpp:261-283: full affine-gap alignments (score + op list) of a pair list.  Pairs are grouped by string1 (for
// the center-star step every pair has the center there): it becomes the wave's shared text and every lane runs its
// own string2 down the rows (batch_affine_tb.hip.h).  Raw bytes, compare path, 32-row strips: the pass covers N-1
// pairs next to the all-pairs score pass over N(N-1)/2, so it is built for exactness, not for speed.  Wave tasks that would leave the chip
// idle -- few long pairs -- or whose band does not fit run on the stripe engine instead (pair_affine_tb.hip.h, affine_tb_route).
int pwa_align_affine_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                           const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b,
                           uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off, uint64_t* n_ops) try {
    if (!ctx) return PWA_E_INVALID;
    const AffTbRequest rq{match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, score_out, ops, ops_off, n_ops};
    int rc = validate_affine(ctx, rq);
    if (rc != PWA_OK) return rc;
    HIPC(ctx, hipSetDevice(ctx->device));
    ctx->aff_stats = AffineAlignStats{};
    AffLive lp;
    if ((rc = resolve_empty_pairs(ctx, rq, lp)) != PWA_OK) return rc;
    if (lp.live.empty()) return PWA_OK;
    AffArena ar;
    if ((rc = build_raw_arena(ctx, rq, lp.live, ar)) != PWA_OK) return rc;
    std::vector<uint32_t> order;
    std::vector<AffTbTask> ht = group_wave_tasks(rq, lp.live, order);

    size_t free_b = 0, total_b = 0;
    HIPC(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t tb_budget_dw = std::max<uint64_t>(std::min<uint64_t>((uint64_t)(free_b * 0.6), 6ull << 30) / 4, 1);
    const std::vector<uint32_t> stripe_pairs = split_off_stripe_pairs(ctx, rq, lp, order, tb_budget_dw * 4, ht);
    AffResults rs;
    if ((rc = take_result_buffers(ctx, rq, lp, ht.size(), rs)) != PWA_OK) return rc;
    if ((rc = affine_tb_on_stripes(ctx, rq, stripe_pairs, ar, rs, free_b)) != PWA_OK) return rc;

    // ---- chunks of tasks whose code bands fit the budget
    for (size_t t0 = 0; t0 < ht.size();) {
        size_t t1 = t0;
        uint64_t dw = 0;
        while (t1 < ht.size() && (t1 == t0 || dw + ht[t1].tb_dwords <= tb_budget_dw)) dw += ht[t1++].tb_dwords;
        if (dw * 4 > (uint64_t)(free_b * 0.9)) return fail(ctx, PWA_E_NOMEM, "traceback codes of one wave task exceed free HBM");
        if ((rc = run_strip_chunk(ctx, rq, ar, rs, order, ht, t0, t1, dw)) != PWA_OK) return rc;
        t0 = t1;
    }
    return gather_results(ctx, rq, lp.live, stripe_pairs, rs);
} catch (const std::bad_alloc&) {
    return fail(ctx, PWA_E_NOMEM, "host allocation failed");
} catch (...) {
    return fail(ctx, PWA_E_HIP, "unexpected C++ exception");   // nothing may propagate across the C ABI
}

int pwa_align_affine_last_stats(const pwa_ctx* ctx, uint64_t* stripe_pairs, float* fill_ms, float* walk_ms, uint64_t* band_bytes) {
    if (!ctx) return PWA_E_INVALID;
    if (stripe_pairs) *stripe_pairs = ctx->aff_stats.stripe_pairs;
    if (fill_ms) *fill_ms = ctx->aff_stats.fill_ms;
    if (walk_ms) *walk_ms = ctx->aff_stats.walk_ms;
    if (band_bytes) *band_bytes = ctx->aff_stats.band_bytes;
    return PWA_OK;
}

}  // extern "C"
