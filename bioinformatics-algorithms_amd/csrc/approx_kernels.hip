// approx_kernels.hip -- the approximate-search entries of include/pwalign.h (pwa_approx_*): validation, the task plan, the lane
// order, device buffers, the count and the fill pass; the starts pass over a hit list and the host-only minima of
// one (§3.19).  Kernels: approx.hip.h.
#include "../../include/pwalign.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "approx.hip.h"
#include "approx_ctx.h"
#include "sufarr_ctx.h"

using namespace pwa::approx;
using pwa::Dev;
using pwa::Fail;

namespace {

constexpr uint64_t kDefaultSliceHits = 1ull << 27;   // 8 B of staging per hit: 1 GB per slice at most
constexpr uint64_t kMaxSliceHits = 1ull << 31;       // offsets within a slice are uint32

using scan_kernel_t = decltype(&approx_scan_kernel<1, false>);
template <bool FILL>
scan_kernel_t scan_kernel_for(int W) {
    switch (W) {
        case 1: return approx_scan_kernel<1, FILL>;
        case 2: return approx_scan_kernel<2, FILL>;
        case 3: return approx_scan_kernel<3, FILL>;
        case 4: return approx_scan_kernel<4, FILL>;
        case 5: return approx_scan_kernel<5, FILL>;
        case 6: return approx_scan_kernel<6, FILL>;
        case 7: return approx_scan_kernel<7, FILL>;
        default: return approx_scan_kernel<8, FILL>;
    }
}

// Everything a call keeps on the device and the host between its passes
struct Search {
    uint32_t rows = 0;                            // sigma + 1: the codes of the call
    uint64_t n_tasks = 0, columns = 0;
    uint64_t peq_words = 0;                       // of one mask array of the call
    size_t tbytes = 0;                            // of the padded text buffer
    std::vector<Pat> pats;
    uint32_t first_wave[kMaxWords + 2] = {};      // class W's waves are lane_task[64 * first_wave[W] .. 64 * first_wave[W + 1])
    Dev text, blob, d_pats, peq, tasks, lane_task, task_cnt, pat_cnt, pat_best;
    std::vector<uint32_t> h_cnt;                  // hits per pattern
    std::vector<uint64_t> h_best;
};

void launch_scan(const pwa::ApproxCtxView& v, Search& s, bool fill, uint32_t t0, uint32_t t1, const uint32_t* d_off, uint64_t* d_out, uint32_t out_cap) {
    for (int W = 1; W <= kMaxWords; ++W) {
        const uint32_t waves = s.first_wave[W + 1] - s.first_wave[W];
        if (!waves) continue;
        scan_kernel_t kern = fill ? scan_kernel_for<true>(W) : scan_kernel_for<false>(W);
        const size_t lds = (size_t)s.rows * W * 64 * 8;
        if (lds > 64 * 1024) UNIT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(waves), dim3(64), lds, v.stream, s.text.as<uint8_t>(), s.peq.as<uint64_t>(), s.d_pats.as<Pat>(), s.tasks.as<Task>(),
                           s.lane_task.as<uint32_t>() + (size_t)64 * s.first_wave[W], s.rows, s.task_cnt.as<uint32_t>(), s.pat_cnt.as<uint32_t>(),
                           s.pat_best.as<unsigned long long>(), t0, t1, d_off, d_out, out_cap);
        UNIT_CHECK(hipGetLastError());
    }
}

// The limits of include/pwalign.h, without the device; on PWA_OK tab maps a byte to its code and sigma is the number of pattern bytes
int validate(const pwa::ApproxCtxView& v, const char* who, uint64_t n, const uint8_t* pb, const uint64_t* poff, uint32_t n_pat, CodeTable& tab, uint32_t& sigma) {
    if (n >= (1ull << 31)) {
        *v.err = std::string(who) + ": a text of " + std::to_string(n) + " bytes; positions are int32, so at most 2^31 - 1";
        return PWA_E_CAPACITY;
    }
    for (uint32_t q = 0; q < n_pat; ++q) {
        if (poff[q + 1] < poff[q]) return PWA_E_INVALID;
        const uint64_t m = poff[q + 1] - poff[q];
        if (m == 0) {
            *v.err = std::string(who) + ": pattern " + std::to_string(q) + " is empty";
            return PWA_E_INVALID;
        }
        if (m > 64 * kMaxWords) {
            *v.err = std::string(who) + ": pattern " + std::to_string(q) + " has " + std::to_string(m) + " symbols, at most " + std::to_string(64 * kMaxWords);
            return PWA_E_CAPACITY;
        }
    }
    bool seen[256] = {};
    if (n_pat)
        for (uint64_t i = poff[0]; i < poff[n_pat]; ++i) seen[pb[i]] = true;
    sigma = 0;
    for (int c = 0; c < 256; ++c) sigma += seen[c];
    if (sigma > kMaxSym) {
        *v.err = std::string(who) + ": the patterns hold " + std::to_string(sigma) + " distinct byte values, at most " + std::to_string(kMaxSym);
        return PWA_E_CAPACITY;
    }
    uint32_t next = 0;
    for (int c = 0; c < 256; ++c) tab.t[c] = seen[c] ? (uint8_t)next++ : (uint8_t)sigma;
    return PWA_OK;
}

// What every pass starts from: the patterns of the call (s.pats, with bound min(max_dist, m), or m without max_dist) and the places
// of their masks, and on the device the raw text (padded to 16 bytes + 16 with zeros), the pattern bytes and the pattern records,
// enqueued on the stream.  The caller codes the text and builds its masks inside its own events.
void stage_inputs(const pwa::ApproxCtxView& v, Search& s, const uint8_t* text, uint64_t n, const uint8_t* pb, const uint64_t* poff, uint32_t n_pat,
                  const uint32_t* max_dist, uint32_t sigma) {
    s.rows = sigma + 1;
    const uint64_t base = poff[0], bytes = poff[n_pat] - base;
    s.pats.resize(n_pat);
    s.peq_words = 0;
    for (uint32_t q = 0; q < n_pat; ++q) {
        const uint32_t m = (uint32_t)(poff[q + 1] - poff[q]), W = (m + 63) / 64;
        if (s.peq_words + (uint64_t)s.rows * W > 0xffffffffull || poff[q] - base > 0xffffffffull)
            throw Fail{PWA_E_CAPACITY, "pwa_approx: the patterns of one call exceed 32-bit offsets"};
        s.pats[q] = Pat{(uint32_t)(poff[q] - base), m, max_dist ? std::min(max_dist[q], m) : m, (uint32_t)s.peq_words, W};
        s.peq_words += (uint64_t)s.rows * W;
    }
    (void)hipSetDevice(v.device);
    s.tbytes = (n + 15) / 16 * 16 + 16;
    UNIT_CHECK(s.text.alloc(v.poison, s.tbytes));
    UNIT_CHECK(s.blob.alloc(v.poison, bytes));
    UNIT_CHECK(s.d_pats.alloc(v.poison, (size_t)n_pat * sizeof(Pat)));
    UNIT_CHECK(s.peq.alloc(v.poison, s.peq_words * 8));
    UNIT_CHECK(hipMemsetAsync(s.text.p, 0, s.tbytes, v.stream));
    UNIT_CHECK(hipMemcpyAsync(s.text.p, text, n, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(s.blob.p, pb + base, bytes, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(s.d_pats.p, s.pats.data(), (size_t)n_pat * sizeof(Pat), hipMemcpyHostToDevice, v.stream));
}

// Uploads, codes the text, builds the masks, runs the count pass; fills s.h_cnt / s.h_best and the stats of v
void count_pass(const pwa::ApproxCtxView& v, Search& s, const uint8_t* text, uint64_t n, const uint8_t* pb, const uint64_t* poff, uint32_t n_pat,
                const uint32_t* max_dist, const CodeTable& tab, uint32_t sigma) {
    s.rows = sigma + 1;
    s.h_cnt.assign(n_pat, 0);
    s.h_best.assign(n_pat, kNoBest);
    *v.stats = pwa::ApproxStats{};
    if (!n || !n_pat) return;
    // the plan, as any caller gets it
    std::vector<uint32_t> len(n_pat);
    for (uint32_t q = 0; q < n_pat; ++q) len[q] = (uint32_t)(poff[q + 1] - poff[q]);
    uint64_t nt = 0;
    (void)pwa_approx_plan(n, len.data(), max_dist, n_pat, v.chunk, nullptr, nullptr, nullptr, nullptr, 0, &nt);
    if (nt >= kNoTask) throw Fail{PWA_E_CAPACITY, "pwa_approx: " + std::to_string(nt) + " tasks; task numbers are uint32 (raise PWA_APPROX_CHUNK)"};
    std::vector<uint32_t> t_pat(nt);
    std::vector<uint64_t> t_scan(nt), t_lo(nt), t_hi(nt);
    if (pwa_approx_plan(n, len.data(), max_dist, n_pat, v.chunk, t_pat.data(), t_scan.data(), t_lo.data(), t_hi.data(), nt, &nt) != PWA_OK)
        throw Fail{PWA_E_INVALID, "pwa_approx: the task plan failed"};
    s.n_tasks = nt;
    std::vector<Task> tasks(nt);
    for (uint64_t t = 0; t < nt; ++t) {
        tasks[t] = Task{t_pat[t], (uint32_t)t_scan[t], (uint32_t)t_lo[t], (uint32_t)t_hi[t]};
        s.columns += t_hi[t] - t_scan[t];
    }
    // patterns and their masks' places, the uploads every pass shares, then the first tasks
    stage_inputs(v, s, text, n, pb, poff, n_pat, max_dist, sigma);
    std::vector<uint32_t> first_task(n_pat + 1, 0);
    const uint64_t per_pat = (n + v.chunk - 1) / v.chunk;
    for (uint32_t q = 0; q < n_pat; ++q) first_task[q + 1] = first_task[q] + (uint32_t)per_pat;
    // lane order: per word class, chunk by chunk, the patterns of the class side by side; a wave holds one class
    std::vector<uint32_t> lane_task;
    lane_task.reserve(nt + 64 * kMaxWords);
    for (int W = 1; W <= kMaxWords; ++W) {
        s.first_wave[W] = (uint32_t)(lane_task.size() / 64);
        std::vector<uint32_t> of_class;
        for (uint32_t q = 0; q < n_pat; ++q)
            if ((int)s.pats[q].W == W) of_class.push_back(q);
        for (uint64_t c = 0; c < per_pat && !of_class.empty(); ++c)
            for (uint32_t q : of_class) lane_task.push_back(first_task[q] + (uint32_t)c);
        lane_task.resize((lane_task.size() + 63) / 64 * 64, kNoTask);
    }
    s.first_wave[kMaxWords + 1] = (uint32_t)(lane_task.size() / 64);

    UNIT_CHECK(s.tasks.alloc(v.poison, nt * sizeof(Task)));
    UNIT_CHECK(s.lane_task.alloc(v.poison, lane_task.size() * 4));
    UNIT_CHECK(s.task_cnt.alloc(v.poison, nt * 4));
    UNIT_CHECK(s.pat_cnt.alloc(v.poison, (size_t)n_pat * 4));
    UNIT_CHECK(s.pat_best.alloc(v.poison, (size_t)n_pat * 8));
    pwa::Events<2> ev;
    UNIT_CHECK(ev.create());
    UNIT_CHECK(hipMemcpyAsync(s.tasks.p, tasks.data(), nt * sizeof(Task), hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(s.lane_task.p, lane_task.data(), lane_task.size() * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemsetAsync(s.pat_cnt.p, 0, (size_t)n_pat * 4, v.stream));
    UNIT_CHECK(hipMemsetAsync(s.pat_best.p, 0xff, (size_t)n_pat * 8, v.stream));
    UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
    UNIT_CHECK(pwa::recode_bytes(v.stream, s.text.as<uint8_t>(), s.tbytes / 16, tab.t));
    const uint64_t mask_threads = (uint64_t)n_pat * s.rows * kMaxWords;
    approx_masks_kernel<<<(uint32_t)((mask_threads + 255) / 256), 256, 0, v.stream>>>(s.blob.as<uint8_t>(), s.d_pats.as<Pat>(), n_pat, s.rows, tab, s.peq.as<uint64_t>());
    UNIT_CHECK(hipGetLastError());
    launch_scan(v, s, false, 0, 0, nullptr, nullptr, 0);
    UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
    UNIT_CHECK(hipMemcpyAsync(s.h_cnt.data(), s.pat_cnt.p, (size_t)n_pat * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipMemcpyAsync(s.h_best.data(), s.pat_best.p, (size_t)n_pat * 8, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    UNIT_CHECK(hipEventElapsedTime(&v.stats->count_ms, ev.e[0], ev.e[1]));
    v.stats->tasks = nt;
    v.stats->columns = s.columns;
    if (v.debug)
        std::fprintf(stderr, "[pwa] approx count: %u patterns, sigma=%u, %llu tasks, %llu columns, device %.3f ms\n", n_pat, sigma, (unsigned long long)nt,
                     (unsigned long long)s.columns, v.stats->count_ms);
}

// The fill pass: slices of whole tasks whose hits fit the staging budget (one task alone may exceed it: at most chunk hits)
void fill_pass(const pwa::ApproxCtxView& v, Search& s, uint64_t* occ) {
    if (!s.n_tasks) return;
    const uint64_t budget = std::min(v.occ_chunk_hits ? v.occ_chunk_hits : kDefaultSliceHits, kMaxSliceHits);
    std::vector<uint32_t> cnt(s.n_tasks);
    UNIT_CHECK(hipMemcpyAsync(cnt.data(), s.task_cnt.p, s.n_tasks * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    std::vector<pwa::Run> slices = pwa::cut_runs(s.n_tasks, budget, [&](uint64_t t) { return (uint64_t)cnt[t]; });
    slices.erase(std::remove_if(slices.begin(), slices.end(), [](const pwa::Run& sl) { return !sl.weight; }), slices.end());   // (nothing to fill)
    if (slices.empty()) return;
    uint64_t max_hits = 0;
    uint32_t max_nt = 0;
    for (const pwa::Run& sl : slices) {
        max_hits = std::max(max_hits, sl.weight);
        max_nt = std::max(max_nt, (uint32_t)(sl.k1 - sl.k0));
    }
    Dev off, part, stage;
    UNIT_CHECK(off.alloc(v.poison, (size_t)max_nt * 4));
    UNIT_CHECK(part.alloc(v.poison, pwa::scan_part_words(max_nt) * 4));
    UNIT_CHECK(stage.alloc(v.poison, max_hits * 8));
    pwa::Events<2> ev;
    UNIT_CHECK(ev.create());
    uint64_t kept = 0;
    for (const pwa::Run& sl : slices) {
        const uint32_t t0 = (uint32_t)sl.k0, t1 = (uint32_t)sl.k1, nt = t1 - t0;
        const uint64_t hits = sl.weight;
        UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
        UNIT_CHECK(hipMemcpyAsync(off.p, s.task_cnt.as<uint32_t>() + t0, (size_t)nt * 4, hipMemcpyDeviceToDevice, v.stream));
        pwa::scan_excl(v.stream, off.as<uint32_t>(), nt, part.as<uint32_t>());
        UNIT_CHECK(hipGetLastError());
        launch_scan(v, s, true, t0, t1, off.as<uint32_t>(), stage.as<uint64_t>(), (uint32_t)hits);
        UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
        UNIT_CHECK(hipMemcpyAsync(occ + kept, stage.p, hits * 8, hipMemcpyDeviceToHost, v.stream));
        UNIT_CHECK(hipStreamSynchronize(v.stream));
        float ms = 0.f;
        UNIT_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        v.stats->fill_ms += ms;
        kept += hits;
    }
    if (v.debug) std::fprintf(stderr, "[pwa] approx fill: %zu slices, %llu hits, device %.3f ms\n", slices.size(), (unsigned long long)kept, v.stats->fill_ms);
}

using start_kernel_t = decltype(&approx_start_kernel<1>);
start_kernel_t start_kernel_for(int W) {
    switch (W) {
        case 1: return approx_start_kernel<1>;
        case 2: return approx_start_kernel<2>;
        case 3: return approx_start_kernel<3>;
        case 4: return approx_start_kernel<4>;
        case 5: return approx_start_kernel<5>;
        case 6: return approx_start_kernel<6>;
        case 7: return approx_start_kernel<7>;
        default: return approx_start_kernel<8>;
    }
}

// The starts pass: the hits sorted into word classes (a counting sort, stable), then slices of at most PWA_OCC_CHUNK_HITS records, each
// slice one launch per word class it touches; the starts land in a device array parallel to occ and come back in one copy.
void starts_pass(const pwa::ApproxCtxView& v, Search& s, const uint8_t* text, uint64_t n, const uint8_t* pb, const uint64_t* poff, uint32_t n_pat,
                 const uint64_t* occ_off, const uint64_t* occ, const CodeTable& tab, uint32_t sigma, uint32_t* start_out) {
    const uint64_t total = occ_off[n_pat] - occ_off[0];
    stage_inputs(v, s, text, n, pb, poff, n_pat, nullptr, sigma);
    uint64_t class_at[kMaxWords + 2] = {};   // class W's records are sorted[class_at[W] .. class_at[W + 1])
    for (uint32_t q = 0; q < n_pat; ++q) class_at[s.pats[q].W + 1] += occ_off[q + 1] - occ_off[q];
    for (int W = 1; W <= kMaxWords; ++W) class_at[W + 1] += class_at[W];
    std::vector<Hit> sorted(total);
    {
        uint64_t at[kMaxWords + 1];
        for (int W = 1; W <= kMaxWords; ++W) at[W] = class_at[W];
        for (uint32_t q = 0; q < n_pat; ++q)
            for (uint64_t x = occ_off[q]; x < occ_off[q + 1]; ++x)
                sorted[at[s.pats[q].W]++] = Hit{q, (uint32_t)(occ[x] >> 32), (uint32_t)occ[x], (uint32_t)(x - occ_off[0])};
    }
    const uint64_t budget = std::min(v.occ_chunk_hits ? v.occ_chunk_hits : kDefaultSliceHits, kMaxSliceHits);
    const uint64_t slice_cap = std::min(budget, total);
    Dev recs, starts;
    UNIT_CHECK(recs.alloc(v.poison, slice_cap * sizeof(Hit)));
    UNIT_CHECK(starts.alloc(v.poison, total * 4));
    pwa::Events<2> ev;
    UNIT_CHECK(ev.create());
    float ms = 0.f, part = 0.f;
    UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
    UNIT_CHECK(pwa::recode_bytes(v.stream, s.text.as<uint8_t>(), s.tbytes / 16, tab.t));
    const uint64_t mask_threads = (uint64_t)n_pat * s.rows * kMaxWords;
    approx_masks_rev_kernel<<<(uint32_t)((mask_threads + 255) / 256), 256, 0, v.stream>>>(s.blob.as<uint8_t>(), s.d_pats.as<Pat>(), n_pat, s.rows, tab,
                                                                                          s.peq.as<uint64_t>());
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    UNIT_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    uint64_t slices = 0;
    for (uint64_t h0 = 0; h0 < total; h0 += slice_cap, ++slices) {
        const uint64_t h1 = std::min(h0 + slice_cap, total);
        UNIT_CHECK(hipMemcpyAsync(recs.p, sorted.data() + h0, (h1 - h0) * sizeof(Hit), hipMemcpyHostToDevice, v.stream));
        UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
        for (int W = 1; W <= kMaxWords; ++W) {
            const uint64_t c0 = std::max(h0, class_at[W]), c1 = std::min(h1, class_at[W + 1]);
            if (c0 >= c1) continue;
            start_kernel_t kern = start_kernel_for(W);
            const size_t lds = (size_t)s.rows * W * 64 * 8;
            if (lds > 64 * 1024) UNIT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((uint32_t)((c1 - c0 + 63) / 64)), dim3(64), lds, v.stream, s.text.as<uint8_t>(), s.peq.as<uint64_t>(), s.d_pats.as<Pat>(),
                               recs.as<Hit>() + (c0 - h0), (uint32_t)(c1 - c0), s.rows, starts.as<uint32_t>());
            UNIT_CHECK(hipGetLastError());
        }
        UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
        UNIT_CHECK(hipStreamSynchronize(v.stream));   // the records of the next slice go into the same buffer
        UNIT_CHECK(hipEventElapsedTime(&part, ev.e[0], ev.e[1]));
        ms += part;
    }
    UNIT_CHECK(hipMemcpyAsync(start_out, starts.p, total * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    uint64_t columns = 0;   // what the lanes scanned, read off their answers: e - start, or the whole bound where there is none
    for (const Hit& h : sorted) columns += start_out[h.out] == kNoStart ? std::min<uint64_t>(h.end, (uint64_t)s.pats[h.pat].m + h.dist) : h.end - start_out[h.out];
    *v.starts_stats = pwa::ApproxStartsStats{ms, total, columns};
    if (v.debug)
        std::fprintf(stderr, "[pwa] approx starts: %llu hits, %llu slices, %llu columns, device %.3f ms\n", (unsigned long long)total, (unsigned long long)slices,
                     (unsigned long long)columns, ms);
}

}  // namespace

extern "C" {

int pwa_approx_plan(uint64_t n, const uint32_t* pat_len, const uint32_t* max_dist, uint32_t n_pat, uint32_t chunk, uint32_t* task_pat,
                    uint64_t* task_scan_lo, uint64_t* task_lo, uint64_t* task_hi, uint64_t cap, uint64_t* n_tasks) {
    if (!n_tasks || !chunk || ((!pat_len || !max_dist) && n_pat)) return PWA_E_INVALID;
    for (uint32_t q = 0; q < n_pat; ++q)
        if (!pat_len[q]) return PWA_E_INVALID;
    const uint64_t per_pat = n / chunk + (n % chunk != 0);
    *n_tasks = per_pat * n_pat;
    if (*n_tasks > cap) return PWA_E_CAPACITY;
    if (*n_tasks && (!task_pat || !task_scan_lo || !task_lo || !task_hi)) return PWA_E_INVALID;
    uint64_t t = 0;
    for (uint32_t q = 0; q < n_pat; ++q) {
        const uint64_t w = (uint64_t)pat_len[q] + std::min(max_dist[q], pat_len[q]);
        for (uint64_t lo = 0; lo < n; lo += chunk, ++t) {
            task_pat[t] = q;
            task_scan_lo[t] = (lo > w ? lo - w : 0) & ~15ull;
            task_lo[t] = lo;
            task_hi[t] = std::min<uint64_t>(lo + chunk, n);
        }
    }
    return PWA_OK;
}

int pwa_approx_find(pwa_ctx* ctx, const uint8_t* text, uint64_t n, const uint8_t* pat_bytes, const uint64_t* pat_off, uint32_t n_pat,
                    const uint32_t* max_dist, uint32_t* counts_out, int32_t* best_dist_out, uint32_t* best_end_out) {
    if (!ctx || !pat_off || (!text && n) || ((!max_dist || !counts_out) && n_pat) || (!pat_bytes && pat_off[n_pat] != pat_off[0])) return PWA_E_INVALID;
    pwa::ApproxCtxView v = pwa::approx_ctx_view(ctx);
    CodeTable tab;
    uint32_t sigma = 0;
    if (const int rc = validate(v, "pwa_approx_find", n, pat_bytes, pat_off, n_pat, tab, sigma)) return rc;
    return pwa::guarded(v, [&] {
        Search s;
        count_pass(v, s, text, n, pat_bytes, pat_off, n_pat, max_dist, tab, sigma);
        for (uint32_t q = 0; q < n_pat; ++q) {
            counts_out[q] = s.h_cnt[q];
            const bool hit = s.h_best[q] != kNoBest;
            if (best_dist_out) best_dist_out[q] = hit ? (int32_t)(s.h_best[q] >> 32) : -1;
            if (best_end_out) best_end_out[q] = hit ? (uint32_t)s.h_best[q] : 0;
        }
    });
}

int pwa_approx_occurrences(pwa_ctx* ctx, const uint8_t* text, uint64_t n, const uint8_t* pat_bytes, const uint64_t* pat_off, uint32_t n_pat,
                           const uint32_t* max_dist, uint64_t* occ_off, uint64_t* occ, uint64_t cap, uint64_t* needed) {
    if (!ctx || !pat_off || !occ_off || (!text && n) || (!max_dist && n_pat) || (!occ && cap) || (!pat_bytes && pat_off[n_pat] != pat_off[0]))
        return PWA_E_INVALID;
    pwa::ApproxCtxView v = pwa::approx_ctx_view(ctx);
    CodeTable tab;
    uint32_t sigma = 0;
    if (const int rc = validate(v, "pwa_approx_occurrences", n, pat_bytes, pat_off, n_pat, tab, sigma)) return rc;
    return pwa::guarded(v, [&] {
        Search s;
        count_pass(v, s, text, n, pat_bytes, pat_off, n_pat, max_dist, tab, sigma);
        uint64_t total = 0;
        for (uint32_t q = 0; q < n_pat; ++q) {
            occ_off[q] = total;
            total += s.h_cnt[q];
        }
        occ_off[n_pat] = total;
        if (needed) *needed = total;
        if (total > cap) throw Fail{PWA_E_CAPACITY, "pwa_approx_occurrences: " + std::to_string(total) + " hits, capacity " + std::to_string(cap)};
        if (total) fill_pass(v, s, occ);
    });
}

int pwa_approx_starts(pwa_ctx* ctx, const uint8_t* text, uint64_t n, const uint8_t* pat_bytes, const uint64_t* pat_off, uint32_t n_pat,
                      const uint64_t* occ_off, const uint64_t* occ, uint32_t* start_out) {
    if (!ctx || !pat_off || !occ_off || (!text && n) || (!pat_bytes && pat_off[n_pat] != pat_off[0])) return PWA_E_INVALID;
    pwa::ApproxCtxView v = pwa::approx_ctx_view(ctx);
    CodeTable tab;
    uint32_t sigma = 0;
    if (const int rc = validate(v, "pwa_approx_starts", n, pat_bytes, pat_off, n_pat, tab, sigma)) return rc;
    for (uint32_t q = 0; q < n_pat; ++q) {
        if (occ_off[q + 1] < occ_off[q]) return PWA_E_INVALID;
        if (occ_off[q + 1] > occ_off[q] && (!occ || !start_out)) return PWA_E_INVALID;
        const uint64_t m = pat_off[q + 1] - pat_off[q];
        for (uint64_t x = occ_off[q]; x < occ_off[q + 1]; ++x) {
            const uint64_t e = occ[x] >> 32, d = occ[x] & 0xffffffffull;
            if (e == 0 || e > n || d > m) {
                *v.err = "pwa_approx_starts: hit " + std::to_string(x - occ_off[q]) + " of pattern " + std::to_string(q) + " (end " + std::to_string(e) +
                         ", dist " + std::to_string(d) + ") lies outside a text of " + std::to_string(n) + " and a pattern of " + std::to_string(m);
                return PWA_E_INVALID;
            }
        }
    }
    if (n_pat && occ_off[n_pat] - occ_off[0] > 0xffffffffull) {
        *v.err = "pwa_approx_starts: more than 2^32 - 1 hits in one call";
        return PWA_E_CAPACITY;
    }
    return pwa::guarded(v, [&] {
        *v.starts_stats = pwa::ApproxStartsStats{};
        if (!n_pat || occ_off[n_pat] == occ_off[0]) return;
        Search s;
        starts_pass(v, s, text, n, pat_bytes, pat_off, n_pat, occ_off, occ, tab, sigma, start_out);
    });
}

int pwa_approx_starts_last_stats(const pwa_ctx* ctx, float* ms, uint64_t* hits, uint64_t* columns) {
    if (!ctx) return PWA_E_INVALID;
    const pwa::ApproxStartsStats& st = pwa::approx_starts_stats_of(ctx);
    if (ms) *ms = st.ms;
    if (hits) *hits = st.hits;
    if (columns) *columns = st.columns;
    return PWA_OK;
}

int pwa_approx_minima(uint64_t n, const uint32_t* pat_len, const uint32_t* max_dist, uint32_t n_pat, uint64_t* occ_off, uint64_t* occ) {
    if (!occ_off || ((!pat_len || !max_dist) && n_pat)) return PWA_E_INVALID;
    if (n_pat && occ_off[n_pat] != occ_off[0] && !occ) return PWA_E_INVALID;
    // the whole list is checked before any of it moves
    for (uint32_t q = 0; q < n_pat; ++q) {
        if (!pat_len[q] || occ_off[q + 1] < occ_off[q]) return PWA_E_INVALID;
        const uint64_t kq = std::min(max_dist[q], pat_len[q]);
        uint64_t before = 0;
        for (uint64_t x = occ_off[q]; x < occ_off[q + 1]; ++x) {
            const uint64_t e = occ[x] >> 32, d = occ[x] & 0xffffffffull;
            if (e <= before || e > n || d > kq) return PWA_E_INVALID;
            before = e;
        }
    }
    uint64_t kept = n_pat ? occ_off[0] : 0, lo = kept;
    for (uint32_t q = 0; q < n_pat; ++q) {
        const uint64_t hi = occ_off[q + 1], m = pat_len[q], above = std::min<uint64_t>(max_dist[q], m) + 1;   // c of a column without a hit
        occ_off[q] = kept;
        for (uint64_t x = lo; x < hi;) {
            const uint64_t e = occ[x] >> 32, d = occ[x] & 0xffffffffull;
            const uint64_t left = x > lo && (occ[x - 1] >> 32) + 1 == e ? (occ[x - 1] & 0xffffffffull) : e == 1 ? m : above;
            uint64_t f = x;   // the plateau's last hit: adjacent ends of the same distance
            while (f + 1 < hi && (occ[f + 1] >> 32) == (occ[f] >> 32) + 1 && (occ[f + 1] & 0xffffffffull) == d) ++f;
            const uint64_t ef = occ[f] >> 32;
            const bool rises = ef == n || (f + 1 < hi && (occ[f + 1] >> 32) == ef + 1 ? (occ[f + 1] & 0xffffffffull) : above) > d;
            const uint64_t key = occ[x];   // (x - 1 was read above, before anything at or after kept <= x is written)
            if (left > d && rises) occ[kept++] = key;
            x = f + 1;
        }
        lo = hi;
    }
    if (n_pat) occ_off[n_pat] = kept;
    return PWA_OK;
}

int pwa_approx_last_stats(const pwa_ctx* ctx, float* count_ms, float* fill_ms, uint64_t* tasks, uint64_t* columns) {
    if (!ctx) return PWA_E_INVALID;
    const pwa::ApproxStats& st = pwa::approx_stats_of(ctx);
    if (count_ms) *count_ms = st.count_ms;
    if (fill_ms) *fill_ms = st.fill_ms;
    if (tasks) *tasks = st.tasks;
    if (columns) *columns = st.columns;
    return PWA_OK;
}

}  // extern "C"
