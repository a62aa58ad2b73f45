// chain_kernels.hip -- the chaining entries of include/pwalign.h (pwa_chain_plan, pwa_chain_anchors, pwa_chain_last_stats): validation,
// the host-only planner of ranges of consecutive reads under the PWA_RANGE_BYTES budget, the stages that run a plan (buffers, the
// launch list and the kernel of each range, the results).  Kernel: chain.hip.h.
#include "../../include/pwalign.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "chain.hip.h"
#include "chain_ctx.h"

using namespace pwa::chain;
using pwa::Dev;
using pwa::Fail;

namespace {

constexpr uint32_t kNoRead = 0xFFFFFFFFu;
constexpr uint64_t kAnchorBytes = 20, kRecordBytes = 4 * kRecWords;   // t, q, len, f, pred; the result record

struct Call {
    const uint32_t *t = nullptr, *q = nullptr, *len = nullptr;
    const uint64_t* off = nullptr;
    uint32_t n_reads = 0;
    uint32_t lookback = 0, max_dist = 0, bandwidth = 0, gap_scale = 0;
};

// Pointers and parameters, then the reads in order: the code, the first offending read in `bad`, what to say in `what`
int validate(const Call& c, uint32_t& bad, std::string& what) {
    bad = kNoRead;
    if (c.n_reads && (!c.off || !c.t || !c.q || !c.len)) {
        what = "a required pointer is null";
        return PWA_E_INVALID;
    }
    if (c.lookback < 1 || c.lookback > 512 || c.max_dist < 1 || c.max_dist > (1u << 30) || c.bandwidth > (1u << 20) || c.gap_scale > 1024) {
        what = "a parameter is outside its range (lookback 1 .. 512, max_dist 1 .. 2^30, bandwidth 0 .. 2^20, gap_scale 0 .. 1024)";
        return PWA_E_INVALID;
    }
    for (uint32_t r = 0; r < c.n_reads; ++r) {
        const auto fail = [&](int code, const char* why) {
            bad = r;
            what = "read " + std::to_string(r) + ": " + why;
            return code;
        };
        if (c.off[r + 1] < c.off[r]) return fail(PWA_E_INVALID, "anc_off decreases");
        if (c.off[r + 1] - c.off[r] > (1u << 24)) return fail(PWA_E_CAPACITY, "more than 2^24 anchors");
        uint64_t sum = 0, px = 0, py = 0;
        for (uint64_t k = c.off[r]; k < c.off[r + 1]; ++k) {
            if (!c.len[k]) return fail(PWA_E_INVALID, "an anchor of length 0");
            const uint64_t x = (uint64_t)c.t[k] + c.len[k], y = (uint64_t)c.q[k] + c.len[k];
            if (x >= (1ull << 31) || y >= (1ull << 31)) return fail(PWA_E_CAPACITY, "an anchor ends at or beyond 2^31");
            if (k > c.off[r] && (x < px || (x == px && y < py))) return fail(PWA_E_INVALID, "anchors out of (x, y) order");
            px = x;
            py = y;
            sum += c.len[k];
        }
        if (sum >= (1ull << 30)) return fail(PWA_E_CAPACITY, "anchor lengths sum to 2^30 or more");
    }
    return PWA_OK;
}

// ---- the planner: host only, a function of the validated call and a budget

struct Range {
    uint64_t k0 = 0, k1 = 0;    // reads
    uint64_t a0 = 0, a1 = 0;    // anchors
    std::vector<Read> reads;    // the launch list: the reads with anchors, longest first, ties in read order
};

std::vector<Range> plan_ranges(const Call& c, uint64_t budget) {
    std::vector<Range> ranges;
    for (const pwa::Run& cut : pwa::cut_runs(c.n_reads, budget, [&](uint64_t r) { return kAnchorBytes * (c.off[r + 1] - c.off[r]) + kRecordBytes; })) {
        Range g;
        g.k0 = cut.k0;
        g.k1 = cut.k1;
        g.a0 = c.off[g.k0];
        g.a1 = c.off[g.k1];
        for (uint64_t r = g.k0; r < g.k1; ++r)
            if (c.off[r + 1] > c.off[r]) g.reads.push_back(Read{c.off[r] - g.a0, (uint32_t)(c.off[r + 1] - c.off[r]), (uint32_t)(r - g.k0)});
        if (g.reads.empty()) continue;   // every read of it is empty: nothing to launch
        std::stable_sort(g.reads.begin(), g.reads.end(), [](const Read& a, const Read& b) { return a.n > b.n; });
        ranges.push_back(std::move(g));
    }
    return ranges;
}

// ---- the stages of a call over its plan

struct Outputs {
    int32_t* score;
    uint32_t *count, *last, *span;
    int32_t *diag, *f, *pred;
};

// The device buffers of a call -- the fault word for all of it, the others handed out again to every range
struct Buffers {
    Dev t, q, len, f, pred, reads, rec, fault;
    std::vector<int32_t> h_rec;
    bool used = false;

    void take(const pwa::ChainCtxView& v, const std::vector<Range>& ranges) {
        uint64_t max_a = 0, max_l = 0, max_n = 0;
        for (const Range& g : ranges) {
            max_a = std::max(max_a, g.a1 - g.a0);
            max_l = std::max<uint64_t>(max_l, g.reads.size());
            max_n = std::max(max_n, g.k1 - g.k0);
        }
        for (Dev* d : {&t, &q, &len, &f, &pred}) UNIT_CHECK(d->alloc(v.poison, max_a * 4));
        UNIT_CHECK(reads.alloc(v.poison, max_l * sizeof(Read)));
        UNIT_CHECK(rec.alloc(v.poison, max_n * kRecordBytes));
        UNIT_CHECK(fault.alloc(v.poison, 4));
    }
    // Before a range launches: the buffers of the range before, once it is through with them, handed out again
    void again(const pwa::ChainCtxView& v) {
        if (used) {
            UNIT_CHECK(hipStreamSynchronize(v.stream));
            for (Dev* d : {&t, &q, &len, &f, &pred, &reads, &rec}) UNIT_CHECK(d->again(v.poison));
        }
        used = true;
    }
};

using Kernel = void (*)(const Params);
Kernel kernel_for(uint32_t lookback) {
    return lookback <= 64 ? chain_kernel<1> : lookback <= 128 ? chain_kernel<2> : lookback <= 256 ? chain_kernel<4> : chain_kernel<8>;
}

void launch_range(const Call& c, const pwa::ChainCtxView& v, const Buffers& b, const pwa::Events<2>& ev, const Range& g) {
    const uint64_t na = g.a1 - g.a0;
    const uint32_t nl = (uint32_t)g.reads.size();
    UNIT_CHECK(hipMemcpyAsync(b.t.p, c.t + g.a0, na * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.q.p, c.q + g.a0, na * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.len.p, c.len + g.a0, na * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.reads.p, g.reads.data(), nl * sizeof(Read), hipMemcpyHostToDevice, v.stream));
    const Params p{b.t.as<uint32_t>(), b.q.as<uint32_t>(), b.len.as<uint32_t>(), b.reads.as<Read>(), nl, (int32_t)c.lookback, (int32_t)c.max_dist,
                   (int32_t)c.bandwidth, c.gap_scale, b.f.as<int32_t>(), b.pred.as<int32_t>(), b.rec.as<int32_t>(), b.fault.as<uint32_t>()};
    UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
    hipLaunchKernelGGL(kernel_for(c.lookback), dim3((nl + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, v.stream, p);
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
}

// The range's results back, the one synchronisation, and its reads' places in the caller's arrays
void collect_range(const Call& c, const pwa::ChainCtxView& v, Buffers& b, const pwa::Events<2>& ev, const Range& g, const Outputs& o, pwa::ChainStats& st) {
    const uint64_t na = g.a1 - g.a0;
    b.h_rec.assign((g.k1 - g.k0) * kRecWords, 0);
    UNIT_CHECK(hipMemcpyAsync(b.h_rec.data(), b.rec.p, (g.k1 - g.k0) * kRecordBytes, hipMemcpyDeviceToHost, v.stream));
    if (o.f) UNIT_CHECK(hipMemcpyAsync(o.f + g.a0, b.f.p, na * 4, hipMemcpyDeviceToHost, v.stream));
    if (o.pred) UNIT_CHECK(hipMemcpyAsync(o.pred + g.a0, b.pred.p, na * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    float ms = 0.f;
    UNIT_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    st.chain_ms += ms;
    st.anchors += na;
    st.ranges += 1;
    for (const Read& R : g.reads) {   // a read without anchors keeps the host's answer: its record was never written
        const uint64_t r = g.k0 + R.out;
        const int32_t* rec = b.h_rec.data() + (uint64_t)R.out * kRecWords;
        o.score[r] = rec[0];
        o.count[r] = (uint32_t)rec[1];
        o.last[r] = (uint32_t)rec[2];
        for (int k = 0; k < 4; ++k) o.span[4 * r + k] = (uint32_t)rec[3 + k];
        o.diag[2 * r] = rec[7];
        o.diag[2 * r + 1] = rec[8];
    }
}

void run(const Call& c, const pwa::ChainCtxView& v, const Outputs& o) {
    for (uint32_t r = 0; r < c.n_reads; ++r) {   // the answer of a read without anchors; the others are overwritten
        o.score[r] = 0;
        o.count[r] = 0;
        o.last[r] = kNoRead;
        std::fill_n(o.span + 4 * (uint64_t)r, 4, 0u);
        o.diag[2 * (uint64_t)r] = o.diag[2 * (uint64_t)r + 1] = 0;
    }
    pwa::ChainStats st;
    if (!c.n_reads || c.off[c.n_reads] == c.off[0]) {   // nothing for the device to do
        *v.stats = st;
        return;
    }
    UNIT_CHECK(hipSetDevice(v.device));
    uint64_t budget = v.range_bytes;
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        UNIT_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<uint64_t>((uint64_t)(free_b * 0.6), 48ull << 30);
    }
    const std::vector<Range> ranges = plan_ranges(c, budget);
    Buffers b;
    b.take(v, ranges);
    UNIT_CHECK(hipMemsetAsync(b.fault.p, 0, 4, v.stream));
    pwa::Events<2> ev;
    UNIT_CHECK(ev.create());
    for (const Range& g : ranges) {
        b.again(v);
        launch_range(c, v, b, ev, g);
        collect_range(c, v, b, ev, g, o, st);
    }
    uint32_t fault = 0;
    UNIT_CHECK(hipMemcpy(&fault, b.fault.p, 4, hipMemcpyDeviceToHost));
    if (fault) throw Fail{PWA_E_HIP, "pwa_chain_anchors: a back-walk left its chain (internal error)"};
    *v.stats = st;
    if (v.debug)
        std::fprintf(stderr, "[pwa] chain: %u reads, %llu anchors, %llu ranges, lookback %u, %.3f ms\n", c.n_reads, (unsigned long long)st.anchors,
                     (unsigned long long)st.ranges, c.lookback, st.chain_ms);
}

}  // namespace

extern "C" {

int pwa_chain_plan(const uint32_t* anc_t, const uint32_t* anc_q, const uint32_t* anc_len, const uint64_t* anc_off, uint32_t n_reads, uint32_t lookback,
                   uint32_t max_dist, uint32_t bandwidth, uint32_t gap_scale, uint64_t budget_bytes, uint32_t* bad_read, uint64_t* n_ranges) {
    const Call c{anc_t, anc_q, anc_len, anc_off, n_reads, lookback, max_dist, bandwidth, gap_scale};
    uint32_t bad = kNoRead;
    std::string what;
    int rc = PWA_E_NOMEM;
    uint64_t count = 0;
    try {
        rc = validate(c, bad, what);
        if (rc == PWA_OK) count = plan_ranges(c, budget_bytes ? budget_bytes : UINT64_MAX).size();
    } catch (const std::bad_alloc&) {
        rc = PWA_E_NOMEM;
    }
    if (bad_read) *bad_read = bad;
    if (n_ranges) *n_ranges = count;
    return rc;
}

int pwa_chain_anchors(pwa_ctx* ctx, const uint32_t* anc_t, const uint32_t* anc_q, const uint32_t* anc_len, const uint64_t* anc_off, uint32_t n_reads,
                      uint32_t lookback, uint32_t max_dist, uint32_t bandwidth, uint32_t gap_scale, int32_t* score_out, uint32_t* count_out,
                      uint32_t* last_out, uint32_t* span_out, int32_t* diag_out, int32_t* f_out, int32_t* pred_out) {
    if (!ctx) return PWA_E_INVALID;
    pwa::ChainCtxView v = pwa::chain_ctx_view(ctx);
    const Call c{anc_t, anc_q, anc_len, anc_off, n_reads, lookback, max_dist, bandwidth, gap_scale};
    if (n_reads && (!score_out || !count_out || !last_out || !span_out || !diag_out)) {
        *v.err = "pwa_chain_anchors: a required pointer is null";
        return PWA_E_INVALID;
    }
    uint32_t bad = kNoRead;
    std::string what;
    if (const int rc = validate(c, bad, what)) {
        *v.err = "pwa_chain_anchors: " + what;
        return rc;
    }
    return pwa::guarded(v, [&] { run(c, v, Outputs{score_out, count_out, last_out, span_out, diag_out, f_out, pred_out}); });
}

int pwa_chain_last_stats(const pwa_ctx* ctx, float* chain_ms, uint64_t* anchors, uint64_t* ranges) {
    if (!ctx) return PWA_E_INVALID;
    const pwa::ChainStats& st = pwa::chain_stats_of(ctx);
    if (chain_ms) *chain_ms = st.chain_ms;
    if (anchors) *anchors = st.anchors;
    if (ranges) *ranges = st.ranges;
    return PWA_OK;
}

}  // extern "C"
