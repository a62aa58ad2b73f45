// chain_kernels.hip -- the chaining entries of include/pwalign.h (pwa_chain_plan, pwa_chain_anchors, pwa_chain_last_stats): validation,
// the host-only planner of ranges of consecutive reads under the PWA_RANGE_BYTES budget, the stages that run a plan (buffers, the
// launch list and the kernel of each range, the results).  Kernel: chain.hip.h.  Behind them the top-N entries
// (pwa_chain_top_plan, pwa_chain_top, pwa_chain_top_last_stats, pwa_mapq): the same DP on the call's own buffers, then the candidate
// sort (the suffix-array unit's, sufarr_ctx.h) and the selection kernel of chain_top.hip.h.
#include "../../include/pwalign.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "chain.hip.h"
#include "chain_ctx.h"
#include "chain_top.hip.h"
#include "sufarr_ctx.h"

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

std::vector<Range> plan_ranges(const Call& c, uint64_t budget, uint64_t anchor_bytes = kAnchorBytes, uint64_t read_bytes = kRecordBytes) {
    std::vector<Range> ranges;
    for (const pwa::Run& cut : pwa::cut_runs(c.n_reads, budget, [&](uint64_t r) { return anchor_bytes * (c.off[r + 1] - c.off[r]) + read_bytes; })) {
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

// ---- the top-N chains of every read: validation, the stages of a range, the results

// per anchor t, q, len, f, pred, the mark, two sort keys and two sort values; per read its chain slots and its head
constexpr uint64_t kTopAnchorBytes = 48;
uint64_t top_read_bytes(uint32_t max_chains) { return 4ull * kTopRecWords * max_chains + 4 * kTopHeadWords; }

struct TopCall {
    Call c;
    uint32_t max_chains = 0, min_score = 0, min_count = 0, flags = 0;
};

int validate_top(const TopCall& c, uint32_t& bad, std::string& what) {
    bad = kNoRead;
    if (c.c.n_reads && (!c.c.off || !c.c.t || !c.c.q || !c.c.len)) {
        what = "a required pointer is null";
        return PWA_E_INVALID;
    }
    if (c.max_chains < 1 || c.max_chains > 16 || c.min_score < 1 || c.min_score > (1u << 30) || c.min_count < 1 || c.min_count > (1u << 24) ||
        (c.flags & ~(uint32_t)PWA_CHAIN_ROOTED)) {
        what = "a parameter is outside its range (max_chains 1 .. 16, min_score 1 .. 2^30, min_count 1 .. 2^24, flags 0 or PWA_CHAIN_ROOTED)";
        return PWA_E_INVALID;
    }
    return validate(c.c, bad, what);
}

struct TopOutputs {
    uint32_t* n_chains;
    int32_t* score;
    uint32_t *count, *last, *span;
    int32_t *diag, *branch;
    uint32_t* mapq;
    int32_t *f, *pred, *chain_id;
};

struct TopBuffers {
    Dev t, q, len, f, pred, mark, key, val, reads, rec, head, fault;
    pwa::SortScratch sc;
    std::vector<int32_t> h_rec;
    std::vector<uint32_t> h_head;
    bool used = false;

    void take(const pwa::ChainCtxView& v, const std::vector<Range>& ranges, uint32_t max_chains) {
        uint64_t max_a = 0, max_l = 0, max_n = 0;
        for (const Range& g : ranges) {
            max_a = std::max(max_a, g.a1 - g.a0);
            max_l = std::max<uint64_t>(max_l, g.reads.size());
            max_n = std::max(max_n, g.k1 - g.k0);
        }
        for (Dev* d : {&t, &q, &len, &f, &pred, &mark}) UNIT_CHECK(d->alloc(v.poison, max_a * 4));
        UNIT_CHECK(key.alloc(v.poison, max_a * 16));
        UNIT_CHECK(val.alloc(v.poison, max_a * 8));
        sc.alloc(v.poison, max_a);
        UNIT_CHECK(reads.alloc(v.poison, max_l * sizeof(Read)));
        UNIT_CHECK(rec.alloc(v.poison, max_n * max_chains * 4 * kTopRecWords));
        UNIT_CHECK(head.alloc(v.poison, max_n * 4 * kTopHeadWords));
        UNIT_CHECK(fault.alloc(v.poison, 4));
    }
    void again(const pwa::ChainCtxView& v) {
        if (used) {
            UNIT_CHECK(hipStreamSynchronize(v.stream));
            for (Dev* d : {&t, &q, &len, &f, &pred, &mark, &key, &val, &sc.hist, &sc.part, &sc.bits, &reads, &rec, &head}) UNIT_CHECK(d->again(v.poison));
        }
        used = true;
    }
};

// One range: the DP, the candidate order, the selection; events around the DP and around what follows it
void launch_top_range(const TopCall& tc, const pwa::ChainCtxView& v, const TopBuffers& b, pwa::SortScratch& sc, const pwa::Events<3>& ev, const Range& g) {
    const Call& c = tc.c;
    const uint64_t na = g.a1 - g.a0;
    const uint32_t nl = (uint32_t)g.reads.size();
    UNIT_CHECK(hipMemcpyAsync(b.t.p, c.t + g.a0, na * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.q.p, c.q + g.a0, na * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.len.p, c.len + g.a0, na * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.reads.p, g.reads.data(), nl * sizeof(Read), hipMemcpyHostToDevice, v.stream));
    const Params p{b.t.as<uint32_t>(), b.q.as<uint32_t>(), b.len.as<uint32_t>(), b.reads.as<Read>(), nl, (int32_t)c.lookback, (int32_t)c.max_dist,
                   (int32_t)c.bandwidth, c.gap_scale, b.f.as<int32_t>(), b.pred.as<int32_t>(), b.rec.as<int32_t>(), b.fault.as<uint32_t>()};
    const dim3 grid((nl + kWaves - 1) / kWaves), block(64 * kWaves);
    UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
    hipLaunchKernelGGL(kernel_for(c.lookback), grid, block, 0, v.stream, p);   // its record (the first words of rec) is written over below
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
    hipLaunchKernelGGL(chain_top_keys_kernel, grid, block, 0, v.stream, b.reads.as<Read>(), nl, b.f.as<int32_t>(), b.key.as<uint64_t>(), b.val.as<uint32_t>(),
                       b.mark.as<int32_t>());
    UNIT_CHECK(hipGetLastError());
    const int half = pwa::sort_pairs(v.stream, b.key.as<uint64_t>(), b.val.as<uint32_t>(), na, sc);
    const TopParams tp{b.t.as<uint32_t>(), b.q.as<uint32_t>(), b.len.as<uint32_t>(), b.reads.as<Read>(), nl, b.f.as<int32_t>(), b.pred.as<int32_t>(),
                       b.val.as<uint32_t>() + (uint64_t)half * na, b.mark.as<int32_t>(), tc.max_chains, (int32_t)tc.min_score, tc.min_count, tc.flags,
                       b.rec.as<int32_t>(), b.head.as<uint32_t>(), b.fault.as<uint32_t>()};
    hipLaunchKernelGGL(chain_top_kernel, grid, block, 0, v.stream, tp);
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[2], v.stream));
}

void collect_top_range(const TopCall& tc, const pwa::ChainCtxView& v, TopBuffers& b, const pwa::Events<3>& ev, const Range& g, const TopOutputs& o,
                       pwa::ChainTopStats& st) {
    const uint64_t na = g.a1 - g.a0, nk = g.k1 - g.k0, N = tc.max_chains;
    b.h_rec.assign(nk * N * kTopRecWords, 0);
    b.h_head.assign(nk * kTopHeadWords, 0);
    UNIT_CHECK(hipMemcpyAsync(b.h_rec.data(), b.rec.p, nk * N * 4 * kTopRecWords, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.h_head.data(), b.head.p, nk * 4 * kTopHeadWords, hipMemcpyDeviceToHost, v.stream));
    if (o.f) UNIT_CHECK(hipMemcpyAsync(o.f + g.a0, b.f.p, na * 4, hipMemcpyDeviceToHost, v.stream));
    if (o.pred) UNIT_CHECK(hipMemcpyAsync(o.pred + g.a0, b.pred.p, na * 4, hipMemcpyDeviceToHost, v.stream));
    if (o.chain_id) UNIT_CHECK(hipMemcpyAsync(o.chain_id + g.a0, b.mark.p, na * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    float ms = 0.f;
    UNIT_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    st.chain_ms += ms;
    UNIT_CHECK(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
    st.top_ms += ms;
    st.anchors += na;
    st.ranges += 1;
    if (o.chain_id)   // the marks, with those of dropped walks folded into "no kept chain"
        for (uint64_t k = g.a0; k < g.a1; ++k)
            if (o.chain_id[k] < 0) o.chain_id[k] = -1;
    for (const Read& R : g.reads) {   // a read without anchors keeps the host's answer: nothing of it was written
        const uint64_t r = g.k0 + R.out;
        const uint32_t* head = b.h_head.data() + (uint64_t)R.out * kTopHeadWords;
        const uint32_t kept = std::min<uint32_t>(head[0], tc.max_chains);
        o.n_chains[r] = kept;
        st.rounds += head[1];
        for (uint32_t k = 0; k < kept; ++k) {
            const int32_t* rec = b.h_rec.data() + ((uint64_t)R.out * N + k) * kTopRecWords;
            const uint64_t s = r * N + k;
            o.score[s] = rec[0];
            o.count[s] = (uint32_t)rec[1];
            o.last[s] = (uint32_t)rec[2];
            for (int j = 0; j < 4; ++j) o.span[4 * s + j] = (uint32_t)rec[3 + j];
            o.diag[2 * s] = rec[7];
            o.diag[2 * s + 1] = rec[8];
            o.branch[s] = rec[9];
        }
        if (o.mapq && kept) o.mapq[r] = (uint32_t)pwa_mapq(o.score[r * N], (int32_t)head[2], o.count[r * N]);
    }
}

void run_top(const TopCall& tc, const pwa::ChainCtxView& v, pwa::ChainTopStats* stats, const TopOutputs& o) {
    const Call& c = tc.c;
    const uint64_t N = tc.max_chains;
    for (uint64_t r = 0; r < c.n_reads; ++r) {   // the unused slots, and all of a read without anchors
        o.n_chains[r] = 0;
        if (o.mapq) o.mapq[r] = 0;
        for (uint64_t s = r * N; s < (r + 1) * N; ++s) {
            o.score[s] = 0;
            o.count[s] = 0;
            o.last[s] = kNoRead;
            o.branch[s] = -1;
            std::fill_n(o.span + 4 * s, 4, 0u);
            o.diag[2 * s] = o.diag[2 * s + 1] = 0;
        }
    }
    pwa::ChainTopStats st;
    if (!c.n_reads || c.off[c.n_reads] == c.off[0]) {   // nothing for the device to do
        *stats = st;
        return;
    }
    UNIT_CHECK(hipSetDevice(v.device));
    uint64_t budget = v.range_bytes;
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        UNIT_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<uint64_t>((uint64_t)(free_b * 0.6), 48ull << 30);
    }
    const std::vector<Range> ranges = plan_ranges(c, budget, kTopAnchorBytes, top_read_bytes(tc.max_chains));
    TopBuffers b;
    b.take(v, ranges, tc.max_chains);
    UNIT_CHECK(hipMemsetAsync(b.fault.p, 0, 4, v.stream));
    pwa::Events<3> ev;
    UNIT_CHECK(ev.create());
    for (const Range& g : ranges) {
        b.again(v);
        launch_top_range(tc, v, b, b.sc, ev, g);
        collect_top_range(tc, v, b, ev, g, o, st);
    }
    uint32_t fault = 0;
    UNIT_CHECK(hipMemcpy(&fault, b.fault.p, 4, hipMemcpyDeviceToHost));
    if (fault) throw Fail{PWA_E_HIP, "pwa_chain_top: a walk left its chain or a loop met its bound (internal error)"};
    *stats = st;
    if (v.debug)
        std::fprintf(stderr, "[pwa] chain top: %u reads, %llu anchors, %llu ranges, %llu rounds, chain %.3f ms, top %.3f ms\n", c.n_reads,
                     (unsigned long long)st.anchors, (unsigned long long)st.ranges, (unsigned long long)st.rounds, st.chain_ms, st.top_ms);
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

int pwa_mapq(int32_t s1, int32_t s2, uint32_t c1) {
    if (s1 <= 0) return 0;
    const int64_t a = s1, b = std::min<int64_t>(std::max<int64_t>(s2, 0), a), c = std::min<uint32_t>(c1, 10);
    return (int)std::min<int64_t>(60, 60 * (a - b) * c / (10 * a));
}

int pwa_chain_top_plan(const uint32_t* anc_t, const uint32_t* anc_q, const uint32_t* anc_len, const uint64_t* anc_off, uint32_t n_reads, uint32_t lookback,
                       uint32_t max_dist, uint32_t bandwidth, uint32_t gap_scale, uint32_t max_chains, uint32_t min_score, uint32_t min_count,
                       uint32_t flags, uint64_t budget_bytes, uint32_t* bad_read, uint64_t* n_ranges) {
    const TopCall c{{anc_t, anc_q, anc_len, anc_off, n_reads, lookback, max_dist, bandwidth, gap_scale}, max_chains, min_score, min_count, flags};
    uint32_t bad = kNoRead;
    std::string what;
    int rc = PWA_E_NOMEM;
    uint64_t count = 0;
    try {
        rc = validate_top(c, bad, what);
        if (rc == PWA_OK) count = plan_ranges(c.c, budget_bytes ? budget_bytes : UINT64_MAX, kTopAnchorBytes, top_read_bytes(max_chains)).size();
    } catch (const std::bad_alloc&) {
        rc = PWA_E_NOMEM;
    }
    if (bad_read) *bad_read = bad;
    if (n_ranges) *n_ranges = count;
    return rc;
}

int pwa_chain_top(pwa_ctx* ctx, const uint32_t* anc_t, const uint32_t* anc_q, const uint32_t* anc_len, const uint64_t* anc_off, uint32_t n_reads,
                  uint32_t lookback, uint32_t max_dist, uint32_t bandwidth, uint32_t gap_scale, uint32_t max_chains, uint32_t min_score,
                  uint32_t min_count, uint32_t flags, uint32_t* n_chains_out, int32_t* score_out, uint32_t* count_out, uint32_t* last_out,
                  uint32_t* span_out, int32_t* diag_out, int32_t* branch_out, uint32_t* mapq_out, int32_t* f_out, int32_t* pred_out,
                  int32_t* chain_id_out) {
    if (!ctx) return PWA_E_INVALID;
    pwa::ChainCtxView v = pwa::chain_ctx_view(ctx);
    const TopCall c{{anc_t, anc_q, anc_len, anc_off, n_reads, lookback, max_dist, bandwidth, gap_scale}, max_chains, min_score, min_count, flags};
    if (n_reads && (!n_chains_out || !score_out || !count_out || !last_out || !span_out || !diag_out || !branch_out)) {
        *v.err = "pwa_chain_top: a required pointer is null";
        return PWA_E_INVALID;
    }
    uint32_t bad = kNoRead;
    std::string what;
    if (const int rc = validate_top(c, bad, what)) {
        *v.err = "pwa_chain_top: " + what;
        return rc;
    }
    return pwa::guarded(v, [&] {
        run_top(c, v, pwa::chain_top_stats_of(ctx),
                TopOutputs{n_chains_out, score_out, count_out, last_out, span_out, diag_out, branch_out, mapq_out, f_out, pred_out, chain_id_out});
    });
}

int pwa_chain_top_last_stats(const pwa_ctx* ctx, float* chain_ms, float* top_ms, uint64_t* anchors, uint64_t* rounds, uint64_t* ranges) {
    if (!ctx) return PWA_E_INVALID;
    const pwa::ChainTopStats& st = *pwa::chain_top_stats_of(const_cast<pwa_ctx*>(ctx));
    if (chain_ms) *chain_ms = st.chain_ms;
    if (top_ms) *top_ms = st.top_ms;
    if (anchors) *anchors = st.anchors;
    if (rounds) *rounds = st.rounds;
    if (ranges) *ranges = st.ranges;
    return PWA_OK;
}

}  // extern "C"
