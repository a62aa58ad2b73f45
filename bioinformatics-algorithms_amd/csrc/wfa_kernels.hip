// wfa_kernels.hip -- the wavefront-alignment entries of include/pwalign.h (pwa_wfa_plan, pwa_scores_wfa, pwa_align_wfa_batch(_cigar),
// pwa_align_wfa_codes_batch(_cigar), pwa_wfa_last_stats, and the semi-global pwa_wfa_sg_plan, pwa_scores_wfa_sg, pwa_align_wfa_sg_batch(_cigar)):
// validation, the conversion to penalties, the per-pair plan and bound, the host-only planner of ranges of consecutive pairs under the
// PWA_RANGE_BYTES budget, the stages that run a plan (buffers, the sweep and the walk of each range, the results), the CIGAR / MD:Z
// strings.  Kernels: wfa.hip.h.
#include "../../include/pwalign.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../host/format_ops.h"
#include "wfa.hip.h"
#include "wfa_ctx.h"

using namespace pwa::wfa;
using pwa::Dev;
using pwa::Fail;

namespace {

struct Scoring {
    int match = 0, mismatch = 0, go = 0, ge = 0;
    bool sg = false;   // the semi-global form: penalties per pattern symbol, pen.ed next to pen.e
    Pen pen{};
    uint32_t g = 1;
};

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// The scoring as penalties; PWA_E_INVALID where no penalty form exists
int convert(int match, int mismatch, int go, int ge, Scoring& sc) {
    const int64_t x0 = 2 * ((int64_t)match - mismatch), o0 = -2 * (int64_t)go, e0 = (int64_t)match - 2 * (int64_t)ge;
    if (go > 0 || ge > 0 || x0 <= 0 || e0 <= 0) return PWA_E_INVALID;
    const int64_t g = gcd64(gcd64(x0, o0), e0);
    if (x0 / g > 0x3fffffff || o0 / g > 0x3fffffff || e0 / g > 0x3fffffff) return PWA_E_CAPACITY;   // (no pair passes the range rule then)
    sc = Scoring{match, mismatch, go, ge, false, Pen{(uint32_t)(x0 / g), (uint32_t)(o0 / g), (uint32_t)(e0 / g), (uint32_t)(e0 / g)}, (uint32_t)g};
    return PWA_OK;
}

// The semi-global form's: counted per pattern symbol, because the text length an alignment consumes is not fixed
int convert_sg(int match, int mismatch, int go, int ge, Scoring& sc) {
    const int64_t x0 = (int64_t)match - mismatch, o0 = -(int64_t)go, i0 = -(int64_t)ge, d0 = (int64_t)match - ge;
    if (go > 0 || ge >= 0 || x0 <= 0 || d0 <= 0) return PWA_E_INVALID;
    const int64_t g = gcd64(gcd64(x0, o0), gcd64(i0, d0));
    if (x0 / g > 0x3fffffff || o0 / g > 0x3fffffff || i0 / g > 0x3fffffff || d0 / g > 0x3fffffff) return PWA_E_CAPACITY;   // (as above)
    sc = Scoring{match, mismatch, go, ge, true, Pen{(uint32_t)(x0 / g), (uint32_t)(o0 / g), (uint32_t)(i0 / g), (uint32_t)(d0 / g)}, (uint32_t)g};
    return PWA_OK;
}

int convert(bool sg, int match, int mismatch, int go, int ge, Scoring& sc) {
    return sg ? convert_sg(match, mismatch, go, ge, sc) : convert(match, mismatch, go, ge, sc);
}

// The geometry of a scoring's form
uint64_t cum_of(const Scoring& sc, uint32_t s, uint32_t n, uint32_t m) { return sc.sg ? cum<true>(s, n, m, sc.pen) : cum<false>(s, n, m, sc.pen); }
uint64_t ring_bytes_of(const Scoring& sc, uint32_t p_max, uint32_t n, uint32_t m) {
    return 4 * (sc.sg ? ring_words<true>(p_max, n, m, sc.pen) : ring_words<false>(p_max, n, m, sc.pen));
}

bool in_range(const Scoring& sc, uint64_t n, uint64_t m) {
    const uint64_t big = std::max<uint64_t>({(uint64_t)std::llabs(sc.match), (uint64_t)std::llabs(sc.mismatch), (uint64_t)std::llabs(sc.go) + (uint64_t)std::llabs(sc.ge)});
    return n + m + 2 < (1ull << 28) && (n + m + 2) * big < (1ull << 28);
}

struct Plan {
    uint32_t n = 0, m = 0;
    bool none = false;      // not found, decided here
    uint32_t p_max = 0;
    uint64_t cells = 0;     // of the wavefronts 0 .. p_max
};

// The bound and the planning unit of one pair inside the range rule
Plan plan_pair(const Scoring& sc, uint64_t n, uint64_t m, const int32_t* min_score) {
    Plan p;
    p.n = (uint32_t)n;
    p.m = (uint32_t)m;
    if (sc.sg) {   // all 'D', or for m >= n all mismatches on the main diagonal; at least n - m 'D' when the pattern is the longer
        const int64_t o = sc.pen.o, ed = sc.pen.ed, x = sc.pen.x;
        int64_t p_max = n ? o + (int64_t)n * ed : 0;
        if (m >= n) p_max = std::min(p_max, (int64_t)n * x);
        if (min_score) {
            const int64_t num = (int64_t)sc.match * (int64_t)n - (int64_t)*min_score, g = sc.g;
            p_max = std::min(p_max, num >= 0 ? num / g : -((-num + g - 1) / g));
        }
        if (p_max < 0 || (n > m && p_max < o + (int64_t)(n - m) * ed)) {
            p.none = true;
            return p;
        }
        p.p_max = (uint32_t)p_max;
        p.cells = cum<true>(p.p_max + 1, p.n, p.m, sc.pen);
        return p;
    }
    const int64_t o = sc.pen.o, e = sc.pen.e;
    int64_t p_max = (n ? o + (int64_t)n * e : 0) + (m ? o + (int64_t)m * e : 0);
    if (min_score) {
        const int64_t num = (int64_t)sc.match * (int64_t)(n + m) - 2 * (int64_t)*min_score, g = sc.g;
        const int64_t fl = num >= 0 ? num / g : -((-num + g - 1) / g);
        p_max = std::min(p_max, fl);
    }
    const int64_t gap = n == m ? 0 : o + (int64_t)(n > m ? n - m : m - n) * e;
    if (p_max < 0 || p_max < gap) {
        p.none = true;
        return p;
    }
    p.p_max = (uint32_t)p_max;
    p.cells = cum(p.p_max + 1, p.n, p.m, sc.pen);
    return p;
}

int32_t score_of(const Scoring& sc, const Plan& p, uint32_t pen) {
    if (sc.sg) return (int32_t)((int64_t)sc.match * p.n - (int64_t)sc.g * pen);
    return (int32_t)(((int64_t)sc.match * ((int64_t)p.n + p.m) - (int64_t)sc.g * pen) / 2);
}

// The forms of a call, and what a call keeps of the wavefronts under each: a ring and nothing else (scores), every wavefront
// (alignments from the stored offsets), or a ring and one code byte per planned cell (alignments from the codes).  The semi-global
// geometry exists for the ring and for the codes only
enum class Form { Offsets, Codes, Scores, SgScores, SgCodes };
enum class Keep { Ring, All, RingCodes };

struct FormInfo {
    bool sg;          // the geometry of the scoring: Scoring::sg of a call of this form
    Keep keep;
    void (*sweep)(SweepParams);
    void (*walk)(WalkParams);              // the walk over the stored offsets, or
    void (*codes_walk)(CodesWalkParams);   // the walk over the codes; neither for a score form
    bool ops;         // op lists, their counts and the fault word
    bool cells;       // end and start cells from the walk
    bool end_k;       // the end diagonal behind the penalty: the second of the
    uint32_t pen_words;   // words of penalty output per pair
    const char* label;    // in the debug line
};

const FormInfo& info(Form form) {
    static const FormInfo table[] = {
        {false, Keep::All, wfa_sweep_kernel<false>, wfa_walk_kernel, nullptr, true, false, false, 1, "align"},
        {false, Keep::RingCodes, wfa_codes_sweep_kernel, nullptr, wfa_codes_walk_kernel, true, false, false, 1, "align (codes)"},
        {false, Keep::Ring, wfa_sweep_kernel<true>, nullptr, nullptr, false, false, false, 1, "scores"},
        {true, Keep::Ring, wfa_sg_sweep_kernel, nullptr, nullptr, false, false, true, 2, "scores"},
        {true, Keep::RingCodes, wfa_sg_codes_sweep_kernel, nullptr, wfa_sg_codes_walk_kernel, true, true, true, 2, "align (codes)"},
    };
    return table[(int)form];
}

// A pair's workspace bytes, a multiple of 4: nothing for a pair the host ruled out
uint64_t ws_bytes_of(const FormInfo& f, const Scoring& sc, const Plan& p) {
    if (p.none) return 0;
    if (f.keep == Keep::All) return 12 * p.cells;
    const uint64_t ring = ring_bytes_of(sc, p.p_max, p.n, p.m);
    return f.keep == Keep::RingCodes ? ring + ((p.cells + 3) & ~3ull) : ring;   // the code plane behind the ring, up to the next int32
}

struct Call {
    pwa::WfaCtxView v;
    Scoring sc;
    const uint8_t* blob = nullptr;
    const uint64_t* seq_off = nullptr;
    uint32_t n_seq = 0;
    const uint32_t *pair_a = nullptr, *pair_b = nullptr;
    uint64_t n_pairs = 0;
    std::vector<Plan> plans;
};

// Scoring (of the form's geometry), required pointers (by the caller), indices and the range rule, in pair order; fills c.plans
int validate(Call& c, Form form, int match, int mismatch, int go, int ge, const int32_t* min_score, const char* who) {
    const bool sg = info(form).sg;
    if (const int rc = convert(sg, match, mismatch, go, ge, c.sc)) {
        *c.v.err = std::string(who) + (sg ? ": the scoring has no penalty form (gap_open <= 0, gap_extend < 0, match > mismatch, match - gap_extend > 0)"
                                          : ": the scoring has no penalty form (gap_open <= 0, gap_extend <= 0, match > mismatch, match - 2 gap_extend > 0)");
        return rc;
    }
    c.plans.resize(c.n_pairs);
    for (uint64_t k = 0; k < c.n_pairs; ++k) {
        const uint32_t a = c.pair_a[k], b = c.pair_b[k];
        if (a >= c.n_seq || b >= c.n_seq || c.seq_off[a + 1] < c.seq_off[a] || c.seq_off[b + 1] < c.seq_off[b] || c.seq_off[a + 1] > c.seq_off[c.n_seq] ||
            c.seq_off[b + 1] > c.seq_off[c.n_seq]) {
            *c.v.err = std::string(who) + ": pair " + std::to_string(k) + " names a sequence outside the list";
            return PWA_E_INVALID;
        }
        const uint64_t n = c.seq_off[a + 1] - c.seq_off[a], m = c.seq_off[b + 1] - c.seq_off[b];
        if (!in_range(c.sc, n, m)) {
            *c.v.err = std::string(who) + ": pair " + std::to_string(k) + " (" + std::to_string(n) + " x " + std::to_string(m) + ") exceeds the score range";
            return PWA_E_CAPACITY;
        }
        c.plans[k] = plan_pair(c.sc, n, m, min_score ? min_score + k : nullptr);
    }
    return PWA_OK;
}

// ---- the planner: host only, a function of the validated call, its form and a budget (pwa::selftest_wfa_plan checks it without a GPU)

struct Range {
    uint64_t k0 = 0, k1 = 0;
    uint64_t ws_bytes = 0, op_bytes = 0;
    std::vector<Pair> pairs;   // the launch list: the pairs the host did not rule out, longest plan first, ties in pair order; out = k - k0
};

struct RangePlan {
    std::vector<uint64_t> ws_at;   // [k]: first int32 of pair k's workspace slice in its range's workspace
    std::vector<uint64_t> op_at;   // [k]: first byte of pair k's op region (n + m bytes) in the call's op lists; [n_pairs]: their sum.  Zeros for a score form
    std::vector<Range> ranges;     // consecutive pairs, by workspace and op bytes together; one pair alone may exceed the budget
    uint64_t max_ws = 0, max_ops = 0, max_n = 0;   // the largest range's workspace bytes, op bytes and pairs: the capacities of the buffers
};

RangePlan plan_ranges(const Call& c, Form form, uint64_t budget) {
    const FormInfo& f = info(form);
    const uint64_t np = c.n_pairs;
    RangePlan rp;
    rp.ws_at.assign(np, 0);
    rp.op_at.assign(np + 1, 0);
    std::vector<uint64_t> ws(np);   // every pair's workspace bytes
    for (uint64_t k = 0; k < np; ++k) {
        ws[k] = ws_bytes_of(f, c.sc, c.plans[k]);
        rp.op_at[k + 1] = rp.op_at[k] + (f.ops ? c.plans[k].n + c.plans[k].m : 0);
    }
    std::vector<uint64_t> order;
    for (const pwa::Run& cut : pwa::cut_runs(np, budget, [&](uint64_t k) { return ws[k] + (rp.op_at[k + 1] - rp.op_at[k]); })) {
        Range r;
        r.k0 = cut.k0;
        r.k1 = cut.k1;
        r.op_bytes = rp.op_at[r.k1] - rp.op_at[r.k0];
        order.clear();
        for (uint64_t k = r.k0; k < r.k1; ++k) {
            rp.ws_at[k] = r.ws_bytes / 4;
            r.ws_bytes += ws[k];
            if (!c.plans[k].none) order.push_back(k);
        }
        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return c.plans[a].cells > c.plans[b].cells; });
        for (uint64_t k : order) {
            const Plan& p = c.plans[k];
            r.pairs.push_back(Pair{c.seq_off[c.pair_a[k]], c.seq_off[c.pair_b[k]], rp.ws_at[k], rp.op_at[k] - rp.op_at[r.k0], p.n, p.m, p.p_max, (uint32_t)(k - r.k0)});
        }
        rp.max_ws = std::max(rp.max_ws, r.ws_bytes);
        rp.max_ops = std::max(rp.max_ops, r.op_bytes);
        rp.max_n = std::max(rp.max_n, r.k1 - r.k0);
        rp.ranges.push_back(std::move(r));
    }
    return rp;
}

// ---- the stages of a call over its plan

// What run() brings back: penalty[k] = P or kNotFound; op lists packed pair after pair into `ops` (pair k at op_at[k], n + m bytes of
// room, n_ops[k] of them written).  The semi-global form: end_k[k] = the end diagonal, cells[4 k ..] = end (i, j), start (i, j) of an
// alignment call; zeros for a pair not found
struct Results {
    std::vector<uint32_t> penalty, n_ops, cells;
    std::vector<int32_t> end_k;
    std::vector<uint8_t> ops;
    std::vector<uint64_t> op_at;
};

// The device buffers of a call -- the blob and the fault word for all of it, the others handed out again to every range -- and the
// host side of a range's copies back.  A buffer the form does not have stays empty
struct Buffers {
    Dev blob, ws, pairs, pen, nops, ops, fault, cells;
    std::vector<uint32_t> h_pen, h_nops, h_cells;
    bool used = false;   // by a range of this call

    void take(const pwa::WfaCtxView& v, const FormInfo& f, const RangePlan& rp, uint64_t blob_bytes) {
        UNIT_CHECK(blob.alloc(v.poison, blob_bytes + kPad));
        UNIT_CHECK(ws.alloc(v.poison, rp.max_ws));
        UNIT_CHECK(pairs.alloc(v.poison, rp.max_n * sizeof(Pair)));
        UNIT_CHECK(pen.alloc(v.poison, rp.max_n * 4 * f.pen_words));
        if (f.cells) UNIT_CHECK(cells.alloc(v.poison, rp.max_n * 16));
        if (f.ops) {
            UNIT_CHECK(nops.alloc(v.poison, rp.max_n * 4));
            UNIT_CHECK(ops.alloc(v.poison, rp.max_ops));
            UNIT_CHECK(fault.alloc(v.poison, 4));
        }
    }
    // Before a range launches: the buffers of the range before, once it is through with them, handed out again
    void again(const pwa::WfaCtxView& v) {
        if (used) {
            UNIT_CHECK(hipStreamSynchronize(v.stream));
            for (Dev* d : {&ws, &pairs, &pen, &nops, &ops, &cells})
                if (d->p) UNIT_CHECK(d->again(v.poison));
        }
        used = true;
    }
};

// The sweep and, where the form has one, the walk of a range's launch list, between the three events
void launch_range(const pwa::WfaCtxView& v, const FormInfo& f, const Pen& pen, const Buffers& b, const pwa::Events<3>& ev, const Range& r) {
    const uint32_t nl = (uint32_t)r.pairs.size();
    const dim3 grid((nl + kWaves - 1) / kWaves), block(64 * kWaves);
    UNIT_CHECK(hipMemcpyAsync(b.pairs.p, r.pairs.data(), nl * sizeof(Pair), hipMemcpyHostToDevice, v.stream));
    const SweepParams sp{b.blob.as<uint8_t>(), b.pairs.as<Pair>(), nl, pen, b.ws.as<int32_t>(), b.pen.as<uint32_t>()};
    UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
    hipLaunchKernelGGL(f.sweep, grid, block, 0, v.stream, sp);
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
    if (f.codes_walk) {
        const CodesWalkParams wp{b.blob.as<uint8_t>(), b.pairs.as<Pair>(), nl, pen, b.ws.as<int32_t>(), b.pen.as<uint32_t>(), b.ops.as<uint8_t>(),
                                 b.nops.as<uint32_t>(), b.fault.as<uint32_t>(), b.cells.as<uint32_t>()};
        hipLaunchKernelGGL(f.codes_walk, grid, block, 0, v.stream, wp);
        UNIT_CHECK(hipGetLastError());
    } else if (f.walk) {
        const WalkParams wp{b.pairs.as<Pair>(), nl, pen, b.ws.as<int32_t>(), b.pen.as<uint32_t>(), b.ops.as<uint8_t>(), b.nops.as<uint32_t>(), b.fault.as<uint32_t>()};
        hipLaunchKernelGGL(f.walk, grid, block, 0, v.stream, wp);
        UNIT_CHECK(hipGetLastError());
    }
    UNIT_CHECK(hipEventRecord(ev.e[2], v.stream));
}

// The range's results back, the one synchronisation, and its pairs' places in `res`, in pair order (a pair left out of the launch keeps
// kNotFound and no ops; its slots were never written)
void collect_range(const Call& c, const FormInfo& f, Buffers& b, const pwa::Events<3>& ev, const Range& r, const RangePlan& rp, Results& res, pwa::WfaStats& st) {
    const pwa::WfaCtxView& v = c.v;
    const uint64_t cnt = r.k1 - r.k0;
    b.h_pen.assign(cnt * f.pen_words, kNotFound);
    b.h_nops.assign(cnt, 0);
    b.h_cells.assign(f.sg ? 4 * cnt : 0, 0);
    UNIT_CHECK(hipMemcpyAsync(b.h_pen.data(), b.pen.p, cnt * 4 * f.pen_words, hipMemcpyDeviceToHost, v.stream));
    if (f.cells) UNIT_CHECK(hipMemcpyAsync(b.h_cells.data(), b.cells.p, cnt * 16, hipMemcpyDeviceToHost, v.stream));
    if (f.ops) {
        UNIT_CHECK(hipMemcpyAsync(b.h_nops.data(), b.nops.p, cnt * 4, hipMemcpyDeviceToHost, v.stream));
        if (r.op_bytes) UNIT_CHECK(hipMemcpyAsync(res.ops.data() + rp.op_at[r.k0], b.ops.p, r.op_bytes, hipMemcpyDeviceToHost, v.stream));
    }
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    float sweep = 0.f, walk = 0.f;
    UNIT_CHECK(hipEventElapsedTime(&sweep, ev.e[0], ev.e[1]));
    UNIT_CHECK(hipEventElapsedTime(&walk, ev.e[1], ev.e[2]));
    st.sweep_ms += sweep;
    st.walk_ms += walk;
    for (uint64_t k = r.k0; k < r.k1; ++k) {
        const Plan& p = c.plans[k];
        if (p.none) continue;
        const uint32_t pen = res.penalty[k] = b.h_pen[(k - r.k0) * f.pen_words];
        res.n_ops[k] = f.ops ? b.h_nops[k - r.k0] : 0;
        if (f.end_k && pen != kNotFound) {
            res.end_k[k] = (int32_t)b.h_pen[2 * (k - r.k0) + 1];
            if (f.cells) std::copy_n(b.h_cells.begin() + 4 * (k - r.k0), 4, res.cells.begin() + 4 * k);
        }
        st.cells += cum_of(c.sc, (pen == kNotFound ? p.p_max : pen) + 1, p.n, p.m);
    }
}

// The fault word of the walks, the call's stats, the debug line
void finish(const Call& c, const FormInfo& f, const Buffers& b, const RangePlan& rp, pwa::WfaStats& st) {
    const pwa::WfaCtxView& v = c.v;
    const Pen& pen = c.sc.pen;
    st.workspace_bytes = rp.max_ws;
    if (f.ops) {
        uint32_t fault = 0;
        UNIT_CHECK(hipMemcpy(&fault, b.fault.p, 4, hipMemcpyDeviceToHost));
        if (fault) throw Fail{PWA_E_HIP, "pwa_align_wfa: a walk left its wavefronts (internal error)"};
    }
    *v.stats = st;
    if (v.debug)
        std::fprintf(stderr, "[pwa] wfa %s%s: %llu pairs, %zu ranges, x=%u o=%u e=%u ed=%u, %llu cells, workspace %llu B, sweep %.3f ms, walk %.3f ms\n", f.sg ? "sg " : "",
                     f.label, (unsigned long long)c.n_pairs, rp.ranges.size(), pen.x, pen.o, pen.e, pen.ed, (unsigned long long)st.cells,
                     (unsigned long long)st.workspace_bytes, st.sweep_ms, st.walk_ms);
}

// The sweep (and, for the alignment forms, the walk) of every pair
void run(Call& c, Form form, Results& res) {
    const pwa::WfaCtxView& v = c.v;
    const FormInfo& f = info(form);
    const uint64_t np = c.n_pairs;
    res.penalty.assign(np, kNotFound);
    res.n_ops.assign(np, 0);
    res.end_k.assign(f.sg ? np : 0, 0);
    res.cells.assign(f.sg ? 4 * np : 0, 0);
    pwa::WfaStats st;
    if (std::all_of(c.plans.begin(), c.plans.end(), [](const Plan& p) { return p.none; })) {   // nothing for the device to do
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
    RangePlan rp = plan_ranges(c, form, budget);
    res.ops.resize(rp.op_at[np]);
    const uint64_t blob_bytes = c.seq_off[c.n_seq];
    Buffers b;
    b.take(v, f, rp, blob_bytes);
    if (blob_bytes) UNIT_CHECK(hipMemcpyAsync(b.blob.p, c.blob, blob_bytes, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemsetAsync(b.blob.as<uint8_t>() + blob_bytes, 0, kPad, v.stream));
    if (f.ops) UNIT_CHECK(hipMemsetAsync(b.fault.p, 0, 4, v.stream));
    pwa::Events<3> ev;
    UNIT_CHECK(ev.create());
    for (const Range& r : rp.ranges) {
        if (r.pairs.empty()) continue;   // every pair of it was decided on the host
        b.again(v);
        launch_range(v, f, c.sc.pen, b, ev, r);
        collect_range(c, f, b, ev, r, rp, res, st);
    }
    finish(c, f, b, rp, st);
    res.op_at.swap(rp.op_at);
}

Call begin(pwa_ctx* ctx, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs) {
    return Call{pwa::wfa_ctx_view(ctx), Scoring{}, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, {}};
}

// pwa_wfa_plan and pwa_wfa_sg_plan: pen = the penalties of the form, then g
int plan_call(bool sg, int match, int mismatch, int gap_open, int gap_extend, const uint64_t* n, const uint64_t* m, const int32_t* min_score, uint64_t n_pairs,
              int32_t* pen, uint64_t* p_max, uint64_t* cells) {
    if (!pen || ((!n || !m) && n_pairs)) return PWA_E_INVALID;
    Scoring sc;
    if (const int rc = convert(sg, match, mismatch, gap_open, gap_extend, sc)) return rc;
    for (uint64_t k = 0; k < n_pairs; ++k)
        if (!in_range(sc, n[k], m[k])) return PWA_E_CAPACITY;
    *pen++ = (int32_t)sc.pen.x;
    *pen++ = (int32_t)sc.pen.o;
    *pen++ = (int32_t)sc.pen.e;
    if (sg) *pen++ = (int32_t)sc.pen.ed;
    *pen = (int32_t)sc.g;
    for (uint64_t k = 0; k < n_pairs; ++k) {
        const Plan p = plan_pair(sc, n[k], m[k], min_score ? min_score + k : nullptr);
        if (p_max) p_max[k] = p.none ? UINT64_MAX : p.p_max;
        if (cells) cells[k] = p.none ? 0 : p.cells;
    }
    return PWA_OK;
}

// What every result writer starts pair k with: its score, PWA_WFA_NONE for a pair not found, and the semi-global alignments' end and
// start cells (either array may be null; (0, 0) twice for a pair not found) -> found
bool put_score(const Call& c, const Results& r, uint64_t k, int32_t* score_out, uint64_t* end_cells = nullptr, uint64_t* start_cells = nullptr) {
    const bool hit = r.penalty[k] != kNotFound;
    score_out[k] = hit ? score_of(c.sc, c.plans[k], r.penalty[k]) : PWA_WFA_NONE;
    for (int x = 0; x < 2; ++x) {
        if (end_cells) end_cells[2 * k + x] = r.cells[4 * k + x];
        if (start_cells) start_cells[2 * k + x] = r.cells[4 * k + 2 + x];
    }
    return hit;
}

// pwa_scores_wfa and pwa_scores_wfa_sg (end_j_out: the semi-global form's end on the text)
int scores_call(Form form, const char* who, pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, const int32_t* min_score, int32_t* score_out,
                uint32_t* penalty_out, uint64_t* end_j_out) {
    if (!ctx || !seq_off || (!seq_bytes && n_seq && seq_off[n_seq]) || ((!pair_a || !pair_b || !score_out) && n_pairs)) return PWA_E_INVALID;
    Call c = begin(ctx, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs);
    if (const int rc = validate(c, form, match, mismatch, gap_open, gap_extend, min_score, who)) return rc;
    return pwa::guarded(c.v, [&] {
        Results r;
        run(c, form, r);
        for (uint64_t k = 0; k < n_pairs; ++k) {
            const bool hit = put_score(c, r, k, score_out);
            if (penalty_out) penalty_out[k] = r.penalty[k];
            if (end_j_out) end_j_out[k] = hit ? (uint64_t)((int64_t)c.plans[k].n + r.end_k[k]) : 0;
        }
    });
}

// pwa_align_wfa_batch, pwa_align_wfa_codes_batch and pwa_align_wfa_sg_batch: one body (end_cells, start_cells: the semi-global form's)
int align_ops(Form form, const char* who, pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
              const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops,
              const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells, uint64_t* start_cells, const int32_t* min_score) {
    if (!ctx || !seq_off || (!seq_bytes && n_seq && seq_off[n_seq]) || ((!pair_a || !pair_b || !score_out || !ops || !ops_off || !n_ops) && n_pairs))
        return PWA_E_INVALID;
    Call c = begin(ctx, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs);
    if (const int rc = validate(c, form, match, mismatch, gap_open, gap_extend, min_score, who)) return rc;
    return pwa::guarded(c.v, [&] {
        Results r;
        run(c, form, r);
        for (uint64_t k = 0; k < n_pairs; ++k) {
            n_ops[k] = put_score(c, r, k, score_out, end_cells, start_cells) ? r.n_ops[k] : 0;
            if (n_ops[k]) std::memcpy(ops + ops_off[k], r.ops.data() + r.op_at[k], n_ops[k]);
        }
    });
}

// pwa_align_wfa_batch_cigar, pwa_align_wfa_codes_batch_cigar and pwa_align_wfa_sg_batch_cigar
int align_strings(Form form, const char* who, pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                  const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                  uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells, uint64_t* start_cells,
                  uint64_t needed[2], const int32_t* min_score) {
    if (!ctx || !seq_off || !cigar_off || !mdz_off || (!seq_bytes && n_seq && seq_off[n_seq]) || (!cigar && cigar_cap) || (!mdz && mdz_cap) ||
        ((!pair_a || !pair_b || !score_out) && n_pairs))
        return PWA_E_INVALID;
    Call c = begin(ctx, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs);
    if (const int rc = validate(c, form, match, mismatch, gap_open, gap_extend, min_score, who)) return rc;
    return pwa::guarded(c.v, [&] {
        Results r;
        run(c, form, r);
        // the strings are formatted here, on the host, from the op lists (a pair not found has no strings at all, which
        // the device pass of cigar.hip.h cannot express); pattern and text at the start cell, which the semi-global form moves along the text
        uint64_t at_c = 0, at_m = 0;
        std::vector<char> cg, md;
        for (uint64_t k = 0; k < n_pairs; ++k) {
            cigar_off[k] = at_c;
            mdz_off[k] = at_m;
            if (!put_score(c, r, k, score_out, end_cells, start_cells)) continue;
            cg.resize(pwa_cigar_bound(r.n_ops[k]));
            md.resize(pwa_mdz_bound(r.n_ops[k]));
            const uint64_t start_j = info(form).cells ? r.cells[4 * k + 3] : 0;
            const pwa::FormatLen len = pwa::format_ops(seq_bytes + seq_off[pair_a[k]], seq_bytes + seq_off[pair_b[k]] + start_j, r.ops.data() + r.op_at[k], r.n_ops[k],
                                                       cg.data(), md.data());
            if (at_c + len.cigar <= cigar_cap && len.cigar) std::memcpy(cigar + at_c, cg.data(), len.cigar);
            if (at_m + len.mdz <= mdz_cap && len.mdz) std::memcpy(mdz + at_m, md.data(), len.mdz);
            at_c += len.cigar;
            at_m += len.mdz;
        }
        cigar_off[n_pairs] = at_c;
        mdz_off[n_pairs] = at_m;
        if (needed) {
            needed[0] = at_c;
            needed[1] = at_m;
        }
        if (at_c > cigar_cap || at_m > mdz_cap)
            throw Fail{PWA_E_CAPACITY, std::string(who) + ": the strings need " + std::to_string(at_c) + " + " + std::to_string(at_m) + " bytes"};
    });
}

}  // namespace

extern "C" {

int pwa_wfa_plan(int match, int mismatch, int gap_open, int gap_extend, const uint64_t* n, const uint64_t* m, const int32_t* min_score,
                 uint64_t n_pairs, int32_t pen[4], uint64_t* p_max, uint64_t* cells) {
    return plan_call(false, match, mismatch, gap_open, gap_extend, n, m, min_score, n_pairs, pen, p_max, cells);
}

int pwa_wfa_sg_plan(int match, int mismatch, int gap_open, int gap_extend, const uint64_t* n, const uint64_t* m, const int32_t* min_score,
                    uint64_t n_pairs, int32_t pen[5], uint64_t* p_max, uint64_t* cells) {
    return plan_call(true, match, mismatch, gap_open, gap_extend, n, m, min_score, n_pairs, pen, p_max, cells);
}

int pwa_scores_wfa(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                   const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, const int32_t* min_score, int32_t* score_out, uint32_t* penalty_out) {
    return scores_call(Form::Scores, "pwa_scores_wfa", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, min_score, score_out,
                       penalty_out, nullptr);
}

int pwa_scores_wfa_sg(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                      const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, const int32_t* min_score, int32_t* score_out, uint32_t* penalty_out,
                      uint64_t* end_j_out) {
    return scores_call(Form::SgScores, "pwa_scores_wfa_sg", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, min_score,
                       score_out, penalty_out, end_j_out);
}

int pwa_align_wfa_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                        const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off,
                        uint64_t* n_ops, const int32_t* min_score) {
    return align_ops(Form::Offsets, "pwa_align_wfa_batch", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                     score_out, ops, ops_off, n_ops, nullptr, nullptr, min_score);
}

int pwa_align_wfa_codes_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                              const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off,
                              uint64_t* n_ops, const int32_t* min_score) {
    return align_ops(Form::Codes, "pwa_align_wfa_codes_batch", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                     score_out, ops, ops_off, n_ops, nullptr, nullptr, min_score);
}

int pwa_align_wfa_sg_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                           const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off,
                           uint64_t* n_ops, uint64_t* end_cells, uint64_t* start_cells, const int32_t* min_score) {
    return align_ops(Form::SgCodes, "pwa_align_wfa_sg_batch", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                     score_out, ops, ops_off, n_ops, end_cells, start_cells, min_score);
}

int pwa_align_wfa_batch_cigar(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                              uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                              uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t needed[2],
                              const int32_t* min_score) {
    return align_strings(Form::Offsets, "pwa_align_wfa_batch_cigar", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b,
                         n_pairs, score_out, cigar, cigar_cap, cigar_off, mdz, mdz_cap, mdz_off, nullptr, nullptr, needed, min_score);
}

int pwa_align_wfa_codes_batch_cigar(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                                    uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                                    uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t needed[2],
                                    const int32_t* min_score) {
    return align_strings(Form::Codes, "pwa_align_wfa_codes_batch_cigar", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b,
                         n_pairs, score_out, cigar, cigar_cap, cigar_off, mdz, mdz_cap, mdz_off, nullptr, nullptr, needed, min_score);
}

int pwa_align_wfa_sg_batch_cigar(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                                 uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                                 uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells,
                                 uint64_t* start_cells, uint64_t needed[2], const int32_t* min_score) {
    return align_strings(Form::SgCodes, "pwa_align_wfa_sg_batch_cigar", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b,
                         n_pairs, score_out, cigar, cigar_cap, cigar_off, mdz, mdz_cap, mdz_off, end_cells, start_cells, needed, min_score);
}

int pwa_wfa_last_stats(const pwa_ctx* ctx, float* sweep_ms, float* walk_ms, uint64_t* cells, uint64_t* workspace_bytes) {
    if (!ctx) return PWA_E_INVALID;
    const pwa::WfaStats& st = pwa::wfa_stats_of(ctx);
    if (sweep_ms) *sweep_ms = st.sweep_ms;
    if (walk_ms) *walk_ms = st.walk_ms;
    if (cells) *cells = st.cells;
    if (workspace_bytes) *workspace_bytes = st.workspace_bytes;
    return PWA_OK;
}

}  // extern "C"

// pwa_selftest_host: plan_ranges under every form on random pair lists with made-up budgets, against what any plan must satisfy and
// what the kernels of wfa.hip.h will address (their own host-callable formulas), not against a second copy of the planner.  0, or the
// number of the failing check (they continue selftest_align_plan's).
int pwa::selftest_wfa_plan(uint64_t x, int check) {
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    static const int scorings[3][4] = {{1, -4, -6, -1}, {1, -40, -6, -1}, {1, -80, -6, -1}};   // rings of 16, 83, 163 (semi-global: 9, 42, 82) wavefronts
    for (int round = 0; round < 45; ++round) {   // every form under every scoring without bounds, with loose ones, with tight ones
        const Form form = (Form)(round % 5);
        const FormInfo& f = info(form);
        const int* const s = scorings[round / 5 % 3];
        const int bounds = round / 15;
        const uint32_t n_seq = 120;
        const uint64_t np = 200 + rnd() % 300;
        std::vector<uint64_t> off(n_seq + 1, 0);
        for (uint32_t q = 0; q < n_seq; ++q) {   // a quarter empty or tiny, a few of some thousand symbols
            const uint64_t r = rnd() % 16;
            off[q + 1] = off[q] + (r == 0 ? 0 : r < 4 ? 1 + rnd() % 4 : r < 13 ? 5 + rnd() % 300 : 300 + rnd() % 3000);
        }
        std::vector<uint32_t> pa(np), pb(np);
        std::vector<int32_t> min_score(np);
        uint64_t tight = 0;   // pairs still to come of a run that the host rules out
        for (uint64_t k = 0; k < np; ++k) {
            pa[k] = (uint32_t)(rnd() % n_seq);   // either side may be the longer, and both may be empty
            pb[k] = (uint32_t)(rnd() % n_seq);
            const int64_t n = (int64_t)(off[pa[k] + 1] - off[pa[k]]), m = (int64_t)(off[pb[k] + 1] - off[pb[k]]);
            const int64_t best = f.sg ? s[0] * n : s[0] * (n + m) / 2;   // no alignment scores above it
            if (bounds == 2 && !tight && rnd() % 6 == 0) tight = 1 + rnd() % 5;
            min_score[k] = (int32_t)(tight ? best + 1 : bounds == 2 ? best - (int64_t)(rnd() % 40) : best - 40 - (int64_t)(rnd() % 20000));
            tight -= tight ? 1 : 0;
        }
        Call c;
        std::string err;
        c.v.err = &err;
        c.seq_off = off.data();
        c.n_seq = n_seq;
        c.pair_a = pa.data();
        c.pair_b = pb.data();
        c.n_pairs = np;
        if (validate(c, form, s[0], s[1], s[2], s[3], bounds ? min_score.data() : nullptr, "selftest") != PWA_OK || c.sc.sg != f.sg) return check + 1;
        uint64_t ruled_out = 0;
        for (const Plan& p : c.plans) ruled_out += p.none;
        if (bounds == 2 && ruled_out < 4) return check + 2;   // (the lists are made to have them)
        // budgets: everything in one range, which gives the list's weight; a few ranges; a handful of pairs per range; less than any pair
        uint64_t weight = 0;
        for (int b = 0; b < 4; ++b) {
            const uint64_t budget = b == 0 ? 1ull << 62 : b == 1 ? weight / (3 + rnd() % 6) : b == 2 ? weight / np * (2 + rnd() % 8) : rnd() % 64;
            const RangePlan rp = plan_ranges(c, form, budget);
            if (rp.ws_at.size() != np || rp.op_at.size() != np + 1 || rp.ranges.empty()) return check + 1;
            if (b == 0) {
                if (rp.ranges.size() != 1) return check + 1;
                weight = rp.ranges[0].ws_bytes + rp.ranges[0].op_bytes;
            }
            // bytes of pair k's workspace slice and of its op slice, as the plan states them: up to the next pair's, or the range's end
            auto ws_of = [&](const Range& r, uint64_t k) { return (k + 1 < r.k1 ? 4 * rp.ws_at[k + 1] : r.ws_bytes) - 4 * rp.ws_at[k]; };
            auto op_of = [&](uint64_t k) { return rp.op_at[k + 1] - rp.op_at[k]; };
            uint64_t max_ws = 0, max_ops = 0, max_n = 0;
            for (size_t i = 0; i < rp.ranges.size(); ++i) {
                const Range& r = rp.ranges[i];
                const uint64_t cnt = r.k1 - r.k0;
                // 1: the ranges partition the list in order; each fits the budget or is one pair; none could have taken the next pair
                if (r.k0 != (i ? rp.ranges[i - 1].k1 : 0) || r.k1 <= r.k0 || r.k1 > np || (i + 1 == rp.ranges.size() && r.k1 != np)) return check + 1;
                if (cnt > 1 && r.ws_bytes + r.op_bytes > budget) return check + 1;
                if (r.k1 < np && r.ws_bytes + r.op_bytes + ws_of(rp.ranges[i + 1], r.k1) + op_of(r.k1) <= budget) return check + 1;
                // 2: the launch list: every pair not ruled out once, no other; by falling cells, ties in pair order; the records
                std::vector<uint32_t> times(cnt, 0);
                for (size_t q = 0; q < r.pairs.size(); ++q) {
                    const Pair& P = r.pairs[q];
                    if (P.out >= cnt) return check + 2;
                    const uint64_t k = r.k0 + P.out;
                    const Plan& p = c.plans[k];
                    ++times[P.out];
                    if (p.none || P.pat != off[pa[k]] || P.txt != off[pb[k]] || P.n != p.n || P.m != p.m || P.p_max != p.p_max || P.ws != rp.ws_at[k] ||
                        P.ops != rp.op_at[k] - rp.op_at[r.k0])
                        return check + 2;
                    if (q) {
                        const uint64_t before = r.k0 + r.pairs[q - 1].out;
                        if (c.plans[before].cells < p.cells || (c.plans[before].cells == p.cells && before >= k)) return check + 2;
                    }
                }
                for (uint64_t k = r.k0; k < r.k1; ++k)
                    if (times[k - r.k0] != (c.plans[k].none ? 0u : 1u)) return check + 2;
                // 3: the workspace slices are disjoint, end inside the range's workspace and hold what the kernels address
                std::vector<std::pair<uint64_t, uint64_t>> slices;   // [first, second) in bytes
                for (const Pair& P : r.pairs) {
                    const uint64_t ring = 4 * (f.sg ? ring_words<true>(P.p_max, P.n, P.m, c.sc.pen) : ring_words<false>(P.p_max, P.n, P.m, c.sc.pen));
                    const uint64_t cells = f.sg ? cum<true>(P.p_max + 1, P.n, P.m, c.sc.pen) : cum<false>(P.p_max + 1, P.n, P.m, c.sc.pen);
                    const uint64_t need = f.keep == Keep::All ? 12 * cells : f.keep == Keep::RingCodes ? ring + cells : ring;
                    if (need == 0 || ws_of(r, r.k0 + P.out) < need) return check + 3;
                    slices.emplace_back(4 * P.ws, 4 * P.ws + need);
                }
                std::sort(slices.begin(), slices.end());
                for (size_t q = 0; q < slices.size(); ++q)
                    if (slices[q].second > r.ws_bytes || (q && slices[q].first < slices[q - 1].second)) return check + 3;
                // 4: the op slices: n + m bytes each, one behind the other in pair order, inside the range's op bytes; none for a score form
                uint64_t ops = 0;
                for (uint64_t k = r.k0; k < r.k1; ++k) {
                    if (op_of(k) != (f.ops ? (uint64_t)c.plans[k].n + c.plans[k].m : 0) || rp.op_at[k] - rp.op_at[r.k0] != ops) return check + 4;
                    ops += op_of(k);
                }
                if (r.op_bytes != ops || (!f.ops && rp.op_at[np])) return check + 4;
                max_ws = std::max(max_ws, r.ws_bytes);
                max_ops = std::max(max_ops, r.op_bytes);
                max_n = std::max(max_n, cnt);
            }
            // 5: the capacities cover every range, and the workspace's is the largest range's (what the stats report)
            if (rp.max_ws != max_ws || rp.max_ops < max_ops || rp.max_n < max_n) return check + 5;
            if (b && rp.ranges.size() < 2) return check + 1;   // (the budgets are made to cut)
        }
    }
    return 0;
}
