// wfa_kernels.hip -- the wavefront-alignment entries of include/pwalign.h (pwa_wfa_plan, pwa_scores_wfa, pwa_align_wfa_batch(_cigar),
// pwa_align_wfa_codes_batch(_cigar), pwa_wfa_last_stats, and the semi-global pwa_wfa_sg_plan, pwa_scores_wfa_sg, pwa_align_wfa_sg_batch(_cigar)):
// validation, the conversion to penalties, the per-pair plan and bound, ranges of consecutive pairs under the PWA_RANGE_BYTES budget, the sweep
// and the walk of each range, the CIGAR / MD:Z strings.  Kernels: wfa.hip.h.
#include "../../include/pwalign.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
    sc.match = match;
    sc.mismatch = mismatch;
    sc.go = go;
    sc.ge = ge;
    sc.pen = Pen{(uint32_t)(x0 / g), (uint32_t)(o0 / g), (uint32_t)(e0 / g), (uint32_t)(e0 / g)};
    sc.g = (uint32_t)g;
    return PWA_OK;
}

// The semi-global form's: counted per pattern symbol, because the text length an alignment consumes is not fixed
int convert_sg(int match, int mismatch, int go, int ge, Scoring& sc) {
    const int64_t x0 = (int64_t)match - mismatch, o0 = -(int64_t)go, i0 = -(int64_t)ge, d0 = (int64_t)match - ge;
    if (go > 0 || ge >= 0 || x0 <= 0 || d0 <= 0) return PWA_E_INVALID;
    const int64_t g = gcd64(gcd64(x0, o0), gcd64(i0, d0));
    if (x0 / g > 0x3fffffff || o0 / g > 0x3fffffff || i0 / g > 0x3fffffff || d0 / g > 0x3fffffff) return PWA_E_CAPACITY;   // (as above)
    sc.match = match;
    sc.mismatch = mismatch;
    sc.go = go;
    sc.ge = ge;
    sc.sg = true;
    sc.pen = Pen{(uint32_t)(x0 / g), (uint32_t)(o0 / g), (uint32_t)(i0 / g), (uint32_t)(d0 / g)};
    sc.g = (uint32_t)g;
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

struct Range {
    uint64_t k0 = 0, k1 = 0;
    uint64_t ws_bytes = 0, op_bytes = 0;
};

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

// Scoring, required pointers (by the caller), indices and the range rule, in pair order; fills c.plans
int validate(Call& c, bool sg, int match, int mismatch, int go, int ge, const int32_t* min_score, const char* who) {
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

// What a call keeps of the wavefronts: a ring and nothing else (scores), every wavefront (alignments from the stored offsets), or a
// ring and one code byte per planned cell (alignments from the codes)
enum class Form { Scores, Offsets, Codes };

// What run() brings back: penalty[k] = P or kNotFound; op lists packed pair after pair into `ops` (pair k at op_at[k], n + m bytes of
// room, n_ops[k] of them written).  The semi-global form: end_k[k] = the end diagonal, cells[4 k ..] = end (i, j), start (i, j) of an
// alignment call; zeros for a pair not found
struct Results {
    std::vector<uint32_t> penalty, n_ops, cells;
    std::vector<int32_t> end_k;
    std::vector<uint8_t> ops;
    std::vector<uint64_t> op_at;
};

// The sweep (and, for the alignment forms, the walk) of every pair
void run(Call& c, Form form, Results& res) {
    const pwa::WfaCtxView& v = c.v;
    const uint64_t np = c.n_pairs;
    const bool sg = c.sc.sg;
    std::vector<uint32_t>&penalty = res.penalty, &n_ops = res.n_ops;
    std::vector<uint8_t>& ops = res.ops;
    std::vector<uint64_t>& op_at = res.op_at;
    penalty.assign(np, kNotFound);
    n_ops.assign(np, 0);
    op_at.assign(np + 1, 0);
    res.end_k.assign(sg ? np : 0, 0);
    res.cells.assign(sg ? 4 * np : 0, 0);
    pwa::WfaStats st;
    const bool want_ops = form != Form::Scores;
    if (want_ops) {
        for (uint64_t k = 0; k < np; ++k) op_at[k + 1] = op_at[k] + c.plans[k].n + c.plans[k].m;
        ops.resize(op_at[np]);
    }
    const Pen pen = c.sc.pen;
    auto ws_bytes = [&](const Plan& p) -> uint64_t {
        if (p.none) return 0;
        if (form == Form::Offsets) return 12 * p.cells;
        const uint64_t ring = ring_bytes_of(c.sc, p.p_max, p.n, p.m);
        return form == Form::Codes ? ring + ((p.cells + 3) & ~3ull) : ring;   // the code plane behind the ring, up to the next int32
    };
    bool any = false;
    for (const Plan& p : c.plans) any = any || !p.none;
    if (!any) {
        *v.stats = st;
        return;
    }
    (void)hipSetDevice(v.device);
    uint64_t budget = v.range_bytes;
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        UNIT_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<uint64_t>((uint64_t)(free_b * 0.6), 48ull << 30);
    }
    // ranges of consecutive pairs, by workspace and op bytes together; one pair alone may exceed the budget
    auto op_bytes = [&](const Plan& p) -> uint64_t { return want_ops ? p.n + p.m : 0; };
    std::vector<Range> ranges;
    uint64_t max_ws = 0, max_ops = 0, max_n = 0;
    for (const pwa::Run& cut : pwa::cut_runs(np, budget, [&](uint64_t k) { return ws_bytes(c.plans[k]) + op_bytes(c.plans[k]); })) {
        Range r{cut.k0, cut.k1};
        for (uint64_t k = r.k0; k < r.k1; ++k) {
            r.ws_bytes += ws_bytes(c.plans[k]);
            r.op_bytes += op_bytes(c.plans[k]);
        }
        ranges.push_back(r);
        max_ws = std::max(max_ws, r.ws_bytes);
        max_ops = std::max(max_ops, r.op_bytes);
        max_n = std::max(max_n, r.k1 - r.k0);
    }
    const uint64_t blob_bytes = c.seq_off[c.n_seq];
    const uint64_t pen_words = sg ? 2 : 1;   // per pair: the penalty, and the semi-global form's end diagonal
    Dev d_blob, d_ws, d_pairs, d_pen, d_nops, d_ops, d_fault, d_cells;
    UNIT_CHECK(d_blob.alloc(v.poison, blob_bytes + kPad));
    UNIT_CHECK(d_ws.alloc(v.poison, max_ws));
    UNIT_CHECK(d_pairs.alloc(v.poison, max_n * sizeof(Pair)));
    UNIT_CHECK(d_pen.alloc(v.poison, max_n * 4 * pen_words));
    if (want_ops && sg) UNIT_CHECK(d_cells.alloc(v.poison, max_n * 16));
    if (want_ops) {
        UNIT_CHECK(d_nops.alloc(v.poison, max_n * 4));
        UNIT_CHECK(d_ops.alloc(v.poison, max_ops));
        UNIT_CHECK(d_fault.alloc(v.poison, 4));
    }
    if (blob_bytes) UNIT_CHECK(hipMemcpyAsync(d_blob.p, c.blob, blob_bytes, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemsetAsync(d_blob.as<uint8_t>() + blob_bytes, 0, kPad, v.stream));
    if (want_ops) UNIT_CHECK(hipMemsetAsync(d_fault.p, 0, 4, v.stream));
    pwa::Events<3> ev;
    UNIT_CHECK(ev.create());
    std::vector<Pair> pairs;
    std::vector<uint32_t> h_pen, h_nops, h_cells;
    std::vector<uint64_t> order;
    bool first = true;
    for (const Range& r : ranges) {
        const uint64_t cnt = r.k1 - r.k0;
        // launch order: longest plan first; pairs the host decided are left out
        order.clear();
        for (uint64_t k = r.k0; k < r.k1; ++k)
            if (!c.plans[k].none) order.push_back(k);
        if (order.empty()) continue;
        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return c.plans[a].cells > c.plans[b].cells; });
        std::vector<uint64_t> ws_at(cnt + 1, 0);
        for (uint64_t k = r.k0; k < r.k1; ++k) ws_at[k - r.k0 + 1] = ws_at[k - r.k0] + ws_bytes(c.plans[k]) / 4;
        pairs.clear();
        for (uint64_t k : order) {
            const Plan& p = c.plans[k];
            pairs.push_back(Pair{c.seq_off[c.pair_a[k]], c.seq_off[c.pair_b[k]], ws_at[k - r.k0], want_ops ? op_at[k] - op_at[r.k0] : 0, p.n, p.m, p.p_max,
                                 (uint32_t)(k - r.k0)});
        }
        if (!first) {   // the buffers of the range before, handed out again
            UNIT_CHECK(hipStreamSynchronize(v.stream));
            UNIT_CHECK(d_ws.again(v.poison));
            UNIT_CHECK(d_pairs.again(v.poison));
            UNIT_CHECK(d_pen.again(v.poison));
            if (want_ops) {
                UNIT_CHECK(d_nops.again(v.poison));
                UNIT_CHECK(d_ops.again(v.poison));
                if (sg) UNIT_CHECK(d_cells.again(v.poison));
            }
        }
        first = false;
        const uint32_t nl = (uint32_t)pairs.size(), blocks = (nl + kWaves - 1) / kWaves;
        UNIT_CHECK(hipMemcpyAsync(d_pairs.p, pairs.data(), nl * sizeof(Pair), hipMemcpyHostToDevice, v.stream));
        const SweepParams sp{d_blob.as<uint8_t>(), d_pairs.as<Pair>(), nl, pen, d_ws.as<int32_t>(), d_pen.as<uint32_t>()};
        UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
        if (form == Form::Offsets)
            hipLaunchKernelGGL(wfa_sweep_kernel<false>, dim3(blocks), dim3(64 * kWaves), 0, v.stream, sp);
        else if (form == Form::Codes)
            hipLaunchKernelGGL(sg ? wfa_sg_codes_sweep_kernel : wfa_codes_sweep_kernel, dim3(blocks), dim3(64 * kWaves), 0, v.stream, sp);
        else
            hipLaunchKernelGGL(sg ? wfa_sg_sweep_kernel : wfa_sweep_kernel<true>, dim3(blocks), dim3(64 * kWaves), 0, v.stream, sp);
        UNIT_CHECK(hipGetLastError());
        UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
        if (form == Form::Codes) {
            const CodesWalkParams wp{d_blob.as<uint8_t>(), d_pairs.as<Pair>(), nl, pen, d_ws.as<int32_t>(), d_pen.as<uint32_t>(), d_ops.as<uint8_t>(),
                                     d_nops.as<uint32_t>(), d_fault.as<uint32_t>(), d_cells.as<uint32_t>()};
            hipLaunchKernelGGL(sg ? wfa_sg_codes_walk_kernel : wfa_codes_walk_kernel, dim3(blocks), dim3(64 * kWaves), 0, v.stream, wp);
            UNIT_CHECK(hipGetLastError());
        } else if (want_ops) {
            const WalkParams wp{d_pairs.as<Pair>(), nl, pen, d_ws.as<int32_t>(), d_pen.as<uint32_t>(), d_ops.as<uint8_t>(), d_nops.as<uint32_t>(), d_fault.as<uint32_t>()};
            hipLaunchKernelGGL(wfa_walk_kernel, dim3(blocks), dim3(64 * kWaves), 0, v.stream, wp);
            UNIT_CHECK(hipGetLastError());
        }
        UNIT_CHECK(hipEventRecord(ev.e[2], v.stream));
        h_pen.assign(cnt * pen_words, kNotFound);
        h_nops.assign(cnt, 0);
        h_cells.assign(sg ? 4 * cnt : 0, 0);
        UNIT_CHECK(hipMemcpyAsync(h_pen.data(), d_pen.p, cnt * 4 * pen_words, hipMemcpyDeviceToHost, v.stream));
        if (want_ops && sg) UNIT_CHECK(hipMemcpyAsync(h_cells.data(), d_cells.p, cnt * 16, hipMemcpyDeviceToHost, v.stream));
        if (want_ops) {
            UNIT_CHECK(hipMemcpyAsync(h_nops.data(), d_nops.p, cnt * 4, hipMemcpyDeviceToHost, v.stream));
            if (r.op_bytes) UNIT_CHECK(hipMemcpyAsync(ops.data() + op_at[r.k0], d_ops.p, r.op_bytes, hipMemcpyDeviceToHost, v.stream));
        }
        UNIT_CHECK(hipStreamSynchronize(v.stream));
        float a = 0.f, b = 0.f;
        UNIT_CHECK(hipEventElapsedTime(&a, ev.e[0], ev.e[1]));
        UNIT_CHECK(hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        st.sweep_ms += a;
        st.walk_ms += b;
        for (uint64_t k : order) {   // (a pair left out of the launch keeps kNotFound and no ops; its slots were never written)
            penalty[k] = h_pen[(k - r.k0) * pen_words];
            n_ops[k] = want_ops ? h_nops[k - r.k0] : 0;
            const Plan& p = c.plans[k];
            if (sg && penalty[k] != kNotFound) {
                res.end_k[k] = (int32_t)h_pen[2 * (k - r.k0) + 1];
                if (want_ops) std::copy_n(h_cells.begin() + 4 * (k - r.k0), 4, res.cells.begin() + 4 * k);
            }
            st.cells += cum_of(c.sc, (penalty[k] == kNotFound ? p.p_max : penalty[k]) + 1, p.n, p.m);
        }
    }
    st.workspace_bytes = max_ws;
    if (want_ops) {
        uint32_t fault = 0;
        UNIT_CHECK(hipMemcpy(&fault, d_fault.p, 4, hipMemcpyDeviceToHost));
        if (fault) throw Fail{PWA_E_HIP, "pwa_align_wfa: a walk left its wavefronts (internal error)"};
    }
    *v.stats = st;
    if (v.debug)
        std::fprintf(stderr, "[pwa] wfa %s%s: %llu pairs, %zu ranges, x=%u o=%u e=%u ed=%u, %llu cells, workspace %llu B, sweep %.3f ms, walk %.3f ms\n", sg ? "sg " : "",
                     form == Form::Codes ? "align (codes)" : want_ops ? "align" : "scores", (unsigned long long)np, ranges.size(), pen.x, pen.o, pen.e, pen.ed, (unsigned long long)st.cells,
                     (unsigned long long)st.workspace_bytes, st.sweep_ms, st.walk_ms);
}

Call begin(pwa_ctx* ctx, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs) {
    Call c;
    c.v = pwa::wfa_ctx_view(ctx);
    c.blob = seq_bytes;
    c.seq_off = seq_off;
    c.n_seq = n_seq;
    c.pair_a = pair_a;
    c.pair_b = pair_b;
    c.n_pairs = n_pairs;
    return c;
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

// pwa_scores_wfa and pwa_scores_wfa_sg (end_j_out: the semi-global form's end on the text)
int scores_call(bool sg, const char* who, pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, const int32_t* min_score, int32_t* score_out,
                uint32_t* penalty_out, uint64_t* end_j_out) {
    if (!ctx || !seq_off || (!seq_bytes && n_seq && seq_off[n_seq]) || ((!pair_a || !pair_b || !score_out) && n_pairs)) return PWA_E_INVALID;
    Call c = begin(ctx, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs);
    if (const int rc = validate(c, sg, match, mismatch, gap_open, gap_extend, min_score, who)) return rc;
    return pwa::guarded(c.v, [&] {
        Results r;
        run(c, Form::Scores, r);
        for (uint64_t k = 0; k < n_pairs; ++k) {
            const bool hit = r.penalty[k] != kNotFound;
            score_out[k] = hit ? score_of(c.sc, c.plans[k], r.penalty[k]) : PWA_WFA_NONE;
            if (penalty_out) penalty_out[k] = r.penalty[k];
            if (end_j_out) end_j_out[k] = hit ? (uint64_t)((int64_t)c.plans[k].n + r.end_k[k]) : 0;
        }
    });
}

// The semi-global form's end and start cells of pair k (either array may be null); (0, 0) twice for a pair not found
void put_cells(const Results& r, uint64_t k, uint64_t* end_cells, uint64_t* start_cells) {
    for (int x = 0; x < 2; ++x) {
        if (end_cells) end_cells[2 * k + x] = r.cells[4 * k + x];
        if (start_cells) start_cells[2 * k + x] = r.cells[4 * k + 2 + x];
    }
}

// pwa_align_wfa_batch, pwa_align_wfa_codes_batch and pwa_align_wfa_sg_batch: one body, the forms of the workspace and of the sweep
int align_ops(Form form, bool sg, const char* who, pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
              const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops,
              const uint64_t* ops_off, uint64_t* n_ops, uint64_t* end_cells, uint64_t* start_cells, const int32_t* min_score) {
    if (!ctx || !seq_off || (!seq_bytes && n_seq && seq_off[n_seq]) || ((!pair_a || !pair_b || !score_out || !ops || !ops_off || !n_ops) && n_pairs))
        return PWA_E_INVALID;
    Call c = begin(ctx, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs);
    if (const int rc = validate(c, sg, match, mismatch, gap_open, gap_extend, min_score, who)) return rc;
    return pwa::guarded(c.v, [&] {
        Results r;
        run(c, form, r);
        for (uint64_t k = 0; k < n_pairs; ++k) {
            const bool hit = r.penalty[k] != kNotFound;
            score_out[k] = hit ? score_of(c.sc, c.plans[k], r.penalty[k]) : PWA_WFA_NONE;
            n_ops[k] = hit ? r.n_ops[k] : 0;
            if (n_ops[k]) std::memcpy(ops + ops_off[k], r.ops.data() + r.op_at[k], n_ops[k]);
            if (sg) put_cells(r, k, end_cells, start_cells);
        }
    });
}

// pwa_align_wfa_batch_cigar, pwa_align_wfa_codes_batch_cigar and pwa_align_wfa_sg_batch_cigar
int align_strings(Form form, bool sg, const char* who, pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes,
                  const uint64_t* seq_off, uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                  uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells, uint64_t* start_cells,
                  uint64_t needed[2], const int32_t* min_score) {
    if (!ctx || !seq_off || !cigar_off || !mdz_off || (!seq_bytes && n_seq && seq_off[n_seq]) || (!cigar && cigar_cap) || (!mdz && mdz_cap) ||
        ((!pair_a || !pair_b || !score_out) && n_pairs))
        return PWA_E_INVALID;
    Call c = begin(ctx, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs);
    if (const int rc = validate(c, sg, match, mismatch, gap_open, gap_extend, min_score, who)) return rc;
    return pwa::guarded(c.v, [&] {
        Results r;
        run(c, form, r);
        // the strings are formatted here, on the host, from the op lists (a pair not found has no strings at all, which
        // the device pass of cigar.hip.h cannot express); pattern and text at the start cell, which the semi-global form moves along the text
        uint64_t at_c = 0, at_m = 0;
        std::vector<char> cg, md;
        for (uint64_t k = 0; k < n_pairs; ++k) {
            const bool hit = r.penalty[k] != kNotFound;
            score_out[k] = hit ? score_of(c.sc, c.plans[k], r.penalty[k]) : PWA_WFA_NONE;
            cigar_off[k] = at_c;
            mdz_off[k] = at_m;
            if (sg) put_cells(r, k, end_cells, start_cells);
            if (!hit) continue;
            cg.resize(pwa_cigar_bound(r.n_ops[k]));
            md.resize(pwa_mdz_bound(r.n_ops[k]));
            const uint64_t start_j = sg ? r.cells[4 * k + 3] : 0;
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
    return scores_call(false, "pwa_scores_wfa", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, min_score, score_out,
                       penalty_out, nullptr);
}

int pwa_scores_wfa_sg(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                      const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, const int32_t* min_score, int32_t* score_out, uint32_t* penalty_out,
                      uint64_t* end_j_out) {
    return scores_call(true, "pwa_scores_wfa_sg", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs, min_score,
                       score_out, penalty_out, end_j_out);
}

int pwa_align_wfa_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                        const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off,
                        uint64_t* n_ops, const int32_t* min_score) {
    return align_ops(Form::Offsets, false, "pwa_align_wfa_batch", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                     score_out, ops, ops_off, n_ops, nullptr, nullptr, min_score);
}

int pwa_align_wfa_codes_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                              const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off,
                              uint64_t* n_ops, const int32_t* min_score) {
    return align_ops(Form::Codes, false, "pwa_align_wfa_codes_batch", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                     score_out, ops, ops_off, n_ops, nullptr, nullptr, min_score);
}

int pwa_align_wfa_sg_batch(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                           const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, uint8_t* ops, const uint64_t* ops_off,
                           uint64_t* n_ops, uint64_t* end_cells, uint64_t* start_cells, const int32_t* min_score) {
    return align_ops(Form::Codes, true, "pwa_align_wfa_sg_batch", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b, n_pairs,
                     score_out, ops, ops_off, n_ops, end_cells, start_cells, min_score);
}

int pwa_align_wfa_batch_cigar(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                              uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                              uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t needed[2],
                              const int32_t* min_score) {
    return align_strings(Form::Offsets, false, "pwa_align_wfa_batch_cigar", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b,
                         n_pairs, score_out, cigar, cigar_cap, cigar_off, mdz, mdz_cap, mdz_off, nullptr, nullptr, needed, min_score);
}

int pwa_align_wfa_codes_batch_cigar(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                                    uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                                    uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t needed[2],
                                    const int32_t* min_score) {
    return align_strings(Form::Codes, false, "pwa_align_wfa_codes_batch_cigar", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b,
                         n_pairs, score_out, cigar, cigar_cap, cigar_off, mdz, mdz_cap, mdz_off, nullptr, nullptr, needed, min_score);
}

int pwa_align_wfa_sg_batch_cigar(pwa_ctx* ctx, int match, int mismatch, int gap_open, int gap_extend, const uint8_t* seq_bytes, const uint64_t* seq_off,
                                 uint32_t n_seq, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, int32_t* score_out, char* cigar,
                                 uint64_t cigar_cap, uint64_t* cigar_off, char* mdz, uint64_t mdz_cap, uint64_t* mdz_off, uint64_t* end_cells,
                                 uint64_t* start_cells, uint64_t needed[2], const int32_t* min_score) {
    return align_strings(Form::Codes, true, "pwa_align_wfa_sg_batch_cigar", ctx, match, mismatch, gap_open, gap_extend, seq_bytes, seq_off, n_seq, pair_a, pair_b,
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

