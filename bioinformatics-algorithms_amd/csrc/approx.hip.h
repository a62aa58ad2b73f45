// approx.hip.h -- kernels of the k-edit approximate search (pwa_approx_*, approx_kernels.hip): Sellers' DP in Myers' bit-parallel
// columns, one lane per task.  DESIGN.md §3.18.
//
// A lane carries a column of 64 * W rows (W = ceil(m / 64) 64-bit words; a wave holds tasks of one W) as vertical deltas Pv (+1) and
// Mv (-1), held as 2 W 32-bit registers each.  The pattern sits at the TOP of that column: its row i is bit pad + i, pad = 64 W - m,
// and the pad rows below it are rows that every symbol matches and that start at 0, so they stay 0 for good and act as row 0 of the
// DP (D[0][j] = 0).  Row m is then bit 31 of the last register for every lane, whatever its m: the score follows one fixed bit.
// One text symbol: Eq = the lane's mask of that symbol (LDS, [code][word][lane]: a wave's 8-byte reads are consecutive, and a lane
// reads only what it wrote itself, so the kernel has no barrier), then over the registers in ascending order
//     Xh = (((Eq & Pv) + Pv + carry) ^ Pv) | Eq      Ph = Mv | ~(Xh | Pv)      Mh = Pv & Xh
//     Ph' = Ph << 1 | (Ph of the register below) >> 31, Mh' likewise (v_alignbit_b32)
//     Pv = Mh' | ~(Eq | Mv | Ph')                    Mv = Ph' & (Eq | Mv)
// with the add's carry (v_addc_co_u32) and the two shifted-out bits passing from register to register; the input at bit 0 is 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pwa {
namespace approx {

constexpr int kMaxWords = 8;        // 64-bit words per column: patterns of at most 512
constexpr int kMaxSym = 32;         // distinct pattern bytes per call; code kMaxSym at most stands for every other byte
constexpr uint32_t kNoTask = 0xffffffffu;
constexpr uint64_t kNoBest = ~0ull;

struct CodeTable {
    uint8_t t[256];
};
struct Pat {        // one pattern on the device
    uint32_t off;   // of its bytes in the blob
    uint32_t m;
    uint32_t k;     // min(max_dist, m)
    uint32_t peq;   // of its masks in the mask array, in 64-bit words: [code 0 .. sigma][word 0 .. W)
    uint32_t W;
};
struct Task {   // text columns [lo, hi) to report, scanned from the fresh column at scan_lo (a multiple of 16)
    uint32_t pat, scan_lo, lo, hi;
};

// Masks of every pattern: thread (pattern, code, word).  Code sigma (no pattern byte) keeps the pad bits only.
__global__ __launch_bounds__(256) void approx_masks_kernel(const uint8_t* __restrict__ blob, const Pat* __restrict__ pats, uint32_t n_pat, uint32_t rows,
                                                           const CodeTable tab, uint64_t* __restrict__ peq) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t q = x / (rows * kMaxWords);
    const uint32_t r = (uint32_t)(x % (rows * kMaxWords)), code = r / kMaxWords, w = r % kMaxWords;
    if (q >= n_pat) return;
    const Pat p = pats[q];
    if (w >= p.W) return;
    const uint32_t pad = 64 * p.W - p.m;
    uint64_t bits = 0;
    for (uint32_t b = 0; b < 64; ++b) {
        const uint32_t pos = 64 * w + b;
        if (pos < pad || tab.t[blob[p.off + (pos - pad)]] == code) bits |= 1ull << b;
    }
    peq[p.peq + code * p.W + w] = bits;
}

// One wave per workgroup, lane l of workgroup b runs task lane_task[64 b + l] (kNoTask: none).  LDS: rows * W * 64 masks of 8 bytes.
// FILL = false: task_cnt[task] = its hits, pat_cnt[pattern] += them, pat_best[pattern] = min(dist << 32 | end).
// FILL = true: only tasks t0 <= task < t1; the keys end << 32 | dist of a task go to out[task_off[task - t0] ...), below out_cap.
template <int W, bool FILL>
__global__ __launch_bounds__(64) void approx_scan_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ peq, const Pat* __restrict__ pats,
                                                         const Task* __restrict__ tasks, const uint32_t* __restrict__ lane_task, uint32_t rows,
                                                         uint32_t* __restrict__ task_cnt, uint32_t* __restrict__ pat_cnt,
                                                         unsigned long long* __restrict__ pat_best, uint32_t t0, uint32_t t1,
                                                         const uint32_t* __restrict__ task_off, uint64_t* __restrict__ out, uint32_t out_cap) {
    extern __shared__ uint2 approx_lds[];
    constexpr int N = 2 * W;
    const uint32_t lane = threadIdx.x;
    const uint32_t tid = lane_task[blockIdx.x * 64 + lane];
    if (tid == kNoTask) return;
    if (FILL && (tid < t0 || tid >= t1)) return;
    const Task tk = tasks[tid];
    const Pat p = pats[tk.pat];
    {
        const uint2* src = reinterpret_cast<const uint2*>(peq + p.peq);
        for (uint32_t i = 0; i < rows * W; ++i) approx_lds[i * 64 + lane] = src[i];
    }
    uint32_t pv[N], mv[N];
    {
        const uint32_t pad = 64 * W - p.m;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const uint32_t b = 32 * i;   // ones from bit pad up
            pv[i] = pad <= b ? ~0u : pad >= b + 32 ? 0u : ~0u << (pad - b);
            mv[i] = 0;
        }
    }
    int score = (int)p.m;
    const int k = (int)p.k;
    const uint32_t span = tk.hi - tk.lo;
    uint32_t rel = tk.scan_lo - tk.lo;   // column - lo, mod 2^32: a column reports when rel < span
    uint32_t cnt = 0;
    uint64_t best = kNoBest;
    uint32_t pos = FILL ? task_off[tid - t0] : 0;
    const uint2* eq_lane = approx_lds + lane;
    for (uint32_t j0 = tk.scan_lo; j0 < tk.hi; j0 += 16) {
        uint4 v = *reinterpret_cast<const uint4*>(text + j0);
#pragma nounroll
        for (int d = 0; d < 4; ++d) {   // (the four dwords rotate through v.x: no indexed register file access, a quarter of the code)
            const uint32_t x = v.x;
            v = make_uint4(v.y, v.z, v.w, 0);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint32_t code = (x >> (8 * s)) & 0xffu;
                const uint2* eqp = eq_lane + code * (W * 64);
                uint32_t carry = 0, ph_in = 0, mh_in = 0, ph_top = 0, mh_top = 0;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint2 e2 = eqp[w * 64];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int i = 2 * w + h;
                        const uint32_t eq = h ? e2.y : e2.x;
                        const uint32_t sum = __builtin_addc(eq & pv[i], pv[i], carry, &carry);
                        const uint32_t xh = (sum ^ pv[i]) | eq;
                        const uint32_t ph = mv[i] | ~(xh | pv[i]);
                        const uint32_t mh = pv[i] & xh;
                        const uint32_t xv = eq | mv[i];
                        const uint32_t ph1 = __builtin_amdgcn_alignbit(ph, ph_in, 31);
                        const uint32_t mh1 = __builtin_amdgcn_alignbit(mh, mh_in, 31);
                        pv[i] = mh1 | ~(xv | ph1);
                        mv[i] = ph1 & xv;
                        ph_in = ph;
                        mh_in = mh;
                        if (i == N - 1) {
                            ph_top = ph;
                            mh_top = mh;
                        }
                    }
                }
                score += (int)(ph_top >> 31) - (int)(mh_top >> 31);
                if (rel < span && score <= k) {
                    const uint32_t e = tk.lo + rel + 1;
                    if (FILL) {
                        if (pos < out_cap) out[pos] = (uint64_t)e << 32 | (uint32_t)score;
                        ++pos;
                    } else {
                        const uint64_t key = (uint64_t)(uint32_t)score << 32 | e;
                        best = key < best ? key : best;
                        ++cnt;
                    }
                }
                ++rel;
            }
        }
    }
    if (!FILL) {
        task_cnt[tid] = cnt;
        if (cnt) {
            atomicAdd(&pat_cnt[tk.pat], cnt);
            atomicMin(&pat_best[tk.pat], (unsigned long long)best);
        }
    }
}

// ---- start positions of hits (pwa_approx_starts): the same column, anchored, run backwards from a hit's end.
//
// The start of a hit (e, d) is the largest s with ed(p, text[s:e]) <= d: the first column j at which row m of the reversed pattern
// against text[e-1], text[e-2], ... reaches d under D'[0][j] = j, then s = e - j.  The anchored form differs from the search form in two
// places: the pad rows match NO symbol (Eq = 0 for every code) and hold Pv = Mv = 0, and a 1 enters the Ph shift at bit 0 in every
// column.  The pad rows then keep Ph = 1, Mh = 0, Pv = Mv = 0 for good (Xh = 0 there and no carry leaves them) and hand the +1 of row 0
// into pattern row 1; row m is still bit 31 of the last register.

constexpr uint32_t kNoStart = 0xffffffffu;

struct Hit {   // one hit on the device: the pattern, its end and distance as the occurrence list has them, and where its start goes
    uint32_t pat, end, dist, out;
};

// Masks of every REVERSED pattern with the pad bits clear: thread (pattern, code, word), the layout of approx_masks_kernel.
__global__ __launch_bounds__(256) void approx_masks_rev_kernel(const uint8_t* __restrict__ blob, const Pat* __restrict__ pats, uint32_t n_pat, uint32_t rows,
                                                               const CodeTable tab, uint64_t* __restrict__ peq) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t q = x / (rows * kMaxWords);
    const uint32_t r = (uint32_t)(x % (rows * kMaxWords)), code = r / kMaxWords, w = r % kMaxWords;
    if (q >= n_pat) return;
    const Pat p = pats[q];
    if (w >= p.W) return;
    const uint32_t pad = 64 * p.W - p.m;
    uint64_t bits = 0;
    for (uint32_t b = 0; b < 64; ++b) {
        const uint32_t pos = 64 * w + b;
        if (pos >= pad && tab.t[blob[p.off + (p.m - 1 - (pos - pad))]] == code) bits |= 1ull << b;
    }
    peq[p.peq + code * p.W + w] = bits;
}

// One wave per workgroup, lane l of workgroup b runs hits[64 b + l] (below n_hits) and writes start_out[its out].  LDS as the scan's.
// The coded text is read backwards in aligned dwords, the highest byte first and the next dword one ahead; the dword below the one
// that holds text[0] is never addressed (a lane has stopped by then: j = e is its last column at the latest).
template <int W>
__global__ __launch_bounds__(64) void approx_start_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ peq, const Pat* __restrict__ pats,
                                                          const Hit* __restrict__ hits, uint32_t n_hits, uint32_t rows, uint32_t* __restrict__ start_out) {
    extern __shared__ uint2 approx_lds[];
    constexpr int N = 2 * W;
    const uint32_t lane = threadIdx.x;
    const uint32_t idx = blockIdx.x * 64 + lane;
    if (idx >= n_hits) return;
    const Hit h = hits[idx];
    const Pat p = pats[h.pat];
    const int dist = (int)h.dist;
    int score = (int)p.m;
    if (score <= dist) {   // j = 0, before any symbol: the empty substring
        start_out[h.out] = h.end;
        return;
    }
    {
        const uint2* src = reinterpret_cast<const uint2*>(peq + p.peq);
        for (uint32_t i = 0; i < rows * W; ++i) approx_lds[i * 64 + lane] = src[i];
    }
    uint32_t pv[N], mv[N];
    {
        const uint32_t pad = 64 * W - p.m;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const uint32_t b = 32 * i;   // ones from bit pad up
            pv[i] = pad <= b ? ~0u : pad >= b + 32 ? 0u : ~0u << (pad - b);
            mv[i] = 0;
        }
    }
    const uint32_t jmax = h.end < p.m + h.dist ? h.end : p.m + h.dist;   // >= 1
    const uint32_t* text32 = reinterpret_cast<const uint32_t*>(text);
    uint32_t di = (h.end - 1) >> 2;
    uint32_t left = ((h.end - 1) & 3u) + 1;
    uint32_t cur = text32[di] << (8 * (4 - left));
    uint32_t nxt = di ? text32[di - 1] : 0;
    const uint2* eq_lane = approx_lds + lane;
    uint32_t j = 0, res = kNoStart;
    for (;;) {
        if (left == 0) {
            cur = nxt;
            left = 4;
            --di;
            nxt = di ? text32[di - 1] : 0;
        }
        const uint32_t code = cur >> 24;
        cur <<= 8;
        --left;
        const uint2* eqp = eq_lane + code * (W * 64);
        uint32_t carry = 0, ph_in = 0x80000000u, mh_in = 0, ph_top = 0, mh_top = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint2 e2 = eqp[w * 64];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int i = 2 * w + hh;
                const uint32_t eq = hh ? e2.y : e2.x;
                const uint32_t sum = __builtin_addc(eq & pv[i], pv[i], carry, &carry);
                const uint32_t xh = (sum ^ pv[i]) | eq;
                const uint32_t ph = mv[i] | ~(xh | pv[i]);
                const uint32_t mh = pv[i] & xh;
                const uint32_t xv = eq | mv[i];
                const uint32_t ph1 = __builtin_amdgcn_alignbit(ph, ph_in, 31);
                const uint32_t mh1 = __builtin_amdgcn_alignbit(mh, mh_in, 31);
                pv[i] = mh1 | ~(xv | ph1);
                mv[i] = ph1 & xv;
                ph_in = ph;
                mh_in = mh;
                if (i == N - 1) {
                    ph_top = ph;
                    mh_top = mh;
                }
            }
        }
        score += (int)(ph_top >> 31) - (int)(mh_top >> 31);
        ++j;
        if (score <= dist) {
            res = h.end - j;
            break;
        }
        if (j == jmax) break;
    }
    start_out[h.out] = res;
}

}  // namespace approx
}  // namespace pwa
