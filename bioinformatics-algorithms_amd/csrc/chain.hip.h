// chain.hip.h -- the kernel of the chaining unit: the collinear-chaining DP of include/pwalign.h ("Collinear chaining of anchors")
// over the anchors of many reads, one wave per read, four waves per workgroup, nothing passed between waves.
//
// The look-back window lives in registers: lane L of chunk c holds (x, y, f) of predecessor i - 1 - L - 64 c, and after every step the
// whole window moves one lane up with a wave_shr:1 DPP move -- lane 0 of chunk 0 takes the anchor just finished, lane 0 of chunk c
// lane 63 of chunk c - 1.  The step's own anchor is wave-uniform: a block of 64 anchors is loaded coalesced and read with readlane.
// The winner of a step is the wave's maximum of the 64-bit key cand << 32 | j (the largest j among equal cand), reduced inside each
// row of 16 lanes by DPP and across the four rows by readlane.  The back-walk runs in the same kernel behind a workgroup-scope fence
// (it reads pred words other lanes of the wave stored; the wave's own stores, the CU's own L1 -- no agent-scope fence anywhere).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pwa {
namespace chain {

constexpr int kWaves = 4;            // waves (reads) per workgroup
constexpr uint32_t kRecWords = 10;   // a read's result record: score, count, last, q_b, y_e, t_b, x_e, diag_lo, diag_hi, 0

struct Read {        // one entry of a range's launch list
    uint64_t at;     // first anchor of the read in the range's arrays
    uint32_t n;      // its anchors, >= 1
    uint32_t out;    // its place among the range's reads: the record it writes
};

struct Params {
    const uint32_t *t, *q, *len;   // the range's anchors
    const Read* reads;
    uint32_t n_reads;
    int32_t lookback, max_dist, bandwidth;
    uint32_t gap_scale;
    int32_t *f, *pred;             // one per anchor, local indices
    int32_t* rec;                  // kRecWords per read of the range
    uint32_t* fault;               // one word: set when a back-walk met a pred that does not point backwards
};

__device__ __forceinline__ int shr1(int fill, int v) {   // lane k <- lane k-1; lane 0 takes `fill`
    return __builtin_amdgcn_update_dpp(fill, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

template <int CTRL>
__device__ __forceinline__ int64_t max_with(int64_t k) {   // max of every lane's key and the key of its DPP partner
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(k >> 32), CTRL, 0xf, 0xf, false);
    const int64_t o = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    return o > k ? o : k;
}

// The wave's maximum key, wave-uniform.  Every partner pattern is an involution inside a row of 16 lanes (no lane without a source)
__device__ __forceinline__ int64_t wave_max(int64_t k) {
    k = max_with<0xB1 /* quad_perm:[1,0,3,2] */>(k);
    k = max_with<0x4E /* quad_perm:[2,3,0,1] */>(k);
    k = max_with<0x141 /* row_half_mirror */>(k);
    k = max_with<0x140 /* row_mirror */>(k);
    int64_t best = INT64_MIN;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, 16 * row);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(k >> 32), 16 * row);
        const int64_t o = (int64_t)(((uint64_t)hi << 32) | lo);
        best = o > best ? o : best;
    }
    return best;
}

// C: chunks of 64 predecessors the window holds, 64 C >= lookback
template <int C>
__device__ __forceinline__ void chain_read(const Params& a) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    if (w >= a.n_reads) return;
    const int lane = threadIdx.x & 63;
    const Read R = a.reads[w];
    const uint32_t n = __builtin_amdgcn_readfirstlane(R.n);
    const uint32_t* __restrict__ T = a.t + R.at;
    const uint32_t* __restrict__ Q = a.q + R.at;
    const uint32_t* __restrict__ L = a.len + R.at;
    int32_t* F = a.f + R.at;
    int32_t* P = a.pred + R.at;
    const int32_t H = a.lookback, max_dist = a.max_dist, bandwidth = a.bandwidth;
    const uint32_t gap_scale = a.gap_scale;

    int xw[C], yw[C], fw[C];   // the window; a lane's values count only once its predecessor index is >= 0
#pragma unroll
    for (int c = 0; c < C; ++c) xw[c] = yw[c] = fw[c] = 0;
    int32_t best_f = INT32_MIN;
    uint32_t best_e = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t idx = base + lane;
        int bx = 0, by = 0, bl = 0;   // this block's anchors, one per lane
        if (idx < n) {
            bl = (int)L[idx];
            bx = (int)(T[idx] + (uint32_t)bl);
            by = (int)(Q[idx] + (uint32_t)bl);
        }
        int of = 0, op = 0;           // this block's results, one per lane
        const uint32_t cnt = min(64u, n - base);
        for (uint32_t s = 0; s < cnt; ++s) {
            const int xi = __builtin_amdgcn_readlane(bx, s), yi = __builtin_amdgcn_readlane(by, s), li = __builtin_amdgcn_readlane(bl, s);
            const int32_t i = (int32_t)(base + s);
            int64_t key = INT64_MIN;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int32_t off = lane + 64 * c, j = i - 1 - off;
                const int32_t dx = xi - xw[c], dy = yi - yw[c];
                const uint32_t dd = (uint32_t)abs(dx - dy);
                const bool adm = j >= 0 && off < H && dx > 0 && dx <= max_dist && dy > 0 && dy <= max_dist && dd <= (uint32_t)bandwidth;
                const uint32_t beta = dd ? ((gap_scale * dd) >> 8) + ((31u - (uint32_t)__builtin_clz(dd | 1u)) >> 1) : 0u;
                const int32_t cand = (int32_t)((uint32_t)fw[c] + (uint32_t)min(li, min(dx, dy)) - beta);
                const int64_t k = adm ? (int64_t)(((uint64_t)(uint32_t)cand << 32) | (uint32_t)j) : INT64_MIN;
                key = k > key ? k : key;
            }
            key = wave_max(key);
            const int32_t cand = (int32_t)(key >> 32);
            const bool take = key != INT64_MIN && cand > li;
            const int32_t fi = take ? cand : li, pi = take ? (int32_t)(uint32_t)key : -1;
            if (lane == (int)s) {
                of = fi;
                op = pi;
            }
            if (fi > best_f) {   // strictly: the smallest index with maximal f
                best_f = fi;
                best_e = (uint32_t)i;
            }
#pragma unroll
            for (int c = C - 1; c > 0; --c) {
                xw[c] = shr1(__builtin_amdgcn_readlane(xw[c - 1], 63), xw[c]);
                yw[c] = shr1(__builtin_amdgcn_readlane(yw[c - 1], 63), yw[c]);
                fw[c] = shr1(__builtin_amdgcn_readlane(fw[c - 1], 63), fw[c]);
            }
            xw[0] = shr1(xi, xw[0]);
            yw[0] = shr1(yi, yw[0]);
            fw[0] = shr1(fi, fw[0]);
        }
        if (idx < n) {
            F[idx] = of;
            P[idx] = op;
        }
    }

    // The back-walk: from e along pred, at most n anchors, each hop strictly backwards; everything that steers it is wave-uniform
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the pred words other lanes of this wave stored
    uint32_t cur = best_e, b = best_e, count = 0;
    int32_t dlo = INT32_MAX, dhi = INT32_MIN;
    bool ended = false;
    // A chain mostly steps to a near predecessor: the 64 anchors of cur's block are loaded at once (pred and t - q, one per lane) and
    // the walk hops through readlane until it leaves the block downwards -- one round of loads per block, not per hop
    bool stop = false;
    while (!stop && count < n) {
        const uint32_t base = cur & ~63u, idx = base + lane;
        int32_t pv = -1, dv = 0;
        if (idx < n) {
            pv = __hip_atomic_load(P + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            dv = (int32_t)(T[idx] - Q[idx]);
        }
        do {
            const int32_t d = __builtin_amdgcn_readlane(dv, cur - base), p = __builtin_amdgcn_readlane(pv, cur - base);
            dlo = min(dlo, d);
            dhi = max(dhi, d);
            ++count;
            b = cur;
            if (p < 0 || (uint32_t)p >= cur) {   // the chain's first anchor, or a pred that does not point backwards
                ended = p < 0;
                stop = true;
                break;
            }
            cur = (uint32_t)p;
        } while (cur >= base && count < n);
    }
    if (lane == 0) {
        int32_t* rec = a.rec + (uint64_t)R.out * kRecWords;
        const uint32_t le = L[best_e];
        rec[0] = best_f;
        rec[1] = (int32_t)count;
        rec[2] = (int32_t)best_e;
        rec[3] = (int32_t)Q[b];
        rec[4] = (int32_t)(Q[best_e] + le);
        rec[5] = (int32_t)T[b];
        rec[6] = (int32_t)(T[best_e] + le);
        rec[7] = dlo;
        rec[8] = dhi;
        rec[9] = 0;
        if (!ended) *a.fault = 1u;
    }
}

template <int C>
__global__ __launch_bounds__(64 * kWaves) void chain_kernel(const Params a) {
    chain_read<C>(a);
}

}  // namespace chain
}  // namespace pwa
