// chain_top.hip.h -- the selection stage behind the chaining DP: the top-N chains of every read by marked back-walks, as
// include/pwalign.h defines them ("Top-N chains of a read").  One wave per read, four waves per workgroup, nothing passed between
// waves.
//
// The candidates of a read arrive sorted (f descending, the smaller index first): S holds the local anchor indices in that order, the
// work of the suffix-array unit's radix sort over the keys chain_top_keys_kernel writes.  A block of 64 candidates is loaded coalesced,
// their f and marks gathered, and the free ones with f >= min_score balloted; the lowest lane's candidate is walked as chain.hip.h's
// back-walk walks (one round of loads per block of 64 anchors, hops through readlane, wave-uniform control flow), its anchors marked,
// and the block's marks gathered again, because the walk may have claimed a later candidate.  The marks a wave reads back are its own
// stores: a workgroup-scope fence and relaxed workgroup-scope atomics, as the back-walk does for pred -- no agent-scope fence, no spin.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain.hip.h"

namespace pwa {
namespace chain {

constexpr int32_t kFree = -1, kDropped = -2;   // an anchor's mark: free, the kept chain's index c >= 0, or claimed by a dropped walk
constexpr uint32_t kTopRecWords = 10;          // a kept chain: score, count, last, q_b, y_e, t_b, x_e, diag_lo, diag_hi, branch
constexpr uint32_t kTopHeadWords = 4;          // a read: chains kept, rounds, the best score among its rooted chains 1 .., 0
constexpr uint32_t kRooted = 1;                // PWA_CHAIN_ROOTED

struct TopParams {
    const uint32_t *t, *q, *len;   // the range's anchors
    const Read* reads;
    uint32_t n_reads;
    const int32_t *f, *pred;       // the DP chain_kernel left on the device
    const uint32_t* sorted;        // per read, at its anchors' place: the local indices in candidate order
    int32_t* mark;                 // one per anchor
    uint32_t max_chains;
    int32_t min_score;
    uint32_t min_count, flags;
    int32_t* rec;                  // kTopRecWords per (read of the range, chain slot)
    uint32_t* head;                // kTopHeadWords per read of the range
    uint32_t* fault;               // one word: set when a loop met its bound or a pred does not point backwards
};

// The sort's input: key = read << 32 | (0x7FFFFFFF - f), value = the anchor's local index; every mark free
__global__ __launch_bounds__(64 * kWaves) void chain_top_keys_kernel(const Read* reads, uint32_t n_reads, const int32_t* f, uint64_t* key, uint32_t* val,
                                                                     int32_t* mark) {
    const uint32_t w = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (w >= n_reads) return;
    const Read R = reads[w];
    for (uint32_t i = threadIdx.x & 63; i < R.n; i += 64) {
        key[R.at + i] = ((uint64_t)R.out << 32) | (uint32_t)(0x7FFFFFFF - f[R.at + i]);
        val[R.at + i] = i;
        mark[R.at + i] = kFree;
    }
}

struct Walk {
    uint32_t count, b;
    int32_t dlo, dhi, branch;
    bool ended;
};

// One walk from e.  CLAIM: stop before a marked anchor, note the span and the diagonals; otherwise exactly `hops` anchors are marked
// again (a dropped walk's second pass).  Every anchor visited gets mark `value`, stored once per block of 64
template <bool CLAIM>
__device__ __forceinline__ Walk walk_from(uint32_t e, uint32_t n, uint32_t hops, int32_t value, const int32_t* P, const uint32_t* T, const uint32_t* Q,
                                          int32_t* M, int lane) {
    Walk w{0u, e, INT32_MAX, INT32_MIN, -1, false};
    uint32_t cur = e;
    bool stop = false;
    while (!stop && w.count < hops) {
        const uint32_t base = cur & ~63u, idx = base + lane;
        int32_t pv = -1, dv = 0, mv = kFree;
        if (idx < n) {
            pv = P[idx];
            if (CLAIM) {
                mv = __hip_atomic_load(M + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                dv = (int32_t)(T[idx] - Q[idx]);
            }
        }
        bool mine = false;   // this lane's anchor is part of the walk
        do {
            const uint32_t at = cur - base;
            if (CLAIM && __builtin_amdgcn_readlane(mv, at) != kFree) {   // never at e itself: it was balloted free
                w.branch = (int32_t)cur;
                w.ended = true;
                stop = true;
                break;
            }
            const int32_t p = __builtin_amdgcn_readlane(pv, at);
            if (CLAIM) {
                const int32_t d = __builtin_amdgcn_readlane(dv, at);
                w.dlo = min(w.dlo, d);
                w.dhi = max(w.dhi, d);
            }
            mine = mine || lane == (int)at;
            ++w.count;
            w.b = cur;
            if (p < 0 || (uint32_t)p >= cur) {   // the walk's first anchor, or a pred that does not point backwards
                w.ended = p < 0;
                stop = true;
                break;
            }
            cur = (uint32_t)p;
        } while (cur >= base && w.count < hops);
        if (mine) __hip_atomic_store(M + idx, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // mine: idx < n
    }
    return w;
}

__global__ __launch_bounds__(64 * kWaves) void chain_top_kernel(const TopParams a) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    if (w >= a.n_reads) return;
    const int lane = threadIdx.x & 63;
    const Read R = a.reads[w];
    const uint32_t n = __builtin_amdgcn_readfirstlane(R.n);
    const uint32_t* __restrict__ T = a.t + R.at;
    const uint32_t* __restrict__ Q = a.q + R.at;
    const uint32_t* __restrict__ L = a.len + R.at;
    const int32_t* __restrict__ F = a.f + R.at;
    const int32_t* P = a.pred + R.at;
    const uint32_t* __restrict__ S = a.sorted + R.at;
    int32_t* M = a.mark + R.at;
    const uint32_t N = a.max_chains, min_count = a.min_count;
    const int32_t min_score = a.min_score;
    const bool rooted = (a.flags & kRooted) != 0;

    uint32_t kept = 0, rounds = 0;
    int32_t second = 0;   // the best score among the kept chains 1 .. with branch = -1
    bool fault = false, done = false;
    for (uint32_t base = 0; base < n && !done; base += 64) {
        const uint32_t pos = base + lane;
        uint32_t ci = 0;
        int32_t cf = INT32_MIN;
        if (pos < n) {
            ci = S[pos];
            cf = ci < n ? F[ci] : INT32_MIN;
        }
        const bool cand = cf >= min_score;
        if (__builtin_amdgcn_ballot_w64(cand) != ~0ull) done = true;   // f descends: no later block holds a candidate
        for (int it = 0; it <= 64; ++it) {                             // every round claims a candidate of this block
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // the marks this wave stored
            const int32_t mk = cand ? __hip_atomic_load(M + ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : kDropped;
            const uint64_t open = __builtin_amdgcn_ballot_w64(mk == kFree);
            if (!open) break;
            if (it == 64 || rounds >= n) {
                fault = done = true;
                break;
            }
            const int l = __builtin_ctzll(open);
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ci, l);
            const int32_t fe = __builtin_amdgcn_readlane(cf, l);
            ++rounds;
            const Walk k = walk_from<true>(e, n, n, (int32_t)kept, P, T, Q, M, lane);
            if (!k.ended) {
                fault = done = true;
                break;
            }
            const int32_t score = fe - (k.branch >= 0 ? F[k.branch] : 0);
            if (score >= min_score && k.count >= min_count && (!rooted || k.branch < 0)) {
                if (lane == 0) {
                    int32_t* rec = a.rec + ((uint64_t)R.out * N + kept) * kTopRecWords;
                    const uint32_t le = L[e];
                    rec[0] = score;
                    rec[1] = (int32_t)k.count;
                    rec[2] = (int32_t)e;
                    rec[3] = (int32_t)Q[k.b];
                    rec[4] = (int32_t)(Q[e] + le);
                    rec[5] = (int32_t)T[k.b];
                    rec[6] = (int32_t)(T[e] + le);
                    rec[7] = k.dlo;
                    rec[8] = k.dhi;
                    rec[9] = k.branch;
                }
                if (kept && k.branch < 0) second = max(second, score);
                if (++kept == N) {
                    done = true;
                    break;
                }
            } else {
                (void)walk_from<false>(e, n, k.count, kDropped, P, T, Q, M, lane);
            }
        }
    }
    if (lane == 0) {
        uint32_t* head = a.head + (uint64_t)R.out * kTopHeadWords;
        head[0] = kept;
        head[1] = rounds;
        head[2] = (uint32_t)second;
        head[3] = 0;
        if (fault) *a.fault = 1u;
    }
}

}  // namespace chain
}  // namespace pwa
