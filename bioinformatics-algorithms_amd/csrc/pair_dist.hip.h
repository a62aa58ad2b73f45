// pair_dist.hip.h -- hw4's NW distance of long pairs on the stripe engine (gfx950 / MI355X).
//
// Replaces, per pair, hw4/hw4.cpp:16-72 (needleman_wunsch with hw4's tie-break: v = diag + s; if (up > v) up; if (left > v)
// left -- diag >= up >= left) followed by the distance rule of main (146-152), like the strip kernels of batch_nwdist.hip.h,
// but with the stripe engine's mapping (pair_fill.hip.h): a pair is cut into stripes of 64 * RL rows, one wave per stripe
// sweeps anti-diagonals, the row above a lane's first row comes from lane k-1 through a DPP wave shift, stripes of a
// workgroup pass their bottom rows through an LDS ring, and a helper wave owns every HBM hand-off between workgroups.
// A list of few long pairs (16 mitochondrial genomes = 120 pairs) thus runs on thousands of waves instead of 120 lanes.
//
// Every cell carries TWO values, the score and the distance of the path the reference's walk takes through it:
//     key = H * 4 + prio, prio(diag) = 2, prio(up) = 1, prio(left) = 0   -- one max3 over three keys picks hw4's winner
//     D   = D[pred] + (diag ? (s1[i-1] != s2[j-1]) : 1),  D[i][0] = i, D[0][j] = j
// Cells are kept as (4 H, D); both travel together through every hand-off (DPP shift, LDS ring, HBM row: one 64-bit
// word per column).  The result is D (and H) at (n, m), written by the lane that holds row n: no band, no walk.
// The host routes only pairs whose keys stay inside int32 ((n + m + 2) * max|score| < 2^28, pwalign.hip).
#pragma once
#include "pair_fill.hip.h"

namespace pwa {

typedef PWA_GLOBAL uint64_t g_u64;

template <int W>
struct DistShared {
    int ring_h[W + 1][kRing];     // ring[w]: row above compute wave w (4 H); ring[W]: bottom row of the last wave
    int ring_d[W + 1][kRing];     // ... and its distances
    uint8_t text[kTRing];
    uint32_t ready[W + 1];        // columns written into ring[w]
    uint32_t taken[W + 1];        // columns consumed from ring[w]
    uint32_t txt_ready;
    uint32_t task;
};

__device__ __forceinline__ uint64_t dist_pack(int h, int d) { return (uint64_t)(uint32_t)h | ((uint64_t)(uint32_t)d << 32); }

// One anti-diagonal step of a stripe.  EDGE = some lanes of this step lie outside the matrix (their state stays frozen,
// so a lane that has left keeps its last column's values).
//   hk, hd: (4 H, D) of the lane's rows at the previous column;  dk, dd: the diagonal of row 0;  bk, bd: the lane's bottom row
//   km, kx: 4 s + 2 for a match / mismatch;  ku = 4 gap + 1, kl = 4 gap
template <int RL, bool EDGE>
__device__ __forceinline__ void dist_step(int t, int lane, int m, const int (&pc)[RL], int (&hk)[RL], int (&hd)[RL], int& dk, int& dd,
                                          int& bk, int& bd, int& tch, int& topk, int& topd, int& tcv, int& colk, int& cold, int km,
                                          int kx, int ku, int kl) {
    const int up_k = wave_shr1(topk, bk);   // (4 H, D)[i_first-1][j]; lane 0: the staged row above the stripe
    const int up_d = wave_shr1(topd, bd);
    tch = wave_shr1(tcv, tch);              // text symbol of column c; lane 0: the staged text
    topk = wave_shl1(topk, topk);           // rotate the staged vectors: lane 0 sees the next column next step
    topd = wave_shl1(topd, topd);
    tcv = wave_shl1(tcv, tcv);
    const int c = t - lane;
    if (!EDGE || (c >= 0 && c < m)) {
        int gk = dk, gd = dd, uk = up_k, ud = up_d;
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const bool eq = pc[r] == tch;
            const int kd = p_addw(gk, eq ? km : kx);                           // hw4.cpp:36   diag + s
            const int kup = p_addw(uk, ku), klf = p_addw(hk[r], kl);           //      32-33  up + gap, left + gap
            const int k = max(kd, max(kup, klf));                              //      36-47  diag >= up >= left
            const int d = (k == kd) ? p_addw(gd, eq ? 0 : 1) : p_addw((k == kup) ? ud : hd[r], 1);   // 146-152 along the walk
            gk = hk[r];
            gd = hd[r];
            uk = k & ~3;
            ud = d;
            hk[r] = uk;
            hd[r] = d;
        }
        dk = up_k;
        dd = up_d;
        bk = uk;
        bd = ud;
    }
    colk = wave_shl1(bk, colk);   // lane 63 inserts its bottom-row values (column t-63), the rest shifts down
    cold = wave_shl1(bd, cold);
}

template <int RL, int W>
__global__ __launch_bounds__(64 * (W + 1)) void pair_dist_kernel(const PairParams G) {
    constexpr int CH = kCH;
    __shared__ DistShared<W> sh;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gap = G.gap;
    const uint32_t spin_limit = 1u << 26;
    for (;;) {
        __syncthreads();   // everybody is done with the previous task's LDS state
        if (threadIdx.x == 0) sh.task = atomicAdd(G.queue, 1u);
        if (threadIdx.x < 2 * (W + 1) + 1) {
            if (threadIdx.x <= W) sh.ready[threadIdx.x] = 0;
            else if (threadIdx.x <= 2 * W + 1) sh.taken[threadIdx.x - (W + 1)] = 0;
            else sh.txt_ready = 0;
        }
        __syncthreads();
        const uint32_t tid = __builtin_amdgcn_readfirstlane(sh.task);
        if (tid >= G.n_tasks) break;
        const StripeTask task = G.tasks[tid];
        const PairDesc P = G.pairs[task.pair];
        const int ss = (int)task.super;
        const int n = P.n, m = P.m;
        const int T = m + 63;
        const int n_chunks = (T + CH - 1) / CH;
        const int n_super = ((int)P.n_stripes + W - 1) / W;
        const bool top_global = ss > 0, bot_global = ss + 1 < n_super;
        const int wl = min(W - 1, (int)P.n_stripes - 1 - ss * W);   // last active compute wave
        g_cu8* txt = (g_cu8*)P.txt;

        if (wave == W) {
            // =================== helper wave: every global-memory hand-off of this workgroup (as in pair_fill_kernel) ===================
            // rows: one 64-bit word (4 H, D) per column, super-stripe s at rows + 2 * s * row_stride (int32 units)
            g_u64* rin = (g_u64*)P.rows + (size_t)(top_global ? ss - 1 : 0) * P.row_stride;
            g_u64* rout = (g_u64*)P.rows + (size_t)ss * P.row_stride;
            g_u32* prog_in = (g_u32*)(G.progress + (top_global ? tid - 1 : tid));   // previous super-stripe, same pair
            g_u32* prog_out = (g_u32*)(G.progress + tid);
            int kin = 0, kout = 0;
            uint32_t idle = 0;
            for (;;) {
                const bool done_in = kin >= m, done_out = !bot_global || kout >= m;
                if (done_in && done_out) break;
                bool progress = false;
                if (!done_in) {   // ---- stage text + the row above wave 0, up to kTrip columns per trip
                    int lim = min(m, min((int)lds_peek(&sh.taken[0]) + kRing, (int)lds_peek(&sh.taken[wl]) + kTRing));
                    if (top_global) lim = min(lim, (int)__hip_atomic_load(prog_in, PWA_RLX_AGENT));   // sc1 poll
                    const int hi = min(lim, kin + kTrip);
                    if (hi > kin) {
                        uint64_t v[kTrip / 64];
                        int tc[kTrip / 64];
#pragma unroll
                        for (int u = 0; u < kTrip / 64; ++u) {   // all loads of the trip in flight together
                            const int c = kin + u * 64 + lane;
                            v[u] = 0;
                            tc[u] = 0;
                            if (c < hi) {
                                if (top_global) v[u] = __hip_atomic_load(rin + c, PWA_RLX_AGENT);   // sc1: issued after the poll's value is known
                                else v[u] = dist_pack(p_mulw(c + 1, 4 * gap), c + 1);              // (4 H, D)[0][j], hw4.cpp:25-28
                                tc[u] = txt[c];
                            }
                        }
#pragma unroll
                        for (int u = 0; u < kTrip / 64; ++u) {
                            const int c = kin + u * 64 + lane;
                            if (c < hi) {
                                sh.ring_h[0][ring_slot(c)] = (int)(uint32_t)v[u];
                                sh.ring_d[0][ring_slot(c)] = (int)(uint32_t)(v[u] >> 32);
                                sh.text[c % kTRing] = (uint8_t)tc[u];
                            }
                        }
                        lds_post(&sh.ready[0], (uint32_t)hi);
                        lds_post(&sh.txt_ready, (uint32_t)hi);
                        kin = hi;
                        progress = true;
                    }
                }
                if (!done_out) {   // ---- publish the bottom row of the last wave
                    const int hi = min((int)lds_peek(&sh.ready[W]), kout + kTrip);
                    if (hi > kout) {
#pragma unroll
                        for (int u = 0; u < kTrip / 64; ++u) {
                            const int c = kout + u * 64 + lane;
                            if (c < hi) __hip_atomic_store(rout + c, dist_pack(sh.ring_h[W][ring_slot(c)], sh.ring_d[W][ring_slot(c)]), PWA_RLX_AGENT);   // sc1
                        }
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                   // only this wave's own stores
                        if (lane == 0) __hip_atomic_store(prog_out, (uint32_t)hi, PWA_RLX_AGENT);
                        lds_post(&sh.taken[W], (uint32_t)hi);
                        kout = hi;
                        progress = true;
                    }
                }
                if (progress) {
                    idle = 0;
                } else {
                    if (top_global || bot_global) __builtin_amdgcn_s_sleep(2);
                    else __builtin_amdgcn_s_sleep(PWA_HELPER_NAP);
                    if (++idle > spin_limit) {   // bounded: flag the failure, let the host report it
                        if (lane == 0) __hip_atomic_store((g_u32*)(G.queue + 1), 1u, PWA_RLX_AGENT);
                        break;
                    }
                }
            }
        } else if (wave <= wl) {
            // =================== compute wave `wave`: stripe ss*W + wave ===================
            const int s = ss * W + wave;
            const bool has_out = wave < wl || (wave == W - 1 && bot_global);
            const int i_first = s * 64 * RL + lane * RL + 1;   // first row of this lane (1-based)
            int pc[RL], hk[RL], hd[RL];
#pragma unroll
            for (int r = 0; r < RL; ++r) {
                const int i = i_first + r;
                pc[r] = (i <= n) ? (int)((g_cu8*)P.pat)[i - 1] : 256;   // 256 never equals a text symbol
                hk[r] = p_mulw(i, 4 * gap);                               // (4 H, D)[i][0], hw4.cpp:21-24
                hd[r] = i;
            }
            int dk = p_mulw(i_first - 1, 4 * gap), dd = i_first - 1;     // (4 H, D)[i_first-1][0]
            const int km = (int)((unsigned)G.match * 4u + 2u), kx = (int)((unsigned)G.mismatch * 4u + 2u);
            const int ku = (int)((unsigned)gap * 4u + 1u), kl = (int)((unsigned)gap * 4u);
            int* rin_h = sh.ring_h[wave];
            int* rin_d = sh.ring_d[wave];
            int* rout_h = sh.ring_h[wave + 1];
            int* rout_d = sh.ring_d[wave + 1];
            int bk = 0, bd = 0, tch = 0, colk = 0, cold = 0;
            bool failed = false;
            for (int ch = 0; ch < n_chunks; ++ch) {
                const int t0 = ch * CH;
                // ---- wait for the row above and the text of columns t0 .. t0+CH-1, then take them
                const uint32_t need = (uint32_t)min(m, t0 + CH);
                for (uint32_t spins = 0; !failed && (lds_peek(&sh.ready[wave]) < need || lds_peek(&sh.txt_ready) < need);) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > spin_limit) failed = true;
                }
                const int c0 = t0 + lane;
                int topk = 0, topd = 0, tcv = 0;
                if (lane < CH && c0 < m) {
                    topk = rin_h[ring_slot(c0)];
                    topd = rin_d[ring_slot(c0)];
                    tcv = sh.text[c0 % kTRing];
                }
                lds_post(&sh.taken[wave], need);
                if (t0 >= 63 && t0 + CH < m) {   // every lane inside the matrix
#pragma unroll PWA_STEP_UNROLL
                    for (int q = 0; q < CH; ++q)
                        dist_step<RL, false>(t0 + q, lane, m, pc, hk, hd, dk, dd, bk, bd, tch, topk, topd, tcv, colk, cold, km, kx, ku, kl);
                } else {
                    const int qn = min(CH, T - t0);
#pragma unroll 1
                    for (int q = 0; q < qn; ++q)
                        dist_step<RL, true>(t0 + q, lane, m, pc, hk, hd, dk, dd, bk, bd, tch, topk, topd, tcv, colk, cold, km, kx, ku, kl);
#pragma unroll 1
                    for (int q = qn; q < CH; ++q) {   // keep the collectors aligned
                        colk = wave_shl1(bk, colk);
                        cold = wave_shl1(bd, cold);
                    }
                }
                // ---- bottom row out: after the chunk lane 64-CH+q holds column t0 - 63 + q
                if (has_out) {
                    const int hi = min(m, t0 - 63 + CH);
                    if (hi > 0) {
                        for (uint32_t spins = 0; !failed && hi - (int)lds_peek(&sh.taken[wave + 1]) > kRing;) {   // ring full
                            __builtin_amdgcn_s_sleep(1);
                            if (++spins > spin_limit) failed = true;
                        }
                        const int c = t0 - 63 + (lane - (64 - CH));
                        if (lane >= 64 - CH && c >= 0 && c < m) {
                            rout_h[ring_slot(c)] = colk;
                            rout_d[ring_slot(c)] = cold;
                        }
                        lds_post(&sh.ready[wave + 1], (uint32_t)hi);
                    }
                }
            }
            if (failed && lane == 0) __hip_atomic_store((g_u32*)(G.queue + 1), 1u, PWA_RLX_AGENT);
            // (4 H, D)[n][m]: a lane's state froze when it left the matrix, so the lane that holds row n has its last column
#pragma unroll
            for (int r = 0; r < RL; ++r)
                if (i_first + r == n) {
                    ((PWA_GLOBAL PairResult*)P.res)->score = hk[r] >> 2;
                    if (G.scores_out) ((g_i32*)G.scores_out)[P.out_index] = hd[r];
                }
        }
    }
}

}  // namespace pwa
