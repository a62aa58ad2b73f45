// pair_affine.hip.h -- hw3's affine-gap score of long pairs on the stripe engine (gfx950 / MI355X).
//
// Replaces, per pair, affine_alignment(s1, s2, ..., &score) of hw3/hw3.cpp:23-102 (score only), like the strip kernels of
// batch_affine.hip.h, but with the stripe engine's mapping (pair_fill.hip.h) and the skeleton of pair_dist.hip.h unchanged: a pair
// is cut into stripes of 64 * RL rows, one wave per stripe sweeps anti-diagonals, the row above a lane's first row comes from lane
// k-1 through a DPP wave shift, stripes of a workgroup pass their bottom rows through an LDS ring, and a helper wave owns every HBM
// hand-off between workgroups.  hw3's 120 all-pairs scores of 16 genomes thus run on thousands of waves instead of 120 lanes.
//
// As long as no int32 sum wraps, addition distributes over max, so hw3's V / F / E (55-84) are carried as
//     V = M[i-1][j-1] + s(i,j)       (59-68: the max over V, F, E of the diagonal, plus s)
//     F = G[i-1][j]   + ge           (70-75)
//     E = X[i][j-1]   + ge           (77-82)
//     M = max3(V, F, E)              (86-97 at (n, m): the score)
//     G = max(V + go, F)             (F of the row below)
//     X = max(V + go, E)             (E of the next column, same row)
// Only (M, G) cross rows: they travel together through every hand-off (DPP shift, LDS ring, HBM row: one 64-bit word per column),
// the payload pair_dist moves as (4 H, D).  X and the previous column's M stay in registers, per row.
// Boundaries (39-52): M[0][0] = 0; M[0][j] = E[0][j] = go + ge (j-1); M[i][0] = F[i][0] = go + ge (i-1); G[0][j] (V, F = -inf) and
// X[i][0] (V, E = -inf) are sentinels.  V is a real path value from row 1 and column 1 on, so the sentinel kNeg = -2^29 (+ ge, once)
// never wins a max while real values stay inside +-2^28 -- which the host guarantees before it routes a list here
// ((n + m + 2) * max(|match|, |mismatch|, |go| + |ge|) < 2^28, pwalign.hip).  Ties do not matter: only the value is returned.
// No band, no walk: the lane that holds row n writes M[n][m] into the score vector.
#pragma once
#include "pair_dist.hip.h"

namespace pwa {

constexpr int kAffNeg = -(1 << 29);

// One anti-diagonal step of a stripe.  EDGE = some lanes of this step lie outside the matrix (their state stays frozen, so a lane
// that has left keeps its last column's values).
//   hm, hx: M and X of the lane's rows at the previous column;  dm: M of the row above row 0 at the previous column (the diagonal);
//   bm, bg: (M, G) of the lane's bottom row;  top*, tcv: the staged row above the stripe and the text, rotated one lane per step;
//   colm, colg: the bottom row of lane 63, collected for the ring
template <int RL, bool EDGE>
__device__ __forceinline__ void aff_step(int t, int lane, int m, const int (&pc)[RL], int (&hm)[RL], int (&hx)[RL], int& dm, int& bm,
                                         int& bg, int& tch, int& topm, int& topg, int& tcv, int& colm, int& colg, int sm, int sx,
                                         int go, int ge) {
    const int up_m = wave_shr1(topm, bm);   // (M, G)[i_first-1][j]; lane 0: the staged row above the stripe
    const int up_g = wave_shr1(topg, bg);
    tch = wave_shr1(tcv, tch);              // text symbol of column c; lane 0: the staged text
    topm = wave_shl1(topm, topm);           // rotate the staged vectors: lane 0 sees the next column next step
    topg = wave_shl1(topg, topg);
    tcv = wave_shl1(tcv, tcv);
    const int c = t - lane;
    if (!EDGE || (c >= 0 && c < m)) {
        int dg = dm, ug = up_g;
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int v = p_addw(dg, pc[r] == tch ? sm : sx);   // hw3.cpp:57-68
            const int f = p_addw(ug, ge);                       //         70-75
            const int e = p_addw(hx[r], ge);                    //         77-82
            const int vo = p_addw(v, go);
            dg = hm[r];
            hm[r] = max(v, max(f, e));
            hx[r] = max(vo, e);
            ug = max(vo, f);
        }
        dm = up_m;
        bm = hm[RL - 1];
        bg = ug;
    }
    colm = wave_shl1(bm, colm);   // lane 63 inserts its bottom-row values (column t-63), the rest shifts down
    colg = wave_shl1(bg, colg);
}

template <int RL, int W>
__global__ __launch_bounds__(64 * (W + 1)) void pair_affine_kernel(const PairParams G) {
    constexpr int CH = kCH;
    __shared__ DistShared<W> sh;   // ring_h: M, ring_d: G
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int go = G.gap, ge = G.gap_extend;
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
            // =================== helper wave: every global-memory hand-off of this workgroup (as in pair_dist_kernel) ===================
            // rows: one 64-bit word (M, G) per column, super-stripe s at rows + 2 * s * row_stride (int32 units)
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
                                else v[u] = dist_pack(p_addw(go, p_mulw(c, ge)), kAffNeg);         // (M, G)[0][c+1], hw3.cpp:48-53
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
            int pc[RL], hm[RL], hx[RL];
#pragma unroll
            for (int r = 0; r < RL; ++r) {
                const int i = i_first + r;
                pc[r] = (i <= n) ? (int)((g_cu8*)P.pat)[i - 1] : 256;   // 256 never equals a text symbol
                hm[r] = p_addw(go, p_mulw(i - 1, ge));                    // M[i][0] = F[i][0], hw3.cpp:42-47
                hx[r] = kAffNeg;                                          // X[i][0]: V, E = -inf
            }
            int dm = i_first == 1 ? 0 : p_addw(go, p_mulw(i_first - 2, ge));   // M[i_first-1][0]; M[0][0] = 0 (40)
            const int sm = G.match, sx = G.mismatch;
            int* rin_m = sh.ring_h[wave];
            int* rin_g = sh.ring_d[wave];
            int* rout_m = sh.ring_h[wave + 1];
            int* rout_g = sh.ring_d[wave + 1];
            int bm = 0, bg = 0, tch = 0, colm = 0, colg = 0;
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
                int topm = 0, topg = 0, tcv = 0;
                if (lane < CH && c0 < m) {
                    topm = rin_m[ring_slot(c0)];
                    topg = rin_g[ring_slot(c0)];
                    tcv = sh.text[c0 % kTRing];
                }
                lds_post(&sh.taken[wave], need);
                if (t0 >= 63 && t0 + CH < m) {   // every lane inside the matrix
#pragma unroll PWA_STEP_UNROLL
                    for (int q = 0; q < CH; ++q)
                        aff_step<RL, false>(t0 + q, lane, m, pc, hm, hx, dm, bm, bg, tch, topm, topg, tcv, colm, colg, sm, sx, go, ge);
                } else {
                    const int qn = min(CH, T - t0);
#pragma unroll 1
                    for (int q = 0; q < qn; ++q)
                        aff_step<RL, true>(t0 + q, lane, m, pc, hm, hx, dm, bm, bg, tch, topm, topg, tcv, colm, colg, sm, sx, go, ge);
#pragma unroll 1
                    for (int q = qn; q < CH; ++q) {   // keep the collectors aligned
                        colm = wave_shl1(bm, colm);
                        colg = wave_shl1(bg, colg);
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
                            rout_m[ring_slot(c)] = colm;
                            rout_g[ring_slot(c)] = colg;
                        }
                        lds_post(&sh.ready[wave + 1], (uint32_t)hi);
                    }
                }
            }
            if (failed && lane == 0) __hip_atomic_store((g_u32*)(G.queue + 1), 1u, PWA_RLX_AGENT);
            // M[n][m]: a lane's state froze when it left the matrix, so the lane that holds row n has its last column
#pragma unroll
            for (int r = 0; r < RL; ++r)
                if (i_first + r == n) {
                    ((PWA_GLOBAL PairResult*)P.res)->score = hm[r];
                    if (G.scores_out) ((g_i32*)G.scores_out)[P.out_index] = hm[r];
                }
        }
    }
}

}  // namespace pwa
