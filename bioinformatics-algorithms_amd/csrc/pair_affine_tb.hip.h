// pair_affine_tb.hip.h -- hw3's affine-gap ALIGNMENT of long pairs on the stripe engine (gfx950 / MI355X): fill with a traceback band,
// then a one-wave walk per pair.
//
// Replaces, per pair, the full affine_alignment(s1, s2, ..., &a1, &a2) of hw3/hw3.cpp:23-135 (the N-1 alignments against the center,
// 261-283) like batch_affine_tb.hip.h, but with the stripe engine's mapping: the skeleton of pair_affine.hip.h (stripes of 64 * RL
// rows, one wave per stripe sweeping anti-diagonals, the DPP row shift, the LDS ring, the helper wave for every HBM hand-off, (M, G)
// crossing rows, X and the previous column's M in registers) plus the band of pair_fill.hip.h (tb[stripe][step][lane][RL], one byte
// per cell, 64 RL contiguous bytes per wave and step, fire-and-forget stores).  Rows are string1 (i), columns string2 (j), so the
// reference's F (vertical, 'D') and E (horizontal, 'I') keep their names.
//
// Code byte of cell (i, j), the one batch_affine_tb.hip.h defines (strips and stripes share one code, one walk logic):
//   bits 1:0  A  = argmax of (V, F, E)[i][j] in the reference's order: V, then F if strictly greater, then E if strictly greater
//                  (hw3.cpp:59-68 read at the cell they index, 86-97 at (n, m)): 0 = V, 1 = F, 2 = E;  traceV[i][j] = A[i-1][j-1]
//   bit  2    xF = traceF[i][j]: F[i-1][j] + ge > V[i-1][j] + go + ge, strictly (70-75)
//   bit  3    xE = traceE[i][j]: E[i][j-1] + ge > V[i][j-1] + go + ge, strictly (77-82)
//
// Keyed values.  Every value travels as key = value * 4 + tag, so that one v_max3 / v_max picks the value AND the reference's choice:
//   kv = M4[i-1][j-1] + (4 s + 3)        V, tag 3            M4 = M * 4 (tag 0): the diagonal operand
//   kf = (G[i-1][j] | 3) + (4 ge - 1)    F, tag 2            G, X keys carry tag 2 (opened from V) or 1 (extended)
//   ke = (X[i][j-1] | 3) + (4 ge - 2)    E, tag 1
//   kM = max3(kv, kf, ke)                -> M * 4 + {3, 2, 1}: ties go to V, then F (the reference's order);  A = (kM & 3) ^ 3
//   kvo = kv + (4 go - 1)                V + go, tag 2
//   X = max(kvo, ke)                     tag 2 on a tie: opened, as the reference's strict '>' (77-82);  xE of (i, j+1) = X & 1
//   G = max(kvo, kf - 1)                 likewise (70-75);  xF of (i+1, j) = G & 1
// xF of a lane's first row thus crosses lanes inside G's low bits, with the same DPP shift, ring slot and HBM word that carry G.
//
// Range (the host's guard, pwalign_affine_tb.hip: (n + m + 2) * max(|match|, |mismatch|, |go| + |ge|) < 2^26).  Every real value (a path's score,
// + go once for G / X) is then inside +-2^26, its key inside +-2^28.  The sentinel key kAffTbNeg = -2^30 (value -2^28) enters only as
// G[0][j] and X[i][0]; one + 4 ge later it is beaten by a real value (kvo), so no key leaves (-2^30 - 2^28, 2^28): no int32 wraps, and a
// sentinel-derived candidate never wins a max against a real one, exactly as the reference's INT_MIN/2 never does inside the same range.
//
// Which cells differ from the reference, and why no walk visits them.  Row 0 and column 0 are not in the band: the walk treats them
// analytically (A = V at (0, 0), E on row 0, F on column 0; traceF[i][0] / traceE[0][j] extend except at 1), as affine_walk_kernel does.
// V, and A, of every interior cell are the reference's: V is a real path value from (1, 1) on, and F[1][j] / E[i][1] -- the only
// interior values derived from a sentinel, here and in the reference -- lose to it in both.  So do xF of rows >= 2 and xE of columns >= 2.
// xF of row 1 and xE of column 1 compare two sentinel-derived values: the reference's answer is "go < 0", ours is 0.  A walk reaches
// state F at (1, j) only through A[1][j] = F (needs F[1][j] > V[1][j]), xF[2][j] = 1 (needs F[1][j] > V[1][j] + go) or a final state F
// at (1, m) -- all three impossible while the guard holds -- and state E at (i, 1) likewise: those bits are never read.
#pragma once
#include "pair_affine.hip.h"

namespace pwa {

constexpr int kAffTbNeg = -(1 << 30);   // sentinel KEY (value -2^28)

// One anti-diagonal step of a stripe with codes.  EDGE: some lanes of this step lie outside the matrix (their state stays frozen).
//   hm: M4 of the lane's rows at the previous column;  hx: X keys;  dm: M4 of the row above row 0 at the previous column;
//   bm, bg: (M4, G key) of the lane's bottom row;  top*, tcv: the staged row above the stripe and the text, rotated one lane per step;
//   colm, colg: the bottom row of lane 63, collected for the ring;  kmx / kmm: 4 s + 3 for a match / mismatch;  kgo = 4 go - 1,
//   kf0 = 4 ge - 1, ke0 = 4 ge - 2
template <int RL, bool EDGE>
__device__ __forceinline__ void aff_tb_step(int t, int lane, int m, const int (&pc)[RL], int (&hm)[RL], int (&hx)[RL], int& dm, int& bm,
                                            int& bg, int& tch, int& topm, int& topg, int& tcv, int& colm, int& colg, int kmm, int kmx,
                                            int kgo, int kf0, int ke0, g_u8* tbs) {
    const int up_m = wave_shr1(topm, bm);   // (M4, G)[i_first-1][j]; lane 0: the staged row above the stripe
    const int up_g = wave_shr1(topg, bg);
    tch = wave_shr1(tcv, tch);              // text symbol of column c; lane 0: the staged text
    topm = wave_shl1(topm, topm);           // rotate the staged vectors: lane 0 sees the next column next step
    topg = wave_shl1(topg, topg);
    tcv = wave_shl1(tcv, tcv);
    const int c = t - lane;
    uint32_t codes = 0;
    if (!EDGE || (c >= 0 && c < m)) {
        int dg = dm, ug = up_g;
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int kv = p_addw(dg, pc[r] == tch ? kmm : kmx);   // hw3.cpp:57-68
            const int kf = p_addw(ug | 3, kf0);                    //         70-75
            const int ke = p_addw(hx[r] | 3, ke0);                 //         77-82
            const int km = max(kv, max(kf, ke));
            const int kvo = p_addw(kv, kgo);
            const uint32_t code = (uint32_t)((km & 3) ^ 3) | ((uint32_t)(ug & 1) << 2) | ((uint32_t)(hx[r] & 1) << 3);
            codes |= code << (8 * r);
            dg = hm[r];
            hm[r] = km & ~3;
            hx[r] = max(kvo, ke);
            ug = max(kvo, kf - 1);
        }
        dm = up_m;
        bm = hm[RL - 1];
        bg = ug;
    }
    colm = wave_shl1(bm, colm);   // lane 63 inserts its bottom-row values (column t-63), the rest shifts down
    colg = wave_shl1(bg, colg);
    if (RL == 4) {
        ((g_u32*)tbs)[(size_t)t * 64 + lane] = codes;
    } else {
        static_assert(RL == 2 || RL == 4, "RL");
        ((PWA_GLOBAL uint16_t*)tbs)[(size_t)t * 64 + lane] = (uint16_t)codes;
    }
}

template <int RL, int W>
__global__ __launch_bounds__(64 * (W + 1)) void pair_affine_tb_kernel(const PairParams G) {
    constexpr int CH = kCH;
    __shared__ DistShared<W> sh;   // ring_h: M4, ring_d: G keys
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
            // =================== helper wave: every global-memory hand-off of this workgroup (as in pair_affine_kernel) ===================
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
                                else v[u] = dist_pack(p_mulw(p_addw(go, p_mulw(c, ge)), 4), kAffTbNeg + 2);   // (M4, G)[0][c+1], hw3.cpp:48-53
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
                pc[r] = (i <= n) ? (int)((g_cu8*)P.pat)[i - 1] : 256;        // 256 never equals a text symbol
                hm[r] = p_mulw(p_addw(go, p_mulw(i - 1, ge)), 4);           // M[i][0] = F[i][0], hw3.cpp:42-47
                hx[r] = kAffTbNeg + 2;                                       // X[i][0]: V, E = -inf
            }
            int dm = i_first == 1 ? 0 : p_mulw(p_addw(go, p_mulw(i_first - 2, ge)), 4);   // M4[i_first-1][0]; M[0][0] = 0 (40)
            const int kmm = p_addw(p_mulw(G.match, 4), 3), kmx = p_addw(p_mulw(G.mismatch, 4), 3);
            const int kgo = p_addw(p_mulw(go, 4), -1), kf0 = p_addw(p_mulw(ge, 4), -1), ke0 = p_addw(p_mulw(ge, 4), -2);
            g_u8* tbs = (g_u8*)(P.tb + (size_t)s * band_steps((size_t)m) * 64 * RL);
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
                        aff_tb_step<RL, false>(t0 + q, lane, m, pc, hm, hx, dm, bm, bg, tch, topm, topg, tcv, colm, colg, kmm, kmx, kgo, kf0, ke0, tbs);
                } else {   // (a chunk always ends inside band_steps(m): the whole chunk is stored, padding included)
#pragma unroll 1
                    for (int q = 0; q < CH; ++q)
                        aff_tb_step<RL, true>(t0 + q, lane, m, pc, hm, hx, dm, bm, bg, tch, topm, topg, tcv, colm, colg, kmm, kmx, kgo, kf0, ke0, tbs);
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
                    ((PWA_GLOBAL PairResult*)P.res)->score = hm[r] >> 2;
                    if (G.scores_out) ((g_i32*)G.scores_out)[P.out_index] = hm[r] >> 2;
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The walk (hw3.cpp:103-131), one wave per pair, over the skewed band: three states, 'M' / 'D' / 'I' in traceback order into
// P.ops, the count into P.res->n_ops.  Band windows as pair_traceback_kernel's (BandGeo<64, RL>): WIN-step windows staged into LDS
// by LDS-DMA, window w of the anchor's stripe in buffer w & 1, the window before it in flight and readable once it has landed.
// One trip = one LDS round trip over 64 cells of one line through the anchor:
//   state V at (i, j): lane d reads A(i-1-d, j-1-d): the leading run of A = V is a run of 'M' (107-112), the first other code the
//                      state after it;
//   state F at (i, j): lane d reads xF(i-d, j): the leading run of set bits is a run of 'D' (113-121), then state V;
//   state E at (i, j): lane d reads xE(i, j-d): 'I' (122-130) likewise.
// A cell outside the staged windows (or the matrix) ends the run before it: the next trip stages its window.
template <int RL>
__global__ __launch_bounds__(64) void pair_affine_walk_kernel(const PairParams G) {
    typedef BandGeo<64, RL> Geo;
    constexpr int WIN = 64, SR = Geo::SR, WB = WIN * SR;   // 16 KiB windows for RL = 4
    static_assert(WB % 4096 == 0, "whole 4 KiB pieces per window");
    constexpr int NOCODE = 0xff;
    __shared__ __attribute__((aligned(16))) uint8_t win[2 * WB];
    const int lane = threadIdx.x;
    const uint32_t pid = blockIdx.x;
    if (pid >= G.n_pairs) return;
    const PairDesc P = G.pairs[pid];
    const int n = P.n, m = P.m;
    const size_t T = band_steps((size_t)m);
    g_cu8* tb = (g_cu8*)P.tb;
    g_u8* ops = (g_u8*)P.ops;
    PWA_GLOBAL PairResult* res = (PWA_GLOBAL PairResult*)P.res;

    auto issue = [&](int s, int w) {   // LDS-DMA of window w of stripe s into buffer w & 1: 1 KiB per instruction
        const size_t off0 = ((size_t)s * T + (size_t)w * WIN) * SR;
        const int buf = __builtin_amdgcn_readfirstlane(w & 1);
#pragma unroll
        for (int u = 0; u < WB / 4096; ++u) {
            const PWA_GLOBAL uint32_t* g = (const PWA_GLOBAL uint32_t*)(tb + off0 + (size_t)u * 4096 + lane * 16);
            __attribute__((address_space(3))) uint32_t* l = (__attribute__((address_space(3))) uint32_t*)(win + buf * WB + u * 4096);
            __builtin_amdgcn_global_load_lds(g, l, 16, 0, PWA_WALK_LOAD_AUX);
            __builtin_amdgcn_global_load_lds(g, l, 16, 1024, PWA_WALK_LOAD_AUX);
            __builtin_amdgcn_global_load_lds(g, l, 16, 2048, PWA_WALK_LOAD_AUX);
            __builtin_amdgcn_global_load_lds(g, l, 16, 3072, PWA_WALK_LOAD_AUX);
        }
    };
    int cur_s = -1, cur_w = -1, pre_s = -1, pre_w = -1, since = 0;
    bool pre_done = false;
    auto stage = [&](int ci, int cj) {   // make sure the window holding interior cell (ci, cj) is staged (wave-uniform)
        const unsigned q0 = (unsigned)(ci - 1);
        const int s0 = Geo::stripe(q0), k0 = Geo::lane(Geo::row_in_stripe(q0));
        const int w0 = (cj - 1 + k0) / WIN;
        if (s0 != cur_s || w0 != cur_w) {
            const bool have = s0 == pre_s && w0 == pre_w;   // the window already in flight / landed
            if (!have && pre_s >= 0 && !pre_done) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (it may target the same buffer)
            if (!have) issue(s0, w0);
            if (!(have && pre_done)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // LDS-DMA is ordered for our ds_read by vmcnt
            cur_s = s0;
            cur_w = w0;
            pre_s = -1;
            pre_done = false;
            since = 0;
            if (w0 > 0) {   // the walk only moves backwards
                issue(s0, w0 - 1);
                pre_s = s0;
                pre_w = w0 - 1;
            }
        } else if (pre_s >= 0 && !pre_done && ++since >= 3) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            pre_done = true;
        }
    };
    auto code_at = [&](int ci, int cj) -> int {   // code byte of interior cell (ci, cj) if staged, else NOCODE
        if (ci < 1 || cj < 1) return NOCODE;
        const unsigned q = (unsigned)(ci - 1);
        const int ql = Geo::row_in_stripe(q);
        const int t = cj - 1 + Geo::lane(ql);
        const int tlo = (pre_done ? cur_w - 1 : cur_w) * WIN;
        if (Geo::stripe(q) != cur_s || (unsigned)(t - tlo) >= (unsigned)((cur_w + 1) * WIN - tlo)) return NOCODE;
        return win[(t & (2 * WIN - 1)) * SR + Geo::off(ql)];
    };

    uint32_t cnt = 0;
    int i = n, j = m, state;
    stage(i, j);
    state = __builtin_amdgcn_readfirstlane(code_at(i, j)) & 3;   // hw3.cpp:86-97
    bool fault = false;
    while (i > 0 && j > 0) {
        int k = 0, next = state;   // ops of this trip, the state after them
        if (state == 0) {
            if (i == 1 || j == 1) {   // (i-1, j-1) is on row / column 0: A there is V at (0, 0), E on row 0, F on column 0 (40-53)
                k = 1;
                next = (i == 1 && j == 1) ? 0 : (i == 1 ? 2 : 1);
            } else {
                stage(i - 1, j - 1);
                const int ci = i - 1 - lane, cj = j - 1 - lane;
                int a = NOCODE;
                if (ci >= 1 && cj >= 1) {
                    const int c = code_at(ci, cj);
                    a = c == NOCODE ? NOCODE : (c & 3);
                } else if (ci >= 0 && cj >= 0) {
                    a = (ci == 0 && cj == 0) ? 0 : (ci == 0 ? 2 : 1);
                }
                const unsigned long long vm = __ballot(a == 0);
                const int L = (~vm == 0ull) ? 64 : __builtin_ctzll(~vm);
                const int aL = L < 64 ? __builtin_amdgcn_readlane(a, L) : NOCODE;
                if (aL != NOCODE) {   // M at (i - d, j - d) for d = 0 .. L, then state aL
                    k = L + 1;
                    next = aL;
                } else {              // the run leaves the staged cells: M for d = 0 .. L-1, still in state V
                    k = L;
                    next = 0;
                }
            }
            if (lane < k) ops[cnt + lane] = 'M';
            i -= k;
            j -= k;
        } else {
            const bool vert = state == 1;   // F: up the column ('D'), E: left along the row ('I')
            stage(i, j);
            const int c = vert ? code_at(i - lane, j) : code_at(i, j - lane);
            const int x = c == NOCODE ? NOCODE : ((c >> (vert ? 2 : 3)) & 1);
            const unsigned long long xm = __ballot(x == 1);
            const int R = (~xm == 0ull) ? 64 : __builtin_ctzll(~xm);
            const int xR = R < 64 ? __builtin_amdgcn_readlane(x, R) : NOCODE;
            if (xR != NOCODE) {   // a gap op at every cell d = 0 .. R; the last one was opened from V
                k = R + 1;
                next = 0;
            } else {
                k = R;
                next = state;
            }
            if (lane < k) ops[cnt + lane] = vert ? 'D' : 'I';
            i -= vert ? k : 0;
            j -= vert ? 0 : k;
        }
        if (k == 0) {   // cannot happen (the trip's first cell is staged): never spin on the GPU
            fault = true;
            break;
        }
        cnt += (uint32_t)k;
        state = next;
    }
    // row 0 / column 0 (hw3.cpp:113-130 with traceF[i][0] / traceE[0][j]): state F down column 0, state E along row 0
    for (int o = lane; o < i; o += 64) ops[cnt + o] = 'D';
    cnt += (uint32_t)i;
    for (int o = lane; o < j; o += 64) ops[cnt + o] = 'I';
    cnt += (uint32_t)j;
    if (lane == 0) {
        res->n_ops = cnt;
        res->overflow = (cnt > P.ops_cap || fault) ? 1u : 0u;
    }
}

}  // namespace pwa
