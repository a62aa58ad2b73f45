// gotoh_fill.hip.h -- affine-gap (Gotoh) NW / SW / semi-global alignments of many pairs with short patterns (gfx950 / MI355X):
// pwa_align_gotoh_batch and pwa_align_gotoh_batch_cigar (include/pwalign.h has the semantics, DESIGN.md §3.11 the figures).
//
// The mapping is the mini-stripe engine's (mini_fill.hip.h): a pair = one DPP row of LN = 16 lanes (four pairs per wave) or a whole
// wave (LN = 64, one pair per wave), lane k owns RL consecutive rows, the front is an anti-diagonal, the text symbol and the row above
// travel from lane k-1 to lane k by `row_shr:1` / `wave_shr:1`, tasks are dealt to the waves of four-wave workgroups, and the band is
// BandGeo<LN, RL> (one code byte per cell, written with the same coalesced stores).  What changes is the cell:
//   * a lane keeps, per row slot, H-left and E (registers); the row above brings H and F from lane k-1: two DPP moves per step;
//   * every value is a KEY  V * 8 + prio * 2 + x:  prio = the H tie-break priority of the value's source (the `max3` that picks H also
//     picks its direction), x = for E and F "this gap was opened here" (ties go to OPEN: the open candidate carries x = 1, the extend
//     candidate x = 0).  |V| < 2^28 (the host checks the range bound), so a key never wraps;
//   * there is no -inf: E[i][0] and F[0][j] are set to H + gap_open, whose extension ties the opening -- and a tie opens, which is
//     exactly what -inf gives, with every value inside the range;
//   * code byte: bit 0 = E opened here, bits 1-2 = H source (prio), bit 3 = F opened here.
// Scoring compares raw bytes (any alphabet, NUL and '-' included): one compare and one select per cell, no symbol table.
// SW keeps the first row-major maximum (mini_fill.hip.h's chunk-folded keys), SG the first maximum of row n (sg_track).  The fill
// writes score and end cell into PairResult; the walk starts from them.
#pragma once
#include "mini_fill.hip.h"

namespace pwa {

// H source priorities (larger wins a tie): NW, SG: diag > E ('I', left) > F ('D', up); SW: zero > diag > F > E
template <int MODE>
struct GotohPrio {
    static constexpr bool SW = MODE == 1;
    static constexpr int D = 2, E = SW ? 0 : 1, F = SW ? 1 : 0, Z = 3;
};

// code byte R of a dword <- c & 15 (one SDWA instruction; the first one of a dword zeroes the other bytes)
template <int R>
__device__ __forceinline__ void gotoh_put_code(uint32_t& codes, int c) {
    if (R == 0) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD" : "=v"(codes) : "v"(c), "v"(15));
    if (R == 1) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(codes) : "v"(c), "v"(15));
    if (R == 2) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(codes) : "v"(c), "v"(15));
    if (R == 3) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(codes) : "v"(c), "v"(15));
}

struct GotohConst {
    int cE, cF;     // H * 8 + cE: the E-open candidate of the cell to the right; H * 8 + cF: the F-open candidate of the cell below
    int ge8;        // extension step of a key
};

template <int MODE>
__device__ __forceinline__ GotohConst gotoh_const(const PairParams& G) {   // G.gap = gap_open, G.gap_extend = gap_extend
    typedef GotohPrio<MODE> PR;
    const int oe = p_addw(G.gap, G.gap_extend);
    GotohConst K;
    K.cE = p_addw(p_mulw(oe, 8), 2 * PR::E + 1);
    K.cF = p_addw(p_mulw(oe, 8), 2 * PR::F + 1);
    K.ge8 = p_mulw(G.gap_extend, 8);
    return K;
}

// The diagonal candidate is the one thing a scoring policy decides: diag (kept as H * 8 + cE) + Score::diag(...) is its key.  A policy
// holds its own state and has three hooks, which the chunk and the body call without knowing which policy they were given:
//   slot(byte, in)  per task and row slot: the slot's value from its pattern byte; in = the row is one of the pattern's (i <= n);
//   text(wv, k)     per chunk: lane k's travelling text value from its staged word wv (the lane's byte is byte k & 3 of it);
//   diag(tn, slot)  per cell: the key addend from the travelling text value and the slot value.
// This one compares raw bytes, splatted: match and mismatch as key addends.  subst_fill.hip.h has the table policy.
template <int MODE>
struct GotohByteScore {
    int sM, sX;
    __device__ __forceinline__ explicit GotohByteScore(const PairParams& G) {
        const int kadd = 2 * GotohPrio<MODE>::D - gotoh_const<MODE>(G).cE;
        sM = p_addw(p_mulw(G.match, 8), kadd);
        sX = p_addw(p_mulw(G.mismatch, 8), kadd);
    }
    __device__ __forceinline__ int slot(uint32_t byte, bool in) const { return in ? (int)(byte * 0x01010101u) : 0x100; }   // rows past n: never equal
    __device__ __forceinline__ int text(uint32_t wv, int k) const {
        const uint32_t bsel = (uint32_t)(k & 3) * 0x01010101u;
        return (int)__builtin_amdgcn_perm(wv, wv, bsel);
    }
    __device__ __forceinline__ int diag(int tn, int pc) const { return pc == tn ? sM : sX; }
};

// 16 steps of 64 / LN pairs.  GUARD: some lane is outside its matrix at some step of the chunk -- its state is frozen there.
// BAND = false: no code is built or stored (tba, tbb unused): the scores form.  rs: the policy's row-slot values; tch / tcv: its
// travelling text value.
template <int RL, int MODE, bool GUARD, int LN, bool BAND, class Score>
__device__ __forceinline__ void gotoh_chunk(const int t0, const int k, const int m, const int (&rs)[RL], int (&hl)[RL], int (&el)[RL], int& diag0,
                                            int& bot_h, int& bot_f, int& tch, const int tcv, const int top0, const int top_inc, const GotohConst& K,
                                            int (&bs)[RL], int (&bj)[RL], const int (&own)[RL], int& sg_v, int& sg_t, g_u8* const tba, g_u8* const tbb,
                                            const Score& sc) {
    typedef BandGeo<LN, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr int NQ = (RL + 3) / 4;
    constexpr bool SW = MODE == 1, SG = MODE == 2;
    int cmax[RL], kprev[RL];
    static_for<0, 16>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const int j = t0 + q - k + 1;
        const bool act = !GUARD || (unsigned)(j - 1) < (unsigned)m;
        const int tn = mini_row_shr1<LN>(mini_pick_lane0<q, LN>(tch, tcv), tch);   // this lane's text value
        // the row above: lane k-1's last row of the previous step; lane 0: row 0, H[0][j] and F[0][j] = H[0][j] + gap_open
        const int top_h = p_addw(top0, q * top_inc);
        const int uh_in = mini_row_shr1<LN>(top_h, bot_h);
        const int uf_in = mini_row_shr1<LN>(p_addw(top_h, -K.ge8 - 1), bot_f);
        int dg = diag0, uh = uh_in, uf = uf_in;
        uint32_t codes[NQ];
        int hst[RL];
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int kd = p_addw(dg, sc.diag(tn, rs[r]));
            const int e = max(hl[r], p_addw(el[r] & ~1, K.ge8));           // E: open (x = 1) wins a tie
            const int f = max(uh, p_addw(uf & ~1, K.ge8));                  // F: likewise
            int kk = max(max(kd, e), f);                                      // H and its source in one max3
            if (SW) kk = max(kk, 2 * PR::Z);                                  // the zero floor: key 0 * 8 + 2 * 3
            if constexpr (BAND) {
                const int c = (kk & 6) | (e & 1) | ((f & 1) << 3);
                if (r % 4 == 0) gotoh_put_code<0>(codes[r / 4], c);
                if (r % 4 == 1) gotoh_put_code<1>(codes[r / 4], c);
                if (r % 4 == 2) gotoh_put_code<2>(codes[r / 4], c);
                if (r % 4 == 3) gotoh_put_code<3>(codes[r / 4], c);
            }
            const int base = kk & ~7;                                         // H * 8
            const int hn = p_addw(base, K.cE);
            if (SW) {   // first maximum of the row, mini_fill.hip.h: keys H * 16 + 15 - q folded two steps at a time
                int key = (int)(((unsigned)base << 1) | (unsigned)(15 - q));
                if (GUARD) key = act ? key : 0;
                if (q % 2 == 0) kprev[r] = key;
                else {
                    cmax[r] = q == 1 ? max(kprev[r], key) : max(max(cmax[r], kprev[r]), key);
                    asm volatile("" : "+v"(cmax[r]));
                }
            }
            if (SG) hst[r] = hn;
            dg = hl[r];
            uh = p_addw(base, K.cF);
            uf = f;
            hl[r] = act ? hn : hl[r];
            el[r] = act ? e : el[r];
        }
        if constexpr (SG) sg_track<RL, GUARD>(hst, own, act, t0 + q, sg_v, sg_t);
        const int d0 = p_addw(uh_in, K.cE - K.cF);                           // H[i_first - 1][j] as the next step's diagonal
        diag0 = act ? d0 : diag0;
        bot_h = act ? uh : bot_h;
        bot_f = act ? uf : bot_f;
        tch = tn;
        if constexpr (BAND) {
            if constexpr (Geo::PA == 4) PWA_BAND_STORE((g_u32*)(tba + q * Geo::SR), codes[0]);
            if constexpr (Geo::PA == 8) PWA_BAND_STORE((PWA_GLOBAL mu32x2*)(tba + q * Geo::SR), (mu32x2{codes[0], codes[1]}));
            if constexpr (Geo::PA == 16) PWA_BAND_STORE((PWA_GLOBAL mu32x4*)(tba + q * Geo::SR), (mu32x4{codes[0], codes[1], codes[2], codes[3]}));
            if constexpr (Geo::PB == 2) PWA_BAND_STORE((PWA_GLOBAL uint16_t*)(tbb + q * Geo::SR), (uint16_t)codes[Geo::PA / 4]);
            if constexpr (Geo::PB == 4) PWA_BAND_STORE((g_u32*)(tbb + q * Geo::SR), codes[Geo::PA / 4]);
        }
    });
    if (SW) {
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const bool better = cmax[r] > (bs[r] | 15);   // strictly larger H: an earlier chunk keeps a tie
            bs[r] = better ? cmax[r] : bs[r];
            bj[r] = better ? t0 : bj[r];
        }
    }
}

// The fill (BAND) and its band-less scores form, under the scoring policy sc.  Workgroups of kMiniWaves waves, tasks (64 / LN pairs)
// dealt statically as in mini_fill_kernel; the host sorts the pairs by text length and pads the list to whole tasks with empty
// patterns.  Score and end cell go into PairResult (the walk starts from them).  BAND = false: no code byte is built or stored,
// PairDesc::tb is not read, and the score also goes into PairParams::scores_out at the pair's out_index.
template <int RL, int MODE, int LN, bool BAND, class Score>
__device__ __forceinline__ void gotoh_body(const PairParams& G, const Score& sc) {
    static_assert(LN == 16 || (LN == 64 && (RL == 8 || RL == 16)), "gotoh classes: 16 lanes x kMiniRL, or 64 lanes x 8 | 16 rows");
    typedef BandGeo<LN, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr int PPW = 64 / LN;
    constexpr bool NW = MODE == 0, SG = MODE == 2;
    const int lane = threadIdx.x & 63, k = lane & (LN - 1), grp = lane / LN;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int go = G.gap, ge = G.gap_extend;
    const GotohConst K = gotoh_const<MODE>(G);
    auto h0 = [&](int i) { return NW || SG ? (i ? p_addw(go, p_mulw(i, ge)) : 0) : 0; };   // H[i][0] (and H[0][j] for NW)
    for (uint32_t tid = blockIdx.x * kMiniWaves + wave; tid < G.n_tasks; tid += gridDim.x * kMiniWaves) {
        const PWA_GLOBAL PairDesc* const P = (const PWA_GLOBAL PairDesc*)(G.pairs + (size_t)tid * PPW + grp);
        const int n = P->n, m = P->m;
        g_cu8* const pat = (g_cu8*)P->pat;
        int mmax = m, mmin = m;
        if (PPW == 4) {
            mmax = max(m, __shfl_xor(m, 16));
            mmin = min(m, __shfl_xor(m, 16));
            mmax = max(mmax, __shfl_xor(mmax, 32));
            mmin = min(mmin, __shfl_xor(mmin, 32));
        }
        mmax = __builtin_amdgcn_readfirstlane(mmax);
        mmin = __builtin_amdgcn_readfirstlane(mmin);
        const int n_chunks = (mmax + (LN - 1) + 15) / 16;
        const int i_first = k * RL + 1;
        int rs[RL], hl[RL], el[RL], bs[RL], bj[RL];
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int i = i_first + r;
            rs[r] = sc.slot(i <= n ? pat[i - 1] : 0, i <= n);
            const int h = h0(i);
            hl[r] = p_addw(p_mulw(h, 8), K.cE);
            el[r] = p_addw(p_mulw(p_addw(h, go), 8), 2 * PR::E);                 // E[i][0] = H[i][0] + gap_open: its extension ties the opening
            bs[r] = 0;
            bj[r] = 0;
        }
        int diag0 = p_addw(p_mulw(h0(i_first - 1), 8), K.cE);   // H[i_first - 1][0]
        const int top_inc = NW ? K.ge8 : 0;
        int own[RL] = {};
        if (SG) sg_own(own, i_first, n);
        int sg_v = p_addw(p_mulw(h0(n), 8), K.cE), sg_t = k - 1;   // SG: the record starts at column 0
        g_u8* const tb = BAND ? (g_u8*)P->tb : nullptr;
        const int offa = k * Geo::PA, offb = LN * Geo::PA + k * Geo::PB;
        int bot_h = 0, bot_f = 0, tch = 0;
        // text staging with scalar loads, a chunk ahead (mini_fill_kernel: no vector load may sit among the band stores)
        const uint32_t* tg[PPW];
        int mg[PPW];
#pragma unroll
        for (int x = 0; x < PPW; ++x) {
            const uint64_t tp = (uint64_t)(uintptr_t)P->txt;
            const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)tp, LN * x), hi = __builtin_amdgcn_readlane((uint32_t)(tp >> 32), LN * x);
            tg[x] = (const uint32_t*)(uintptr_t)(((uint64_t)hi << 32) | lo);
            mg[x] = __builtin_amdgcn_readlane(m, LN * x);
        }
        auto stage = [&](int t0s, mu32x4 (&w)[PPW]) {
#pragma unroll
            for (int x = 0; x < PPW; ++x) {
                const int tc = min(t0s, (mg[x] + 15) & ~15);
                w[x] = *(const __attribute__((address_space(4))) mu32x4*)((uintptr_t)tg[x] + (size_t)tc);
            }
        };
        const int wsel = lane >> 2;
        mu32x4 wnext[PPW];
        stage(0, wnext);
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int t0 = ch * 16;
            uint32_t wv = wnext[0][0];
#pragma unroll
            for (int x = 1; x < 4 * PPW; ++x) wv = (wsel == x) ? wnext[x >> 2][x & 3] : wv;
            const int tcv = sc.text(wv, k);
            stage(t0 + 16, wnext);
            const int top0 = p_addw(p_mulw(h0(NW ? t0 + 1 : 0), 8), K.cF);   // H[0][t0 + 1] as an F-open candidate
            g_u8* const tbs = tb + (size_t)t0 * Geo::SR;
            const bool interior = t0 >= LN - 1 && t0 + 16 <= mmin;
            if (interior)
                gotoh_chunk<RL, MODE, false, LN, BAND>(t0, k, m, rs, hl, el, diag0, bot_h, bot_f, tch, tcv, top0, top_inc, K, bs, bj, own, sg_v, sg_t,
                                                       tbs + offa, tbs + offb, sc);
            else
                gotoh_chunk<RL, MODE, true, LN, BAND>(t0, k, m, rs, hl, el, diag0, bot_h, bot_f, tch, tcv, top0, top_inc, K, bs, bj, own, sg_v, sg_t,
                                                      tbs + offa, tbs + offb, sc);
        }
        PWA_GLOBAL PairResult* const res = (PWA_GLOBAL PairResult*)P->res;
        g_i32* const sco = BAND ? nullptr : (g_i32*)G.scores_out + P->out_index;
        if (SG) {
            if (n >= i_first && n < i_first + RL) {
                res->score = (int)((unsigned)sg_v - (unsigned)K.cE) >> 3;
                res->end_i = (uint32_t)n;
                res->end_j = (uint32_t)(sg_t - k + 1);
                if (!BAND) *sco = (int)((unsigned)sg_v - (unsigned)K.cE) >> 3;
            }
        } else if (NW) {
#pragma unroll
            for (int r = 0; r < RL; ++r)
                if (i_first + r == n) {   // the lane's state froze at column m
                    res->score = (int)((unsigned)hl[r] - (unsigned)K.cE) >> 3;
                    res->end_i = (uint32_t)n;
                    res->end_j = (uint32_t)m;
                    if (!BAND) *sco = (int)((unsigned)hl[r] - (unsigned)K.cE) >> 3;
                }
        } else {
            int s_best = 0, i_best = 0, j_best = 0;
#pragma unroll
            for (int r = 0; r < RL; ++r) {
                const int i = i_first + r, h = bs[r] >> 4;
                if (i <= n && h > s_best) {
                    s_best = h;
                    i_best = i;
                    j_best = bj[r] + (15 - (bs[r] & 15)) - k + 1;
                }
            }
#pragma unroll
            for (int off = LN / 2; off >= 1; off >>= 1) {
                const int so = __shfl_xor(s_best, off), io = __shfl_xor(i_best, off), jo = __shfl_xor(j_best, off);
                const bool better = so > s_best || (so == s_best && so > 0 && io < i_best);
                if (better) {
                    s_best = so;
                    i_best = io;
                    j_best = jo;
                }
            }
            if (k == 0 && n > 0) {   // (the padding pairs of the last task share a real pair's result slot)
                res->score = s_best;
                res->end_i = (uint32_t)i_best;
                res->end_j = (uint32_t)j_best;
                if (!BAND) *sco = s_best;
            }
        }
    }
}

// pwa_align_gotoh_batch's fill: G.match / G.mismatch on raw bytes
template <int RL, int MODE, int LN>
__global__ __launch_bounds__(64 * kMiniWaves) void gotoh_fill_kernel(const PairParams G) {
    gotoh_body<RL, MODE, LN, true>(G, GotohByteScore<MODE>(G));
}

// pwa_gotoh_batch_create's band-less form (scores, and end cells, without alignments); no walk follows
template <int RL, int MODE, int LN>
__global__ __launch_bounds__(64 * kMiniWaves) void gotoh_scores_kernel(const PairParams G) {
    gotoh_body<RL, MODE, LN, false>(G, GotohByteScore<MODE>(G));
}

// The classes the fills, the scores forms and the walks are built for: pick(StepIndex<RL>, StepIndex<LN>) for 16 lanes per pair and
// rl in kMiniRL or 64 lanes per pair and rl = 8 | 16, nullptr for anything else.
template <class Pick>
static auto gotoh_for_class(int rl, int ln, Pick pick) -> decltype(pick(StepIndex<8>{}, StepIndex<64>{})) {
    if (ln == 64) return rl == 8 ? pick(StepIndex<8>{}, StepIndex<64>{}) : rl == 16 ? pick(StepIndex<16>{}, StepIndex<64>{}) : nullptr;
    if (ln != 16) return nullptr;
    switch (rl) {
        case 4: return pick(StepIndex<4>{}, StepIndex<16>{});
        case 6: return pick(StepIndex<6>{}, StepIndex<16>{});
        case 8: return pick(StepIndex<8>{}, StepIndex<16>{});
        case 10: return pick(StepIndex<10>{}, StepIndex<16>{});
        case 12: return pick(StepIndex<12>{}, StepIndex<16>{});
        case 16: return pick(StepIndex<16>{}, StepIndex<16>{});
        default: return nullptr;
    }
}

// The walk: one wave per pair, a three-state machine (H, E, F) over the band, one op per iteration.  The band is staged into LDS in
// windows of WIN steps by LDS-DMA (pair_traceback_kernel's scheme): the window of the current cell and, in flight behind it, the one
// before (the walk only ever moves to earlier steps, at most two per op).  Ops are collected in a VGPR, one lane per op, and stored
// 64 at a time.
template <int RL, int MODE, int LN>
__global__ __launch_bounds__(64) void gotoh_walk_kernel(const PairParams G) {
    typedef BandGeo<LN, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr bool SW = MODE == 1, NW = MODE == 0;
    constexpr int SR = Geo::SR;
    constexpr int WIN = LN == 16 ? 32 : 16;
    constexpr int WB = WIN * SR;
    static_assert(WB % 1024 == 0 && WB <= 16384, "walk windows: whole KiB");
    __shared__ __attribute__((aligned(16))) uint8_t win[2 * WB];
    const int lane = threadIdx.x;
    const uint32_t pid = blockIdx.x;
    if (pid >= G.n_pairs) return;
    const PairDesc P = G.pairs[pid];
    g_cu8* const tb = (g_cu8*)P.tb;
    g_u8* const ops = (g_u8*)P.ops;
    PWA_GLOBAL PairResult* const res = (PWA_GLOBAL PairResult*)P.res;
    int i = __builtin_amdgcn_readfirstlane((int)res->end_i);
    int j = __builtin_amdgcn_readfirstlane((int)res->end_j);
    const uint32_t cap = P.ops_cap;
    auto issue = [&](int buf, int w) {   // window w (steps w WIN .. + WIN - 1) into LDS buffer buf: 1 KiB per instruction
        buf = __builtin_amdgcn_readfirstlane(buf);
        const size_t off0 = (size_t)w * WB;
#pragma unroll
        for (int u = 0; u < WB / 1024; ++u)
            __builtin_amdgcn_global_load_lds((const PWA_GLOBAL uint32_t*)(tb + off0 + (size_t)u * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) uint32_t*)(win + buf * WB + u * 1024), 16, 0, 0);
    };
    uint32_t cnt = 0, ob = 0;
    auto put = [&](uint32_t op) {   // (wave-uniform) op number cnt goes to lane cnt % 64; every 64th stores the batch
        const uint32_t slot = cnt & 63u;
        ob = (uint32_t)lane == slot ? op : ob;
        ++cnt;
        if (slot == 63u) ops[cnt - 64u + (uint32_t)lane] = (uint8_t)ob;
    };
    int st = 0;   // 0: H, 1: E, 2: F
    int cur_w = -1, pre_w = -1;
    bool fault = false;
    while (i > 0 && j > 0) {
        if (cnt >= cap) {   // cannot happen (every op moves i or j): never spin on the GPU
            fault = true;
            break;
        }
        const int q = i - 1, t = j - 1 + Geo::lane(q), w = t / WIN;
        if (w != cur_w) {
            if (w != pre_w) issue(w & 1, w);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // LDS-DMA is ordered for our ds_read by vmcnt
            cur_w = w;
            pre_w = -1;
            if (w > 0) {
                issue((w - 1) & 1, w - 1);
                pre_w = w - 1;
            }
        }
        const int c = __builtin_amdgcn_readfirstlane((int)win[(w & 1) * WB + (t - w * WIN) * SR + Geo::off(q)]);
        if (st == 0) {
            const int h = (c >> 1) & 3;
            if (SW && h == PR::Z) break;   // a zero cell
            if (h == PR::D) {
                put('M');
                --i;
                --j;
                continue;
            }
            st = h == PR::E ? 1 : 2;
        }
        if (st == 1) {
            put('I');
            st = (c & 1) ? 0 : 1;
            --j;
        } else {
            put('D');
            st = (c & 8) ? 0 : 2;
            --i;
        }
    }
    if ((uint32_t)lane < (cnt & 63u)) ops[(cnt & ~63u) + (uint32_t)lane] = (uint8_t)ob;   // the last partial batch
    if (!SW && !fault) {
        // column 0 is all 'D'; NW: row 0 all 'I'; SG: the walk ends where it meets row 0
        const uint32_t di = (uint32_t)i;
        if (cnt + di <= cap)
            for (uint32_t o = lane; o < di; o += 64) ops[cnt + o] = 'D';
        cnt += di;
        i = 0;
        if (NW) {
            const uint32_t dj = (uint32_t)j;
            if (cnt + dj <= cap)
                for (uint32_t o = lane; o < dj; o += 64) ops[cnt + o] = 'I';
            cnt += dj;
            j = 0;
        }
    }
    if (lane == 0) {
        res->start_i = (uint32_t)i;
        res->start_j = (uint32_t)j;
        res->n_ops = cnt;
        res->overflow = (cnt > cap || fault) ? 1u : 0u;
    }
}

}  // namespace pwa
