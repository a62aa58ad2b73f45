// subst_fill.hip.h -- affine-gap (gotoh) NW / SW / semi-global alignments and scores of many pairs under a caller-supplied
// substitution matrix (gfx950 / MI355X): pwa_align_subst_batch(_cigar), pwa_subst_batch_create, pwa_scores_subst (include/pwalign.h
// has the semantics, DESIGN.md §3.13 the figures).
//
// Everything but the diagonal candidate is gotoh_fill.hip.h's: the mini-stripe mapping (LN = 16 lanes per pair and four pairs per wave,
// or LN = 64 and one pair per wave; RL rows per lane), the keyed E / F / H cells with their tie-breaks, the code byte, BandGeo<LN, RL>,
// the SW first-maximum keys, sg_track, PairResult -- and the walk, which is gotoh_walk_kernel itself (the code byte is the same).
// The cell's score:
//   * the workgroup first loads the table into LDS, prescaled into key form:  tab[ct * stride + cp] = s(cp, ct) * 8 + 2 * PR::D - K.cE
//     (ct = text code picks the ROW, cp = pattern code the column; stride is the host's: odd below 32 symbols, so that the rows of a
//     small alphabet start in different banks), and the 256-byte map from byte value to code;
//   * the arena stays raw bytes (the walk and the CIGAR / MD:Z passes read them).  A lane turns its RL pattern bytes into byte offsets
//     cp * 4 once per task, and its staged text byte into the row's byte offset ct * stride * 4 once per 16-step chunk; that offset,
//     not the byte, then travels from lane k-1 to lane k with the DPP moves the text symbol used to take;
//   * per cell: one add (row offset + column offset) and one ds_read_b32 give the key addend, in place of a compare and a select.
// Rows past n use code 0: their values feed only rows below them and are kept out of every record by the `i <= n` / `own` tests.
// No vector global load sits among the band stores (mini_fill_kernel): the text is staged with scalar loads, the table is in LDS.
#pragma once
#include "gotoh_fill.hip.h"
#include "subst_table.h"

namespace pwa {

struct SubstLds {
    int tab[kSubstTabWords];
    uint32_t map[kSubstMapWords];
};

// 16 steps of 64 / LN pairs: gotoh_chunk with the table lookup.  tch / tcv carry row byte offsets into L.tab, po[r] column byte offsets.
template <int RL, int MODE, bool GUARD, int LN, bool BAND>
__device__ __forceinline__ void subst_chunk(const int t0, const int k, const int m, const int (&po)[RL], int (&hl)[RL], int (&el)[RL], int& diag0,
                                            int& bot_h, int& bot_f, int& tch, const int tcv, const int top0, const int top_inc, const GotohConst& K,
                                            int (&bs)[RL], int (&bj)[RL], const int (&own)[RL], int& sg_v, int& sg_t, g_u8* const tba, g_u8* const tbb,
                                            const SubstLds& L) {
    typedef BandGeo<LN, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr int NQ = (RL + 3) / 4;
    constexpr bool SW = MODE == 1, SG = MODE == 2;
    int cmax[RL], kprev[RL];
    static_for<0, 16>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const int j = t0 + q - k + 1;
        const bool act = !GUARD || (unsigned)(j - 1) < (unsigned)m;
        const int tn = mini_row_shr1<LN>(mini_pick_lane0<q, LN>(tch, tcv), tch);   // this lane's text symbol, as its row's byte offset
        const char* const row = reinterpret_cast<const char*>(L.tab) + tn;
        const int top_h = p_addw(top0, q * top_inc);
        const int uh_in = mini_row_shr1<LN>(top_h, bot_h);
        const int uf_in = mini_row_shr1<LN>(p_addw(top_h, -K.ge8 - 1), bot_f);
        int dg = diag0, uh = uh_in, uf = uf_in;
        uint32_t codes[NQ];
        int hst[RL];
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int kd = p_addw(dg, *reinterpret_cast<const int*>(row + po[r]));   // diag + s(cp, ct), as a key
            const int e = max(hl[r], p_addw(el[r] & ~1, K.ge8));           // E: open (x = 1) wins a tie
            const int f = max(uh, p_addw(uf & ~1, K.ge8));                  // F: likewise
            int kk = max(max(kd, e), f);                                      // H and its source in one max3
            if (SW) kk = max(kk, 2 * PR::Z);                                  // the zero floor: key 0 * 8 + 2 * 3
            const int base = kk & ~7;                                         // H * 8
            if constexpr (BAND) {
                const int c = (kk & 6) | (e & 1) | ((f & 1) << 3);
                if (r % 4 == 0) gotoh_put_code<0>(codes[r / 4], c);
                if (r % 4 == 1) gotoh_put_code<1>(codes[r / 4], c);
                if (r % 4 == 2) gotoh_put_code<2>(codes[r / 4], c);
                if (r % 4 == 3) gotoh_put_code<3>(codes[r / 4], c);
            }
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

// The fill (BAND) and its band-less scores form: G.gap = gap_open, G.gap_extend = gap_extend, G.match / G.mismatch unused.
// blob: kSubstMapWords words of code map, then n_sym rows of `stride` raw scores, row = text code.  Tasks are dealt as in
// gotoh_fill_kernel; BAND = false also writes the score into G.scores_out at the pair's out_index (gotoh_scores_kernel).
template <int RL, int MODE, int LN, bool BAND>
__device__ __forceinline__ void subst_body(const PairParams& G, const uint32_t* const blob, const int n_sym, const int stride, SubstLds& L) {
    static_assert(LN == 16 || (LN == 64 && (RL == 8 || RL == 16)), "gotoh classes: 16 lanes x kMiniRL, or 64 lanes x 8 | 16 rows");
    typedef BandGeo<LN, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr int PPW = 64 / LN;
    constexpr bool NW = MODE == 0, SG = MODE == 2;
    const int lane = threadIdx.x & 63, k = lane & (LN - 1), grp = lane / LN;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int go = G.gap, ge = G.gap_extend, oe = p_addw(go, ge);
    GotohConst K;
    K.cE = p_addw(p_mulw(oe, 8), 2 * PR::E + 1);
    K.cF = p_addw(p_mulw(oe, 8), 2 * PR::F + 1);
    K.sM = K.sX = 0;
    K.ge8 = p_mulw(ge, 8);
    // the table and the code map into LDS, once per workgroup (a code past the alphabet cannot come from the host: clamped all the same)
    {
        const int words = min(n_sym * stride, kSubstTabWords), kadd = 2 * PR::D - K.cE;
        for (int x = (int)threadIdx.x; x < words; x += 64 * kMiniWaves) L.tab[x] = p_addw(p_mulw((int)blob[kSubstMapWords + x], 8), kadd);
        if (threadIdx.x < (unsigned)kSubstMapWords) L.map[threadIdx.x] = blob[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* const map = reinterpret_cast<const uint8_t*>(L.map);
    const int code_max = n_sym - 1, row_bytes = stride * 4;
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
        int po[RL], hl[RL], el[RL], bs[RL], bj[RL];
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const int i = i_first + r;
            po[r] = i <= n ? min((int)map[pat[i - 1]], code_max) * 4 : 0;   // the row's column in the table; rows past n: code 0
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
        const int bshift = (k & 3) * 8;
        const int wsel = lane >> 2;
        mu32x4 wnext[PPW];
        stage(0, wnext);
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int t0 = ch * 16;
            uint32_t wv = wnext[0][0];
#pragma unroll
            for (int x = 1; x < 4 * PPW; ++x) wv = (wsel == x) ? wnext[x >> 2][x & 3] : wv;
            // the lane's staged text byte -> its code -> the byte offset of that code's table row
            const int tcv = min((int)map[(wv >> bshift) & 0xffu], code_max) * row_bytes;
            stage(t0 + 16, wnext);
            const int top0 = p_addw(p_mulw(h0(NW ? t0 + 1 : 0), 8), K.cF);   // H[0][t0 + 1] as an F-open candidate
            g_u8* const tbs = tb + (size_t)t0 * Geo::SR;
            const bool interior = t0 >= LN - 1 && t0 + 16 <= mmin;
            if (interior)
                subst_chunk<RL, MODE, false, LN, BAND>(t0, k, m, po, hl, el, diag0, bot_h, bot_f, tch, tcv, top0, top_inc, K, bs, bj, own, sg_v, sg_t,
                                                       tbs + offa, tbs + offb, L);
            else
                subst_chunk<RL, MODE, true, LN, BAND>(t0, k, m, po, hl, el, diag0, bot_h, bot_f, tch, tcv, top0, top_inc, K, bs, bj, own, sg_v, sg_t,
                                                      tbs + offa, tbs + offb, L);
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

template <int RL, int MODE, int LN>
__global__ __launch_bounds__(64 * kMiniWaves) void subst_fill_kernel(const PairParams G, const uint32_t* blob, int n_sym, int stride) {
    __shared__ SubstLds L;
    subst_body<RL, MODE, LN, true>(G, blob, n_sym, stride, L);
}

template <int RL, int MODE, int LN>
__global__ __launch_bounds__(64 * kMiniWaves) void subst_scores_kernel(const PairParams G, const uint32_t* blob, int n_sym, int stride) {
    __shared__ SubstLds L;
    subst_body<RL, MODE, LN, false>(G, blob, n_sym, stride, L);
}

}  // namespace pwa
