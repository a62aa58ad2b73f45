// banded_scores.hip.h -- the scores-only form of the banded affine-gap fill (gfx950 / MI355X): pwa_scores_banded (include/pwalign.h has
// the semantics, DESIGN.md §3.14 the figures).  Score and end cell of every pair, no traceback band, no walk.
//
// Geometry and host-visible behaviour are banded_fill.hip.h's, unchanged: one wave per pair, kBandedWaves per workgroup, static
// dealing, stripes of S = 64 RL rows, the column window [c0a, c1] per stripe (banded_c0a / banded_chunks), scalar text staging a chunk
// ahead, the (H, F) hand-off row in LDS, edge and interior chunk forms, PairDesc::pad[0 / 1] = the clamped band, results in PairResult.
// PairDesc::tb, ops and row_stride are not read.  What differs is the cell.  It builds no code byte and stores nothing, so nothing has
// to remember where a value came from: every value is the plain int32 score, not a key with a priority and open / extend flags in its
// low bits.  That drops the `& ~1` on E and F, the `& ~7` that recovers the base, the code-byte construction (gotoh_put_code, four
// SDWA writes per dword), and one of the two re-biased adds: H + (gap_open + gap_extend) is at once the E-open candidate of the cell to
// the right and the F-open candidate of the cell below.  With oe = gap_open + gap_extend, ge = gap_extend, per cell:
//     e = max(hl, el + ge)      hl = H[i][j-1] + oe, el = E[i][j-1]
//     f = max(uh, uf + ge)      uh = H[i-1][j] + oe, uf = F[i-1][j]
//     h = max3(dg + s, e, f)    dg = H[i-1][j-1] + oe (the row slot above's hl, a step old), s = match | mismatch - oe;  SW: and 0
//     hn = h + oe               handed right (hl), down (uh) and, a step later, diagonally (dg)
// The mask is the fill's, word for word: a row's in-band columns are contiguous; a row slot's state (hl, el) starts as the sentinel, or
// as the column-0 boundary where that lies in the band, and is written only by in-band cells; what an out-of-band cell hands down (uh,
// uf) is FORCED to the sentinel at every step, never carried and extended.  So E of a row's first in-band cell, F of a column's first
// in-band cell and anything read across the band edge are the sentinel itself, and the diagonal neighbour of an in-band cell is always
// in the band.
// Why no used sum leaves int32.  A = max(|match|, |mismatch|, |gap_open| + |gap_extend|, 1); the host admits a pair only while
// (n + m + 2) A < 2^28.  A real value V (an H, E or F that stands for a path inside the band) has |V| <= (n + m) A, and the sums formed
// from real values -- V + oe, V + ge, (V + oe) + (match - oe) -- stay within (n + m + 2) A < 2^28.  The sentinel is the plain value
// kBandedSent = -2^30: below every real value and every real value + oe.  hl, el, uh and uf are each a real sum or exactly the sentinel
// (an in-band e is >= hl, an in-band f is >= uh, and what is handed on is one of those or the forced constant), so the only sums a
// sentinel enters where the result is used are el + ge and uf + ge >= -2^30 - A: inside int32, and never above the sentinel, so they
// lose against it or against a real value and are dropped -- a sentinel is not extended twice.  dg of an in-band cell is real (its
// diagonal neighbour is in the band), and every in-band cell of a valid band is reachable from the boundary inside the band, so its H
// is real.  Sums of out-of-band cells may be anything (p_addw wraps without UB); the mask discards them.
// The end-cell records never looked at priority bits and are kept with their tie behaviour: SW the folded (H << 4 | 15 - q) keys per
// row and chunk (first maximum of a row), one (H, i, j) record per lane across stripes replaced on a strictly larger H only, the
// (H desc, i asc) reduction; SG the first maximum of row n over its in-band columns (sg_track's pick); NW the state of row n frozen
// at column m.  SW's H << 4 fits: H <= min(n, m) match < 2^27 under the range rule.
// The EXT form (MODE = kBandedExt; pwa_scores_extend_banded) is banded_fill.hip.h's: NW's boundaries and tie order, the row keys over
// signed H with kBandedExtNone for "no in-band cell", banded_ext_stripe_end at the end of every stripe.  Its H << 4 holds a negative H
// because the host admits an EXT pair only while (n + m + 2) A < 2^27: |H| <= (n + m) A < 2^27, so H * 16 + 0..15 stays inside int32
// and above kBandedExtNone.
#pragma once
#include "banded_fill.hip.h"

namespace pwa {

constexpr int kBandedSent = -(1 << 30);

// GotohByteScore's hooks (raw bytes, splatted and compared) with the diagonal addends as plain values: match | mismatch - oe
struct BandedValueScore : GotohByteScore<0> {
    __device__ __forceinline__ explicit BandedValueScore(const PairParams& G) : GotohByteScore<0>(G) {
        const int oe = p_addw(G.gap, G.gap_extend);
        sM = p_addw(G.match, -oe);
        sX = p_addw(G.mismatch, -oe);
    }
};

// 16 steps of one stripe: banded_chunk's arguments and masks, the value cell, no store.  hl, el, uh, uf, diag0 as in the header comment.
template <int RL, int MODE, bool EDGE, class Score>
__device__ __forceinline__ void banded_scores_chunk(const int t0, const int k, const int jm, const int m, const int xb, const unsigned B, const int (&rs)[RL],
                                                    int (&hl)[RL], int (&el)[RL], int& diag0, int& bot_h, int& bot_f, int& tch, const int tcv,
                                                    const int thv, const int tfv, const int oe, const int ge, int (&bs)[RL], int (&bj)[RL],
                                                    const int (&own)[RL], int& sg_v, int& sg_t, lds_bint2* const row, const Score& sc) {
    constexpr bool SW = MODE == 1, SG = MODE == 2, EXT = MODE == kBandedExt;
    constexpr int SENT = kBandedSent;
    int cmax[RL], kprev[RL];
    static_for<0, 16>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const int x = xb + q;
        const bool started = !EDGE || t0 + q >= k;
        const bool actl = !EDGE || (started && jm + q <= m);
        const int tn = mini_row_shr1<64>(mini_pick_lane0<q, 64>(tch, tcv), tch);
        // the row above: lane k-1's last row of the previous step; lane 0: the hand-off entry of this step's column
        const int uh_in = mini_row_shr1<64>(mini_pick_lane0<q, 64>(thv, thv), bot_h);
        const int uf_in = mini_row_shr1<64>(mini_pick_lane0<q, 64>(tfv, tfv), bot_f);
        int dg = diag0, uh = uh_in, uf = uf_in;
        int hst[RL];
        bool a = false;
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            a = actl && (unsigned)(x - r) < B;                                 // the cell is in the band (and in the matrix)
            const int e = max(hl[r], p_addw(el[r], ge));
            const int f = max(uh, p_addw(uf, ge));
            int h = max(max(p_addw(dg, sc.diag(tn, rs[r])), e), f);
            if (SW) h = max(h, 0);
            const int hn = p_addw(h, oe);
            if (SW || EXT) {   // first maximum of the row over in-band cells (gotoh_chunk's folded keys; EXT: H of either sign)
                int key = (int)(((unsigned)h << 4) | (unsigned)(15 - q));
                key = a ? key : EXT ? kBandedExtNone : 0;
                if (q % 2 == 0) kprev[r] = key;
                else {
                    cmax[r] = q == 1 ? max(kprev[r], key) : max(max(cmax[r], kprev[r]), key);
                    asm volatile("" : "+v"(cmax[r]));
                }
            }
            if (SG) hst[r] = a ? hn : (int)0x80000000;
            dg = hl[r];
            uh = a ? hn : SENT;                                                // out of band: forced, never carried
            uf = a ? f : SENT;
            hl[r] = a ? hn : hl[r];
            el[r] = a ? e : el[r];
        }
        if constexpr (SG) {
            int v = hst[0] & own[0];
#pragma unroll
            for (int r = 1; r < RL; ++r) v |= hst[r] & own[r];
            const bool better = v > sg_v;
            sg_v = better ? v : sg_v;
            sg_t = better ? t0 + q : sg_t;
        }
        diag0 = started ? uh_in : diag0;                                       // H[i_first - 1][j] + oe: the next step's diagonal
        bot_h = uh;
        bot_f = uf;
        tch = tn;
        if (k == 63 && a) row[x - (RL - 1)] = bint2{uh, uf};                   // the stripe's bottom row, for the stripe below
    });
    if (SW || EXT) {
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            const bool better = cmax[r] > (bs[r] | 15);
            bs[r] = better ? cmax[r] : bs[r];
            bj[r] = better ? t0 : bj[r];
        }
    }
}

// The scores pass: banded_body's sweep (same windows, staging, hand-off row and result rules) around the value cell.
// row_cap: entries of a wave's hand-off row (the launch's widest band); dynamic LDS = kBandedWaves * row_cap * 8 bytes.
// EXT: xdrop, the early exit from the stripe loop, rows_out in PairResult::overlap and, with PEND, the pattern-end record as in banded_body.
template <int RL, int MODE, bool PEND = false, class Score>
__device__ __forceinline__ void banded_scores_body(const PairParams& G, const int row_cap, const Score& sc, lds_bint2* const lds, const int xdrop = 0) {
    static_assert(RL == 4 || RL == 8, "banded stripes: 256 or 512 rows");
    constexpr bool EXT = MODE == kBandedExt, NW = MODE == 0 || EXT, SW = MODE == 1, SG = MODE == 2;   // (EXT: NW's matrix)
    constexpr int S = 64 * RL;
    constexpr int SENT = kBandedSent;
    const int k = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    lds_bint2* const row = lds + (size_t)wave * (size_t)row_cap;
    const int go = G.gap, ge = G.gap_extend, oe = p_addw(go, ge);
    auto h0 = [&](int i) { return NW || SG ? (i ? p_addw(go, p_mulw(i, ge)) : 0) : 0; };   // H[i][0]
    for (uint32_t tid = blockIdx.x * kBandedWaves + wave; tid < G.n_pairs; tid += gridDim.x * kBandedWaves) {
        const PWA_GLOBAL PairDesc* const P = (const PWA_GLOBAL PairDesc*)(G.pairs + tid);
        const int n = __builtin_amdgcn_readfirstlane(P->n), m = __builtin_amdgcn_readfirstlane(P->m);
        const int lo = __builtin_amdgcn_readfirstlane((int)P->pad[0]), hi = __builtin_amdgcn_readfirstlane((int)P->pad[1]);
        const int n_str = __builtin_amdgcn_readfirstlane((int)P->n_stripes);
        const unsigned B = (unsigned)(hi - lo + 1);
        g_cu8* const pat = (g_cu8*)P->pat;
        const uint64_t tp = (uint64_t)(uintptr_t)P->txt;
        const uint32_t tlo = __builtin_amdgcn_readfirstlane((uint32_t)tp), thi = __builtin_amdgcn_readfirstlane((uint32_t)(tp >> 32));
        const uintptr_t tg = (uintptr_t)(((uint64_t)thi << 32) | tlo);
        // column 0 of row i holds its mode's boundary value only where the boundary path lies in the band
        auto valid0 = [&](int i) { return SW ? (-i >= lo && -i <= hi) : (hi >= 0 && -i >= lo); };
        int lb_s = 0, lb_i = 0, lb_j = 0;   // SW: this lane's record over all its rows and stripes; EXT: the wave's (uniform)
        int ext_rows = min(n, m - lo);      // EXT: rows_out when no row stops -- the last row that has an in-band cell
        PWA_GLOBAL int* const pend = PEND ? (PWA_GLOBAL int*)P->rows : nullptr;   // the pair's pattern-end record {rmax(n), its first column}
        for (int s = 0; s < n_str; ++s) {
            const int i0 = s * S + 1, ib = i0 - 1;
            const int c0 = max(1, i0 + lo), c1 = min(m, i0 + S - 1 + hi);
            if (c0 > m) break;          // the band has left the matrix
            if (c1 < c0) continue;      // ... or not entered it yet
            const int c0a = ((c0 - 1) & ~15) + 1;
            const int n_chunks = (c1 - c0a + 1 + 63 + 15) / 16;
            const int i_first = i0 + k * RL;
            const bool last = s == n_str - 1;
            int rs[RL], hl[RL], el[RL], bs[RL], bj[RL];
#pragma unroll
            for (int r = 0; r < RL; ++r) {
                const int i = i_first + r;
                rs[r] = sc.slot(i <= n ? pat[i - 1] : 0, i <= n);
                const int h = h0(i);
                const bool v = valid0(i);
                hl[r] = v ? p_addw(h, oe) : SENT;
                el[r] = v ? p_addw(h, go) : SENT;   // E[i][0] = H[i][0] + gap_open: its extension equals the opening
                bs[r] = EXT ? kBandedExtNone : 0;
                bj[r] = 0;
            }
            // the row above at column j (row ib): H + oe and F, the sentinel where it is not in the band
            auto top_at = [&](int j, int& th, int& tf) {
                const bool valid = j >= 1 && j <= m && j - ib >= lo && j - ib <= hi;
                if (s == 0) {   // row 0: H[0][j], F[0][j] = H[0][j] + gap_open
                    th = p_addw(NW ? p_addw(go, p_mulw(j, ge)) : 0, oe);
                    tf = p_addw(th, -ge);
                } else {
                    const bint2 v = row[valid ? j - ib - lo : 0];
                    th = v.x;
                    tf = v.y;
                }
                th = valid ? th : SENT;
                tf = valid ? tf : SENT;
            };
            int diag0 = valid0(i_first - 1) ? p_addw(h0(i_first - 1), oe) : SENT;   // H[i_first - 1][0]
            if (c0a > 1) {   // lane 0: H[ib][c0a - 1] from the row above
                int th, tf;
                top_at(c0a - 1, th, tf);
                diag0 = k == 0 ? th : diag0;
            }
            int own[RL] = {};
            if (SG) sg_own(own, i_first, n);
            int sg_v = valid0(n) ? p_addw(h0(n), oe) : (int)0x80000000, sg_t = k - c0a;   // SG: the record starts at column 0
            int bot_h = SENT, bot_f = SENT, tch = 0;
            const int tbase = c0a - 1;   // text byte of step 0 (a multiple of 16)
            auto stage = [&](int t0s, mu32x4& w) {
                const int tc = min(tbase + t0s, (m + 15) & ~15);
                w = *(const __attribute__((address_space(4))) mu32x4*)(tg + (size_t)tc);
            };
            const int wsel = k >> 2;
            mu32x4 wnext;
            stage(0, wnext);
            for (int ch = 0; ch < n_chunks; ++ch) {
                const int t0 = ch * 16;
                uint32_t wv = wnext[0];
#pragma unroll
                for (int x = 1; x < 4; ++x) wv = (wsel == x) ? wnext[x] : wv;
                const int tcv = sc.text(wv, k);
                stage(t0 + 16, wnext);
                int thv, tfv;
                top_at(c0a + t0 + (k & 15), thv, tfv);
                const int jm = c0a + t0 - k, xb = jm - i_first - lo;
                const bool interior = t0 >= 63 && c0a + t0 + 15 <= m;
                if (interior)
                    banded_scores_chunk<RL, MODE, false>(t0, k, jm, m, xb, B, rs, hl, el, diag0, bot_h, bot_f, tch, tcv, thv, tfv, oe, ge, bs, bj, own, sg_v,
                                                         sg_t, row, sc);
                else
                    banded_scores_chunk<RL, MODE, true>(t0, k, jm, m, xb, B, rs, hl, el, diag0, bot_h, bot_f, tch, tcv, thv, tfv, oe, ge, bs, bj, own, sg_v,
                                                        sg_t, row, sc);
            }
            if constexpr (EXT) {   // (a stop at the first row of a stripe is found here, by that stripe's test, with the record carried in)
                const int stop = banded_ext_stripe_end<RL>(bs, bj, i_first, n, c0a - k, xdrop, lb_s, lb_i, lb_j);
                if (stop) {
                    ext_rows = stop - 1;
                    break;
                }
                if constexpr (PEND)   // row n was kept (ext_rows stays n) and has an in-band cell
                    if (last && n <= m - lo) banded_ext_pattern_end<RL>(pend, bs, bj, i_first, n, c0a - k);
                continue;
            }
            PWA_GLOBAL PairResult* const res = (PWA_GLOBAL PairResult*)P->res;
            if (SG) {
                if (last && n >= i_first && n < i_first + RL) {
                    res->score = p_addw(sg_v, -oe);
                    res->end_i = (uint32_t)n;
                    res->end_j = (uint32_t)(c0a + sg_t - k);
                }
            } else if (NW) {
#pragma unroll
                for (int r = 0; r < RL; ++r)
                    if (last && i_first + r == n) {   // the row's state froze at column m
                        res->score = p_addw(hl[r], -oe);
                        res->end_i = (uint32_t)n;
                        res->end_j = (uint32_t)m;
                    }
            } else {
#pragma unroll
                for (int r = 0; r < RL; ++r) {
                    const int i = i_first + r, h = bs[r] >> 4;
                    if (i <= n && h > lb_s) {   // rows come in increasing order: a tie keeps the earlier row
                        lb_s = h;
                        lb_i = i;
                        lb_j = c0a + bj[r] + (15 - (bs[r] & 15)) - k;
                    }
                }
            }
        }
        if (EXT && k == 0) {
            PWA_GLOBAL PairResult* const res = (PWA_GLOBAL PairResult*)P->res;
            res->score = lb_s;
            res->end_i = (uint32_t)lb_i;
            res->end_j = (uint32_t)lb_j;
            res->overlap = ext_rows;
        }
        if (SW) {
            int s_best = lb_s, i_best = lb_i, j_best = lb_j;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const int so = __shfl_xor(s_best, off), io = __shfl_xor(i_best, off), jo = __shfl_xor(j_best, off);
                const bool better = so > s_best || (so == s_best && so > 0 && io < i_best);
                if (better) {
                    s_best = so;
                    i_best = io;
                    j_best = jo;
                }
            }
            if (k == 0) {
                PWA_GLOBAL PairResult* const res = (PWA_GLOBAL PairResult*)P->res;
                res->score = s_best;
                res->end_i = (uint32_t)i_best;
                res->end_j = (uint32_t)j_best;
            }
        }
    }
}

template <int RL, int MODE>
__global__ __launch_bounds__(64 * kBandedWaves) void banded_scores_kernel(const PairParams G, const int row_cap) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_scores_lds[];
    banded_scores_body<RL, MODE>(G, row_cap, BandedValueScore(G), (lds_bint2*)banded_scores_lds);
}

}  // namespace pwa
