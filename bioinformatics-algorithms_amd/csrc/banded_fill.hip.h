// banded_fill.hip.h -- banded affine-gap (gotoh) NW / SW / semi-global alignments of LONG pairs (gfx950 / MI355X):
// pwa_align_banded_batch and pwa_align_banded_batch_cigar (include/pwalign.h has the semantics, DESIGN.md §3.14 the figures).
//
// Cell (i, j) is in the band iff lo <= j - i <= hi; everything outside is -inf in H, E and F.  One wave per pair sweeps the pair stripe
// by stripe, alone: no flags, no spin-waits, no helper wave.  Stripe s covers S = 64 RL rows from i0 = s S + 1 (lane k owns RL
// consecutive rows), and visits only the column window [c0, c1] = [max(1, i0 + lo), min(m, i0 + S - 1 + hi)] -- started at c0a, c0
// rounded down to a 16-byte text boundary, so that the text is staged with the same aligned scalar loads as in gotoh_body.  Inside the
// window the scheme is gotoh_body's for 64 lanes: anti-diagonal front, `wave_shr:1` for the row above and the travelling text value,
// scalar text staging a chunk ahead, 16-step chunks, the keyed cell of gotoh_chunk (same keys, tie-breaks and code byte), the Score
// policy hooks.  What differs:
//   * the row above lane 0 is the previous stripe's bottom row.  Lane 63 parks the (H, F) keys of its last row's in-band columns in a
//     per-wave hand-off row in LDS, entry j - i - lo (at most one band width of 8-byte entries: kBandedMaxWidth comes from that); the
//     next stripe's lanes 0..15 read 16 entries per chunk and hand them to lane 0 step by step.  The row is reused in place: entry X of
//     the new row is written S + 63 steps after entry X of the old one was read.  Stripe 0 reads the boundary formula instead.  A column
//     that the row above does not hold in band reads as the sentinel.
//   * the mask.  A row's in-band columns are contiguous.  A row slot's state (H-left, E) starts as the sentinel, or as the column-0
//     boundary where that lies in the band, and is written only by in-band cells; what an out-of-band cell hands down (H and F for the
//     row below) is FORCED to the sentinel constant at every step, never carried and extended.  So E of a row's first in-band cell, F
//     of a column's first in-band cell and anything read across the band edge are the sentinel itself, and the diagonal neighbour of
//     an in-band cell is always in the band (same diagonal; at row 0 / column 0 the boundary rule of pwalign.h makes it valid).
//   * results are kept across stripes: SW one (H, i, j) record per lane, replaced on a strictly larger H only; SG the record of row n
//     over in-band columns; NW the state of row n frozen at column m.
// Why no key leaves int32.  A = max(|match|, |mismatch|, |gap_open| + |gap_extend|, 1).  The host admits a pair only while
// (n + m + 2) A < 2^28, so every real value V (an H, E or F that stands for a path, or such a value plus one more step) has
// |V| <= (n + m + 1) A <= 2^28 - 1 - A and its key V * 8 + 0..7 lies in [-2^31 + 8 + 8 A, 2^31 - 8 A).  The sentinel key is
// SENT = -2^31 + 8 A + 1: below every real key whatever its low bits, and all that is ever added to it where the sum is used is one
// gap extension (>= -8 A) or the -2 between the two H forms -- never twice, because the sum is compared, loses against SENT or a real
// key, and is dropped.  Sums that do wrap belong to out-of-band cells, whose results are discarded by the mask.  Every in-band cell of
// a valid band is reachable from the boundary inside the band (pwalign.h: validity), so its H is real.
// The EXT form (MODE = kBandedExt; pwa_extend_banded_batch) is NW's matrix -- boundaries, priorities, code bytes, so the
// NW walk reads its band -- with SW's per-row first-maximum keys over signed H, and a test at the end of every stripe
// (banded_ext_stripe_end) that folds the stripe's rows into the best-cell record in row order and finds the first row that the
// X-drop stops; the wave then leaves the stripe loop.  Why its row key fits: the key is H << 4 | (15 - q) with H of either sign, and
// the host admits an EXT pair only while (n + m + 2) A < 2^27 -- one bit tighter than above -- so |H| <= (n + m) A < 2^27 - 2 A and
// H * 16 + 0..15 lies strictly inside int32; "no in-band cell" is INT_MIN, below every real key, and INT_MIN >> 4 = -2^27 is below
// every real H.  best - xdrop cannot wrap: 0 <= best < 2^27 and 0 <= xdrop <= 2^27.
// Traceback band: per pair, stripe after stripe, a fixed pitch of banded_steps() steps of [64 lanes][RL code bytes] (BandGeo<64, RL>,
// one aligned store per lane and step); step t of stripe s holds lane k's column c0a(s) + t - k.
#pragma once
#include "gotoh_fill.hip.h"

namespace pwa {

constexpr int kBandedMaxWidth = 4096;   // band_hi - band_lo + 1: the hand-off row of a wave is at most 32 KiB of LDS
constexpr int kBandedWaves = 4;         // waves (pairs in flight) per workgroup
constexpr int kBandedExt = 3;           // MODE of the EXT form (extension from (0, 0) with an X-drop): no public mode value
constexpr int kBandedExtNone = (int)0x80000000;   // EXT row key: the row has no in-band cell (yet)

// first column a stripe's front starts at: c0 = max(1, i0 + lo), rounded down to a 16-byte boundary of the text
__host__ __device__ inline int64_t banded_c0a(int64_t i0, int64_t lo) {
    const int64_t c0 = i0 + lo > 1 ? i0 + lo : 1;
    return ((c0 - 1) & ~(int64_t)15) + 1;
}
// band steps of every stripe of a pair (the pitch): its widest window (S - 1 + B columns, at most m) + up to 15 columns of alignment
// + 63 steps of skew, in whole 16-step chunks.  B: the width of the band clamped to the matrix.
__host__ __device__ inline int64_t banded_steps(int64_t rows_per_stripe, int64_t B, int64_t m) {
    const int64_t w = rows_per_stripe - 1 + B < m ? rows_per_stripe - 1 + B : m;
    return (w + 15 + 63 + 15) & ~(int64_t)15;
}
// 16-step chunks the fill runs (and stores) for the stripe that starts at row i0
__host__ __device__ inline int64_t banded_chunks(int64_t i0, int64_t rows_per_stripe, int64_t lo, int64_t hi, int64_t m) {
    const int64_t c0 = i0 + lo > 1 ? i0 + lo : 1;
    const int64_t c1 = i0 + rows_per_stripe - 1 + hi < m ? i0 + rows_per_stripe - 1 + hi : m;
    if (c1 < c0) return 0;
    return (c1 - banded_c0a(i0, lo) + 1 + 63 + 15) / 16;
}

typedef int bint2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) bint2 lds_bint2;

// 16 steps of one stripe.  EDGE: some lane has not started, or lane 0 is at or past column m, at some step of the chunk.
// jm: this lane's column at step t0; xb = jm - i_first - lo: row slot r is in the band iff (unsigned)(xb + q - r) < B.
template <int RL, int MODE, bool EDGE, class Score>
__device__ __forceinline__ void banded_chunk(const int t0, const int k, const int jm, const int m, const int xb, const unsigned B, const int (&rs)[RL],
                                             int (&hl)[RL], int (&el)[RL], int& diag0, int& bot_h, int& bot_f, int& tch, const int tcv, const int thv,
                                             const int tfv, const GotohConst& K, const int SENT, int (&bs)[RL], int (&bj)[RL], const int (&own)[RL],
                                             int& sg_v, int& sg_t, g_u8* const tba, lds_bint2* const row, const Score& sc) {
    typedef BandGeo<64, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr int NQ = (RL + 3) / 4;
    constexpr bool SW = MODE == 1, SG = MODE == 2, EXT = MODE == kBandedExt;
    static_assert(Geo::PB == 0, "banded stripes: one store plane");
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
        uint32_t codes[NQ];
        int hst[RL];
        bool a = false;
#pragma unroll
        for (int r = 0; r < RL; ++r) {
            a = actl && (unsigned)(x - r) < B;                                 // the cell is in the band (and in the matrix)
            const int kd = p_addw(dg, sc.diag(tn, rs[r]));
            const int e = max(hl[r], p_addw(el[r] & ~1, K.ge8));               // E: open (x = 1) wins a tie
            const int f = max(uh, p_addw(uf & ~1, K.ge8));                     // F: likewise
            int kk = max(max(kd, e), f);
            if (SW) kk = max(kk, 2 * PR::Z);
            const int c = (kk & 6) | (e & 1) | ((f & 1) << 3);
            if (r % 4 == 0) gotoh_put_code<0>(codes[r / 4], c);
            if (r % 4 == 1) gotoh_put_code<1>(codes[r / 4], c);
            if (r % 4 == 2) gotoh_put_code<2>(codes[r / 4], c);
            if (r % 4 == 3) gotoh_put_code<3>(codes[r / 4], c);
            const int base = kk & ~7;
            const int hn = p_addw(base, K.cE);
            if (SW || EXT) {   // first maximum of the row over in-band cells (gotoh_chunk's folded keys; EXT: H of either sign)
                int key = (int)(((unsigned)base << 1) | (unsigned)(15 - q));
                key = a ? key : EXT ? kBandedExtNone : 0;
                if (q % 2 == 0) kprev[r] = key;
                else {
                    cmax[r] = q == 1 ? max(kprev[r], key) : max(max(cmax[r], kprev[r]), key);
                    asm volatile("" : "+v"(cmax[r]));
                }
            }
            if (SG) hst[r] = a ? hn : (int)0x80000000;
            dg = hl[r];
            uh = a ? p_addw(base, K.cF) : SENT;                                // out of band: forced, never carried
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
        const int d0 = p_addw(uh_in, K.cE - K.cF);                             // H[i_first - 1][j] as the next step's diagonal
        diag0 = started ? d0 : diag0;
        bot_h = uh;
        bot_f = uf;
        tch = tn;
        if constexpr (Geo::PA == 4) PWA_BAND_STORE((g_u32*)(tba + q * Geo::SR), codes[0]);
        if constexpr (Geo::PA == 8) PWA_BAND_STORE((PWA_GLOBAL mu32x2*)(tba + q * Geo::SR), (mu32x2{codes[0], codes[1]}));
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

// EXT, once per stripe: the stripe's 64 RL row records (bs / bj: each row's maximum over its in-band cells and where its first one is)
// in row order into the wave-uniform best-cell record (best_s, best_i, best_j), and the first row the X-drop stops: row i stops iff
// rmax(i) < best(i - 1) - xdrop (xdrop >= 0; a row without an in-band cell is -inf).  best(i - 1) before the first stop is the
// maximum of the record carried in and of every earlier row, so: an exclusive prefix maximum over lanes of the lanes' row maxima,
// seeded with the carried record; each lane tests its RL rows in order against that running best; one ballot finds the first stopping
// lane; the record is reduced over the rows before the stop by (H desc, i asc) and replaces the carried one on a strictly larger H.
// Returns the stopping row, or 0.  jbase: column of this lane at step 0 (c0a - lane).  Rows past n neither stop nor count.
template <int RL>
__device__ __forceinline__ int banded_ext_stripe_end(const int (&bs)[RL], const int (&bj)[RL], const int i_first, const int n, const int jbase,
                                                     const int xdrop, int& best_s, int& best_i, int& best_j) {
    constexpr int NINF = kBandedExtNone >> 4;   // -2^27: below every real H
    const int k = threadIdx.x & 63;
    int h[RL], pm = NINF;
#pragma unroll
    for (int r = 0; r < RL; ++r) {
        h[r] = i_first + r <= n ? bs[r] >> 4 : NINF;
        pm = max(pm, h[r]);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(pm, off);
        pm = k >= off ? max(pm, o) : pm;
    }
    int b = __shfl_up(pm, 1);
    b = k ? max(b, best_s) : best_s;   // best(i_first - 1), if no row above stops
    int stop_r = RL, cs = NINF, ci = 0, cj = 0;
#pragma unroll
    for (int r = 0; r < RL; ++r) {
        const bool live = i_first + r <= n && stop_r == RL;
        const bool stops = live && xdrop >= 0 && (h[r] == NINF || h[r] < b - xdrop);
        stop_r = stops ? r : stop_r;
        const bool kept = live && !stops;
        if (kept && h[r] > cs) {   // rows in increasing order: a tie keeps the earlier row
            cs = h[r];
            ci = i_first + r;
            cj = jbase + bj[r] + (15 - (bs[r] & 15));
        }
        b = kept ? max(b, h[r]) : b;
    }
    const uint64_t sm = __ballot(stop_r < RL);
    const int first = sm ? (int)__builtin_ctzll(sm) : 64;   // the first stopping lane: rows of the lanes behind it are not considered
    cs = k > first ? NINF : cs;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int so = __shfl_xor(cs, off), io = __shfl_xor(ci, off), jo = __shfl_xor(cj, off);
        const bool better = so > cs || (so == cs && io < ci);
        cs = better ? so : cs;
        ci = better ? io : ci;
        cj = better ? jo : cj;
    }
    const bool take = cs > best_s;
    best_s = __builtin_amdgcn_readfirstlane(take ? cs : best_s);
    best_i = __builtin_amdgcn_readfirstlane(take ? ci : best_i);
    best_j = __builtin_amdgcn_readfirstlane(take ? cj : best_j);
    return sm ? __builtin_amdgcn_readfirstlane(__shfl(i_first + stop_r, first & 63)) : 0;
}

// EXT, once per pair, after the test of the stripe that holds row n found no stop (and no stripe above it did), for a row n that has an
// in-band cell (n <= m - lo): the pattern-end record {rmax(n), the smallest column attaining it} from the row's own record, as
// banded_ext_stripe_end reads it.  One lane holds the row; pend[0..1] keep the host's "no value" wherever this does not run.  It is
// neither reached nor compiled unless the body is instantiated with PEND.
template <int RL>
__device__ __forceinline__ void banded_ext_pattern_end(PWA_GLOBAL int* const pend, const int (&bs)[RL], const int (&bj)[RL], const int i_first, const int n,
                                                       const int jbase) {
#pragma unroll
    for (int r = 0; r < RL; ++r)
        if (i_first + r == n) {
            pend[0] = bs[r] >> 4;
            pend[1] = jbase + bj[r] + (15 - (bs[r] & 15));
        }
}

// The fill.  Workgroups of kBandedWaves waves, pairs dealt statically (the host sorts them longest first); PairDesc::pad[0 / 1] = the band
// clamped to the matrix (lo >= -n, hi <= m), row_stride = the band pitch in steps (banded_steps), n_stripes = ceil(n / 64 RL).
// row_cap: entries of a wave's hand-off row (the launch's widest band); dynamic LDS = kBandedWaves * row_cap * 8 bytes.
// EXT: xdrop is the call's; the wave leaves a pair's stripe loop at the stripe whose test finds a stopping row, and PairResult::overlap
// (unused by the banded class) carries rows_out.  PEND (EXT only; the table kernels of banded_ext_subst_kernels.hip): PairDesc::rows, unused
// by the banded class too, points at the pair's pattern-end record, written by banded_ext_pattern_end when the sweep keeps row n.
template <int RL, int MODE, bool PEND = false, class Score>
__device__ __forceinline__ void banded_body(const PairParams& G, const int row_cap, const Score& sc, lds_bint2* const lds, const int xdrop = 0) {
    static_assert(RL == 4 || RL == 8, "banded stripes: 256 or 512 rows");
    typedef BandGeo<64, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr bool EXT = MODE == kBandedExt, NW = MODE == 0 || EXT, SW = MODE == 1, SG = MODE == 2;   // (EXT: NW's matrix)
    constexpr int S = 64 * RL;
    const int k = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    lds_bint2* const row = lds + (size_t)wave * (size_t)row_cap;
    const int go = G.gap, ge = G.gap_extend;
    const GotohConst K = gotoh_const<MODE>(G);
    const int amax = max(max(max(abs(G.match), abs(G.mismatch)), abs(go) + abs(ge)), 1);
    const int SENT = (int)(0x80000000u + 8u * (unsigned)amax + 1u);
    auto h0 = [&](int i) { return NW || SG ? (i ? p_addw(go, p_mulw(i, ge)) : 0) : 0; };   // H[i][0]
    for (uint32_t tid = blockIdx.x * kBandedWaves + wave; tid < G.n_pairs; tid += gridDim.x * kBandedWaves) {
        const PWA_GLOBAL PairDesc* const P = (const PWA_GLOBAL PairDesc*)(G.pairs + tid);
        const int n = __builtin_amdgcn_readfirstlane(P->n), m = __builtin_amdgcn_readfirstlane(P->m);
        const int lo = __builtin_amdgcn_readfirstlane((int)P->pad[0]), hi = __builtin_amdgcn_readfirstlane((int)P->pad[1]);
        const int pitch = __builtin_amdgcn_readfirstlane((int)P->row_stride), n_str = __builtin_amdgcn_readfirstlane((int)P->n_stripes);
        const unsigned B = (unsigned)(hi - lo + 1);
        g_cu8* const pat = (g_cu8*)P->pat;
        g_u8* const tb = (g_u8*)P->tb;
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
                hl[r] = v ? p_addw(p_mulw(h, 8), K.cE) : SENT;
                el[r] = v ? p_addw(p_mulw(p_addw(h, go), 8), 2 * PR::E) : SENT;   // E[i][0] = H[i][0] + gap_open: its extension ties the opening
                bs[r] = EXT ? kBandedExtNone : 0;
                bj[r] = 0;
            }
            // the row above at column j (row ib): its (H as an F-open candidate, F) keys, the sentinel where it is not in the band
            auto top_at = [&](int j, int& th, int& tf) {
                const bool valid = j >= 1 && j <= m && j - ib >= lo && j - ib <= hi;
                if (s == 0) {   // row 0: H[0][j], F[0][j] = H[0][j] + gap_open
                    th = p_addw(p_mulw(NW ? p_addw(go, p_mulw(j, ge)) : 0, 8), K.cF);
                    tf = p_addw(th, -K.ge8 - 1);
                } else {
                    const bint2 v = row[valid ? j - ib - lo : 0];
                    th = v.x;
                    tf = v.y;
                }
                th = valid ? th : SENT;
                tf = valid ? tf : SENT;
            };
            int diag0 = valid0(i_first - 1) ? p_addw(p_mulw(h0(i_first - 1), 8), K.cE) : SENT;   // H[i_first - 1][0]
            if (c0a > 1) {   // lane 0: H[ib][c0a - 1] from the row above
                int th, tf;
                top_at(c0a - 1, th, tf);
                diag0 = k == 0 ? p_addw(th, K.cE - K.cF) : diag0;
            }
            int own[RL] = {};
            if (SG) sg_own(own, i_first, n);
            int sg_v = valid0(n) ? p_addw(p_mulw(h0(n), 8), K.cE) : (int)0x80000000, sg_t = k - c0a;   // SG: the record starts at column 0
            int bot_h = SENT, bot_f = SENT, tch = 0;
            const int tbase = c0a - 1;   // text byte of step 0 (a multiple of 16)
            auto stage = [&](int t0s, mu32x4& w) {
                const int tc = min(tbase + t0s, (m + 15) & ~15);
                w = *(const __attribute__((address_space(4))) mu32x4*)(tg + (size_t)tc);
            };
            const int wsel = k >> 2;
            mu32x4 wnext;
            stage(0, wnext);
            g_u8* const tbs0 = tb + (size_t)s * (size_t)pitch * Geo::SR + k * Geo::PA;
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
                g_u8* const tbs = tbs0 + (size_t)t0 * Geo::SR;
                const bool interior = t0 >= 63 && c0a + t0 + 15 <= m;
                if (interior)
                    banded_chunk<RL, MODE, false>(t0, k, jm, m, xb, B, rs, hl, el, diag0, bot_h, bot_f, tch, tcv, thv, tfv, K, SENT, bs, bj, own, sg_v, sg_t,
                                                  tbs, row, sc);
                else
                    banded_chunk<RL, MODE, true>(t0, k, jm, m, xb, B, rs, hl, el, diag0, bot_h, bot_f, tch, tcv, thv, tfv, K, SENT, bs, bj, own, sg_v, sg_t,
                                                 tbs, row, sc);
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
                    res->score = (int)((unsigned)sg_v - (unsigned)K.cE) >> 3;
                    res->end_i = (uint32_t)n;
                    res->end_j = (uint32_t)(c0a + sg_t - k);
                }
            } else if (NW) {
#pragma unroll
                for (int r = 0; r < RL; ++r)
                    if (last && i_first + r == n) {   // the row's state froze at column m
                        res->score = (int)((unsigned)hl[r] - (unsigned)K.cE) >> 3;
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
__global__ __launch_bounds__(64 * kBandedWaves) void banded_fill_kernel(const PairParams G, const int row_cap) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_lds[];
    banded_body<RL, MODE>(G, row_cap, GotohByteScore<MODE>(G), (lds_bint2*)banded_lds);
}

// The walk: gotoh_walk_kernel's three-state machine and LDS-DMA window staging over the banded layout.  The band of a pair is a plain
// sequence of 16-step windows (stripe s starts at step s * pitch), so a cell's window is (s * pitch + t) / 16 with t = j - c0a(s) +
// lane; inside a stripe the walk moves to earlier steps as in gotoh_walk_kernel, across a stripe boundary to an unrelated window.
template <int RL, int MODE>
__global__ __launch_bounds__(64) void banded_walk_kernel(const PairParams G) {
    typedef BandGeo<64, RL> Geo;
    typedef GotohPrio<MODE> PR;
    constexpr bool SW = MODE == 1, NW = MODE == 0;
    constexpr int SR = Geo::SR;   // bytes per band step = rows per stripe
    constexpr int WIN = 16;
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
    const int lo = __builtin_amdgcn_readfirstlane((int)P.pad[0]);
    const long long pitch = (long long)__builtin_amdgcn_readfirstlane((int)P.row_stride);
    const uint32_t cap = P.ops_cap;
    auto issue = [&](int buf, long long w) {   // window w into LDS buffer buf: 1 KiB per instruction
        buf = __builtin_amdgcn_readfirstlane(buf);
        const size_t off0 = (size_t)w * WB;
#pragma unroll
        for (int u = 0; u < WB / 1024; ++u)
            __builtin_amdgcn_global_load_lds((const PWA_GLOBAL uint32_t*)(tb + off0 + (size_t)u * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) uint32_t*)(win + buf * WB + u * 1024), 16, 0, 0);
    };
    uint32_t cnt = 0, ob = 0;
    auto put = [&](uint32_t op) {
        const uint32_t slot = cnt & 63u;
        ob = (uint32_t)lane == slot ? op : ob;
        ++cnt;
        if (slot == 63u) ops[cnt - 64u + (uint32_t)lane] = (uint8_t)ob;
    };
    int st = 0;   // 0: H, 1: E, 2: F
    long long cur_w = -1, pre_w = -1;
    bool fault = false;
    while (i > 0 && j > 0) {
        if (cnt >= cap) {   // cannot happen (every op moves i or j): never spin on the GPU
            fault = true;
            break;
        }
        const int q = i - 1, s = q / SR, ql = q - s * SR;
        const int c0 = max(1, s * SR + 1 + lo), c0a = ((c0 - 1) & ~15) + 1;
        const long long t = (long long)s * pitch + (long long)(j - c0a + Geo::lane(ql));
        const long long w = t / WIN;
        if (w != cur_w) {
            if (w != pre_w) {
                if (pre_w >= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (a jump across stripes: let the window in flight land first)
                issue((int)(w & 1), w);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // LDS-DMA is ordered for our ds_read by vmcnt
            cur_w = w;
            pre_w = -1;
            if (w > 0) {
                issue((int)((w - 1) & 1), w - 1);
                pre_w = w - 1;
            }
        }
        const int c = __builtin_amdgcn_readfirstlane((int)win[(int)(w & 1) * WB + (int)(t - w * WIN) * SR + Geo::off(ql)]);
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no window may still be in flight when the wave ends
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
