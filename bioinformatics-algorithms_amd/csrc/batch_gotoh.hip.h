// batch_gotoh.hip.h -- scores-only affine-gap (gotoh) NW and SW alignment of many pairs (gfx950 / MI355X): the strip engine of
// pwa_gotoh_batch_create / pwa_scores_gotoh.  include/pwalign.h (pwa_align_gotoh_batch) has the recurrence, DESIGN.md §3.12 the
// figures.
//
// Mapping of batch_affine.hip.h (lane = pair, text symbol in an SGPR, register strips of R rows, 4 skewed columns per block,
// branch-free strip hand-off through HBM, atomic task queue), three values per row: H, E and Ho = H + oe (oe = gap_open +
// gap_extend).  The strip hand-off carries two values per column: H of the bottom row and the F the next row will see.  Scores only:
// plain int32 maxima, no tie-break keys, no codes.
//   plain   v = Hdiag + s;  f = max(Ho_up, F_up + ge);  e = max(Ho_left, E_left + ge);  h = max3(v, f, e) [SW: and 0];  Ho = h + oe
//           7 VALU per cell + 0.5 for the table (SW: + the zero floor and the running maximum)
//   SHIFT   NW in coordinates shifted by ge (i + j):  v = H~diag + (s - 2 ge);  f = max(Hg_up, F~up);  e = max(Hg_left, E~left);
//           h = max3;  Hg = h + gap_open: 5 + 0.5.  Used when every value stays far inside int32 (host check).
// There is no -inf: E[i][0] = H[i][0] + gap_open and F[0][j] = H[0][j] + gap_open (gotoh_fill.hip.h), whose extension equals the
// opening from the same cell -- the value -inf gives, with every number inside the range bound.
// Rows past a lane's pattern hold a symbol that equals no text symbol.  They only feed rows below them, so NW reads H[n][m] from the
// strip its row n lies in; SW's running maximum includes them, and the host sends an SW list here only when mismatch <= 0 (gap terms
// are <= 0 anyway): such rows never exceed the real rows above them.
#pragma once
#include "batch_affine.hip.h"

namespace pwa {

enum { BM_GNW = 8, BM_GNWS = 9, BM_GSW = 10 };   // gotoh NW plain / shifted, gotoh SW (0..7: batch_scores.hip.h, kernel_table.h)

// AffineParams: go = gap_open, ge = gap_extend; neg is unused.  SHIFT: b.match / b.mismatch and the table hold s - 2 ge.
template <int R, int C, int SCORE, bool LOCAL, bool SHIFT>
__device__ __forceinline__ void gotoh_block(int (&Ho)[R], int (&E)[R], int (&H)[R], const uint32_t (&pk)[R / 4], const uint32_t (&cs)[C],
                                            const int (&htop)[C], const int (&fin)[C], int& topprev, int (&hbot)[C], int (&fbot)[C], int& best,
                                            const AffineParams& P) {
    constexpr int Q = R / 4;
    int d[C], hu[C], fu[C], hl[C];
    const int ge = P.ge, hadd = SHIFT ? P.go : addw(P.go, P.ge);
#pragma unroll
    for (int k = 0; k < C; ++k) {
        d[k] = (k == 0) ? topprev : htop[k - 1];   // H of the row above, previous column
        hu[k] = fin[k];                            // makes the first row's F equal to the handed-in F
        fu[k] = SHIFT ? fin[k] : addw(fin[k], -ge);
        hl[k] = 0;
    }
    topprev = htop[C - 1];
#pragma unroll
    for (int step = 0; step < Q + C - 1; ++step) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int q = step - k;
            if (q >= 0 && q < Q) {
                uint32_t s4 = 0;
                if (SCORE == SC_PERM) s4 = __builtin_amdgcn_perm(P.b.tab_hi, P.b.tab_lo, pk[q] ^ cs[k]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int r = 4 * q + b;
                    int s;
                    if (SCORE == SC_PERM) s = (int)(int8_t)(s4 >> (8 * b));
                    else s = (((pk[q] >> (8 * b)) & 0xffu) == cs[k]) ? P.b.match : P.b.mismatch;
                    const int v = addw(d[k], s);
                    d[k] = H[r];
                    const int f = SHIFT ? max(hu[k], fu[k]) : max(hu[k], addw(fu[k], ge));
                    const int e = SHIFT ? max(Ho[r], E[r]) : max(Ho[r], addw(E[r], ge));
                    int h = max(max(v, f), e);
                    if (LOCAL) {
                        h = max(h, 0);
                        best = max(best, h);
                    }
                    const int ho = addw(h, hadd);
                    Ho[r] = ho;
                    E[r] = e;
                    H[r] = h;
                    hu[k] = ho;
                    fu[k] = f;
                    hl[k] = h;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        hbot[k] = hl[k];                                                      // H of the strip's bottom row
        fbot[k] = SHIFT ? max(hu[k], fu[k]) : max(hu[k], addw(fu[k], ge));    // F of the row below it
    }
}

// MODE: BM_GNW | BM_GNWS | BM_GSW
template <int R, int SCORE, int MODE>
__global__ __launch_bounds__(64, affine_waves_per_simd(R)) void batch_gotoh_kernel(const AffineParams P) {
    constexpr int Q = R / 4;
    constexpr bool LOCAL = MODE == BM_GSW, SHIFT = MODE == BM_GNWS;
    const BatchParams& B = P.b;
    const int lane = threadIdx.x;
    int32_t* const hand = B.hand + (size_t)blockIdx.x * B.hand_stride;
    const int go = P.go, ge = P.ge, oe = addw(go, ge);
    // boundary H[i][0] / H[0][j] for i, j >= 1, and what sits beside it in a row's (column's) state
    auto hb = [&](int x) { return LOCAL ? 0 : (SHIFT ? go : addw(go, mulw(x, ge))); };

    for (;;) {
        uint32_t tid = 0;
        {
            int elect = lane;   // opaque electing lane: see batch_scores.hip.h
            asm volatile("" : "+v"(elect));
            if (elect == 0) tid = atomicAdd(B.queue, 1u);
        }
        tid = __builtin_amdgcn_readfirstlane(tid);
        if (tid >= B.n_tasks) break;

        const BatchTask task = B.tasks[tid];
        const int m = (int)task.text_len;
        const uint32_t* tx = reinterpret_cast<const uint32_t*>(B.arena + task.text_off);
        const uint32_t slot = task.slot0 + lane;
        const uint32_t poff = B.slot_poff[slot];
        const int n = (int)B.slot_plen[slot];
        const uint32_t outi = B.slot_out[slot];
        const int nblk = m >> 2, rem = m & 3;
        int result = 0, best = 0;

        for (int s = 0; s < (int)task.n_strips; ++s) {
            const int row0 = s * R;
            uint32_t pk[Q];
            {
                const uint32_t* pp = reinterpret_cast<const uint32_t*>(B.arena + poff + row0);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int valid = n - (row0 + 4 * q);
                    const uint32_t w = pp[q];
                    const uint32_t keep = valid >= 4 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u));
                    pk[q] = (w & keep) | (B.pad_word & ~keep);
                }
            }
            // ---- column 0: H[i][0], Ho = H[i][0] + oe (SHIFT: + gap_open), E[i][0] = H[i][0] + gap_open
            int Ho[R], E[R], H[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int h0 = hb(row0 + r + 1);
                H[r] = h0;
                Ho[r] = addw(h0, SHIFT ? go : oe);
                E[r] = addw(h0, go);
            }
            int topprev = (s == 0 && !LOCAL) ? 0 : hb(row0);   // H of the row above the strip at column 0: H[0][0] = 0

            const bool has_top = s > 0;
            const bool has_bot = s + 1 < (int)task.n_strips;
            const int32_t* hin = hand + (size_t)((s + 1) & 1) * B.hand_half;
            int32_t* hout = hand + (size_t)(s & 1) * B.hand_half;
            const size_t in_stride = has_top ? 128 : 0, out_stride = has_bot ? 128 : 0;   // two int4 per lane per block
            const int4* hin4 = reinterpret_cast<const int4*>(hin) + lane;
            int4* hout4 = reinterpret_cast<int4*>(hout) + lane;
            int4 hnext = hin4[0], fnext = hin4[64];
            uint32_t cwn = tx[0];
            for (int jb = 0; jb < nblk; ++jb) {
                const uint32_t cw = cwn;
                const int4 hcur = hnext, fcur = fnext;
                cwn = tx[jb + 1];
                hnext = hin4[(size_t)(jb + 1) * in_stride];
                fnext = hin4[(size_t)(jb + 1) * in_stride + 64];
                int htop[4], fin[4], hbot[4], fbot[4];
                uint32_t cs[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t c = (cw >> (8 * k)) & 0xffu;
                    cs[k] = (SCORE == SC_PERM) ? c * 0x01010101u : c;
                }
                {
                    const int hl[4] = {hcur.x, hcur.y, hcur.z, hcur.w}, fl[4] = {fcur.x, fcur.y, fcur.z, fcur.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        // row 0: H[0][j]; F of row 1 = max(H[0][j] + oe, F[0][j] + ge) = H[0][j] + oe
                        const int h0 = hb(4 * jb + k + 1);
                        htop[k] = has_top ? hl[k] : h0;
                        fin[k] = has_top ? fl[k] : addw(h0, SHIFT ? go : oe);
                    }
                }
                gotoh_block<R, 4, SCORE, LOCAL, SHIFT>(Ho, E, H, pk, cs, htop, fin, topprev, hbot, fbot, best, P);
                hout4[(size_t)jb * out_stride] = make_int4(hbot[0], hbot[1], hbot[2], hbot[3]);
                hout4[(size_t)jb * out_stride + 64] = make_int4(fbot[0], fbot[1], fbot[2], fbot[3]);
            }
            if (rem > 0) {
                uint32_t cw = cwn;
                int h0 = hnext.x, h1 = hnext.y, h2 = hnext.z, f0 = fnext.x, f1 = fnext.y, f2 = fnext.z;
#pragma unroll 1
                for (int k = 0; k < rem; ++k) {
                    const uint32_t c = cw & 0xffu;
                    cw >>= 8;
                    const uint32_t cs1[1] = {(SCORE == SC_PERM) ? c * 0x01010101u : c};
                    const int hz = hb(4 * nblk + k + 1);
                    const int htop1[1] = {has_top ? h0 : hz};
                    const int fin1[1] = {has_top ? f0 : addw(hz, SHIFT ? go : oe)};
                    h0 = h1; h1 = h2;
                    f0 = f1; f1 = f2;
                    int hbot1[1], fbot1[1];
                    gotoh_block<R, 1, SCORE, LOCAL, SHIFT>(Ho, E, H, pk, cs1, htop1, fin1, topprev, hbot1, fbot1, best, P);
                    hout[((size_t)nblk * out_stride + lane) * 4 + k] = hbot1[0];
                    hout[((size_t)nblk * out_stride + 64 + lane) * 4 + k] = fbot1[0];
                }
            }
            // ---- NW: H[n][m] sits in this strip for the lanes whose pattern ends here
            if (!LOCAL) {
                const int rl = n - 1 - row0;
                if (rl >= 0 && rl < R) {
                    int v = 0;
#pragma unroll
                    for (int r = 0; r < R; ++r) v = (rl == r) ? H[r] : v;
                    result = v;
                }
            }
        }
        if (outi != 0xffffffffu) B.scores[outi] = LOCAL ? best : (SHIFT ? addw(result, mulw(n + m, ge)) : result);
    }
}

}  // namespace pwa
