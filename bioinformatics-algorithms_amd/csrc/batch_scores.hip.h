// batch_scores.hip.h -- scores-only DP for MANY pairs (gfx950 / MI355X).
//
// Replaces the score part of hw2.cpp's per-pair calls in the loop 328-338:
//   NW  dp[n][m]           recurrence hw2.cpp:138-156
//   SW  max over all cells recurrence hw2.cpp:205-231
//
// Mapping (MI355X-first, nothing like the reference's row-major scalar loop):
//   * one 64-lane wavefront = one "wave task" = up to 64 PATTERNS against ONE shared TEXT;
//     lane l owns the whole DP matrix of pair (pattern_l, text): no cross-lane traffic at all;
//   * the text character of a column is wave-uniform, so it lives in an SGPR (scalar loads);
//   * each lane keeps a register tile of R consecutive DP rows ("strip"): H[R] int32 in VGPRs plus
//     the strip's R pattern symbols packed 4 per VGPR; a column update is R dependent-free
//     register cells; columns are processed 4 at a time in a skewed (anti-diagonal) order so
//     that four independent dependency chains are in flight per lane;
//   * patterns longer than R rows take several strips; the strip's bottom row is handed to the
//     next strip through a per-workgroup HBM row buffer laid out [column/4][lane][4] so that every
//     access is one coalesced 1 KiB dwordx4 wave access (8 B per R cells per lane).  The column
//     loop is kept ONE basic block: the row load/store is unconditional and a stride of 0 parks
//     it on a 1 KiB dummy block when there is no strip above / below (a uniform branch in that
//     loop makes hipcc double the live H registers and spill);
//   * substitution score of 4 rows at once: one v_xor + one v_perm_b32 byte-table lookup
//     (alphabets of <= 7 symbols, scores in int8), then one SDWA add per cell; the generic
//     raw-byte path does compare + select per cell;
//   * wave tasks are pulled from an atomic queue (heterogeneous task sizes).
//
// Integer recurrences only: VALU-issue bound, no MFMA, HBM traffic ~1e-5 B/cell (C3).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pwa {

// NWG: NW in gap-shifted space G = H - g(i+j).
// SWS: SW with a second stored form per row, Hs = max(H + g, 0) (one unsigned saturating subtract).  Both gap
//      candidates then arrive already floored at 0, so  max(0, t, u+g, l+g) = max3(t, Hs_up, Hs_left)  with
//      no explicit 0 and no separate "+ g": 3 VALU per cell instead of 4 (+ 1/2 table + 1/2 running best),
//      at the price of 2R instead of R registers per lane (R <= 96).
enum { BM_SW = 0, BM_NW = 1, BM_NWG = 2, BM_SWS = 6 };
enum { SC_PERM = 0, SC_CMP = 1 };

struct BatchTask {
    uint32_t text_off;   // byte offset of the text symbols in the arena (16-byte aligned)
    uint32_t text_len;   // m
    uint32_t slot0;      // first of this task's 64 lane slots
    uint32_t n_strips;   // ceil(longest pattern of the task / R)
};

struct BatchParams {
    const uint8_t* arena;        // symbols of every sequence, each 16-byte aligned, with slack
    const BatchTask* tasks;
    const uint32_t* slot_poff;   // per slot: arena offset of the pattern
    const uint32_t* slot_plen;   // per slot: pattern length, 0 = empty lane
    const uint32_t* slot_out;    // per slot: index into scores
    const uint32_t* slot_toff;   // LANES kernels (every lane its own text): per slot arena offset / length of the text
    const uint32_t* slot_tlen;
    const uint8_t* lane_text;    // LANES + BM_NWG: right-aligned, front-padded text rows (slot_toff points in here)
    int32_t* scores;
    int32_t* hand;               // strip hand-off rows, one region per workgroup
    uint64_t hand_stride;        // int32 elements per workgroup region (2 halves)
    uint32_t hand_half;          // int32 elements per half
    uint32_t* queue;             // atomic task counter (zeroed before every launch)
    uint32_t n_tasks;
    int32_t match, mismatch, gap;
    uint32_t tab_hi, tab_lo;     // SC_PERM: byte table, selector 0 -> match, 1..7 -> mismatch
    uint32_t pad_word;           // symbol that matches nothing in any text, x4
    uint32_t tpad_word;          // LANES: symbol that matches nothing in any pattern and differs from pad_word, x4
    // CELL16 (packed f16 cells, two pairs per lane): scores as f16 bit patterns of s * 2^-11.  The per-column table's low /
    // high bytes are {lo,hi}16_base ^ ({lo,hi}16_diff << 8c) for text code c (bytes 0..3 = pattern codes 0..3)
    uint32_t lo16_base, lo16_diff, hi16_base, hi16_diff;
    uint32_t gap16x2;            // f16x2 of gap * 2^-11, both halves
};

__device__ __forceinline__ int addw(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int mulw(int a, int b) { return (int)((unsigned)a * (unsigned)b); }

// One block of C columns over the lane's R-row register strip.
//   H[r]     in:  dp[row0+r+1][j0]        (the column left of the block)
//            out: dp[row0+r+1][j0+C]
//   top[k]   dp[row0][j0+1+k]  (row above the strip), topprev = dp[row0][j0]
//   bot[k]   dp[row0+R][j0+1+k]
__device__ __forceinline__ int usub_sat(int a, int b) {   // max(a - b, 0) for a, b >= 0: v_sub_u32 ... clamp
    return (int)__builtin_elementwise_sub_sat((unsigned)a, (unsigned)b);
}

template <int R, int C, int MODE, int SCORE>
__device__ __forceinline__ void dp_block(int (&H)[R], int (&Hs)[MODE == BM_SWS ? R : 1], const uint32_t (&pk)[R / 4],
                                         const uint32_t (&cs)[C], const int (&top)[C], int& topprev, int (&bot)[C], int& best,
                                         const BatchParams& P) {
    constexpr int Q = R / 4;
    int d[C], u[C], hb[C];
    const int gap = P.gap;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        d[k] = (k == 0) ? topprev : top[k - 1];
        u[k] = (MODE == BM_SWS) ? usub_sat(top[k], -gap) : top[k];
        hb[k] = 0;
    }
    topprev = top[C - 1];
    // skewed order: column k runs one quad (4 rows) behind column k-1
#pragma unroll
    for (int step = 0; step < Q + C - 1; ++step) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int q = step - k;
            if (q >= 0 && q < Q) {
                uint32_t s4 = 0;
                if (SCORE == SC_PERM) s4 = __builtin_amdgcn_perm(P.tab_hi, P.tab_lo, pk[q] ^ cs[k]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int r = 4 * q + b;
                    int s;
                    if (SCORE == SC_PERM) s = (int)(int8_t)(s4 >> (8 * b));
                    else s = (((pk[q] >> (8 * b)) & 0xffu) == cs[k]) ? P.match : P.mismatch;
                    const int t = addw(d[k], s);   // diagonal candidate, hw2.cpp:142 / 208
                    const int l = H[r];            // dp[i][j-1]
                    d[k] = l;
                    int h;
                    if (MODE == BM_SWS) {
                        const int ls = Hs[r];                    // max(dp[i][j-1] + g, 0)
                        h = max(max(t, u[k]), ls);               // = max(0, diag, up, left), hw2.cpp:211
                        best = max(best, h);
                        const int hs = usub_sat(h, -gap);
                        Hs[r] = hs;
                        H[r] = h;
                        u[k] = hs;
                        hb[k] = h;
                        continue;
                    }
                    if (MODE == BM_SW) {
                        const int e = addw(max(u[k], l), gap);   // hw2.cpp:209-210
                        h = max(max(t, e), 0);                   // hw2.cpp:211
                        best = max(best, h);                     // hw2.cpp:225 (value only)
                    } else if (MODE == BM_NW) {
                        const int e = addw(max(u[k], l), gap);   // hw2.cpp:140-141
                        h = max(t, e);                           // hw2.cpp:142-153 (value only)
                    } else {
                        h = max(max(t, u[k]), l);                // gap folded into the coordinates
                    }
                    H[r] = h;
                    u[k] = h;
                    hb[k] = h;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < C; ++k) bot[k] = hb[k];
}

// Register budget: H[R] + R/4 packed symbols + ~30 live temporaries.  The second launch-bound is the
// number of waves per SIMD the allocation must leave room for (512 registers per SIMD lane, AGPRs
// included): without it hipcc parks 12 values in AGPRs at R = 152, the wave allocates 268 registers
// and only ONE wave fits per SIMD -- which halves VALU throughput (one wave issues every 4 cycles).
constexpr int strip_waves_per_simd(int R, int MODE) {
    return (MODE == BM_SWS) ? (R > 48 ? 2 : 3) : (R > 104 ? 2 : (R > 80 ? 3 : 4));
}

// ---------------------------------------------------------------------------------------------------
// CELL16: the saturating SW form (BM_SWS, SC_PERM) with TWO pairs per lane in packed f16 cells.  Every score is stored as
// k * 2^-11 with k an integer: the host admits a batch only when |match|, |mismatch|, |gap| <= 127 and
// longest pattern * max(match, 0) <= 2047, so every H, t = d + s and h + g is k * 2^-11 with |k| <= 2047 -- exact in f16
// (normal or zero, no rounding) -- and the clamp of v_pk_add_f16 to [0, 1] is the floor at 0 (h + g never exceeds 1).
// One row of BOTH pairs is then
//   s  = v_perm_b32(table of the column, selector of the row)    both pairs' f16 scores in one dword
//   t  = d + s                  v_pk_add_f16
//   h  = max3(t, Hs_up, Hs_left) v_pk_maximum3_f16              = max(0, diag, up + g, left + g), hw2.cpp:211
//   Hs = clamp(h + g)           v_pk_add_f16 ... clamp
//   best = max3(best, h, h')    (half a v_pk_maximum3_f16 per row)
// = 4.5 VALU per row and two pairs against 2 x 4.06 for the int32 cells.  The text symbol c of a column is wave-uniform, so the
// 8-byte v_perm table is built per column on the scalar unit: bytes 0..3 hold the low bytes of f16(s(p, c)) for pattern codes
// p = 0..3, bytes 4..7 the high bytes; a row's selector is (pA, pA + 4, pB, pB + 4), and 12 (-> 0x00 = +0.0) for pad rows.
// A score of 0 below a pattern's end keeps every padded value <= a real one (g <= 0), as the int32 pad rows do.
// Register state: H, Hs and the selector per row, 3R VGPRs; the hand-off keeps the [column/4][lane][4] layout, each dword the
// two pairs' f16 values.
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ half2_t h2_bits(uint32_t v) { return __builtin_bit_cast(half2_t, v); }
__device__ __forceinline__ uint32_t h2_u32(half2_t v) { return __builtin_bit_cast(uint32_t, v); }
// max(h + g, 0) for both halves: v_pk_add_f16 with the output clamp to [0, 1] (the compiler emits a separate clamping max for the
// builtin form, hence the asm; not volatile, so it schedules like any other instruction)
__device__ __forceinline__ half2_t h2_add_clamp(half2_t h, uint32_t g) {
    uint32_t r;
    asm("v_pk_add_f16 %0, %1, %2 clamp" : "=v"(r) : "v"(h2_u32(h)), "s"(g));
    return h2_bits(r);
}

template <int R, int C>
__device__ __forceinline__ void dp_block16(half2_t (&H)[R], half2_t (&Hs)[R], const uint32_t (&sel)[R], const uint32_t (&tlo)[C],
                                           const uint32_t (&thi)[C], const half2_t (&top)[C], half2_t& topprev, half2_t (&bot)[C],
                                           half2_t& best, uint32_t g) {
    half2_t d[C], u[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        d[k] = (k == 0) ? topprev : top[k - 1];
        u[k] = h2_add_clamp(top[k], g);
    }
    topprev = top[C - 1];
    // skewed order as dp_block: column k runs one quad (4 rows) behind column k-1
#pragma unroll
    for (int step = 0; step < R / 4 + C - 1; ++step) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int q = step - k;
            if (q >= 0 && q < R / 4) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int r = 4 * q + b;
                    // one ordered asm block per row: with the four instructions free to move, hipcc computes the diagonal
                    // candidates of whole columns ahead (they do not depend on the chain) and needs ~45 VGPRs more than
                    // 3R + the skew's d / u, which at R = 76 spill inside the column loop
                    uint32_t hv, hsv = h2_u32(Hs[r]), sv, tv;
                    asm volatile("v_perm_b32 %[s], %[thi], %[tlo], %[sel]\n\t"
                                 "v_pk_add_f16 %[t], %[d], %[s]\n\t"
                                 "v_pk_maximum3_f16 %[h], %[t], %[u], %[hs]\n\t"
                                 "v_pk_add_f16 %[hs], %[h], %[g] clamp"
                                 : [h] "=&v"(hv), [hs] "+v"(hsv), [s] "=&v"(sv), [t] "=&v"(tv)
                                 : [d] "v"(h2_u32(d[k])), [u] "v"(h2_u32(u[k])), [thi] "s"(thi[k]), [tlo] "v"(tlo[k]), [sel] "v"(sel[r]), [g] "s"(g));
                    const half2_t h = h2_bits(hv), hs = h2_bits(hsv);
                    d[k] = H[r];
                    best = __builtin_elementwise_maximum(best, h);
                    Hs[r] = hs;
                    H[r] = h;
                    u[k] = hs;
                    if (r == R - 1) bot[k] = h;
                }
            }
        }
    }
}

// Task = 128 lane slots of one text: lane l runs slot0 + l (pair A, low halves) and slot0 + 64 + l (pair B, high halves).
template <int R, bool MULTI>
__device__ __forceinline__ void scores16_body(const BatchParams& P) {
    static_assert(R % 4 == 0, "a strip is whole quads of rows");
    const int lane = threadIdx.x & 63;
    int32_t* const hand = P.hand + ((size_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * P.hand_stride;
    const uint32_t g = P.gap16x2;

    for (;;) {
        uint32_t tid = 0;
        {
            int elect = lane;   // (opaque, see batch_scores_kernel)
            asm volatile("" : "+v"(elect));
            if (elect == 0) tid = atomicAdd(P.queue, 1u);
        }
        tid = __builtin_amdgcn_readfirstlane(tid);
        if (tid >= P.n_tasks) break;

        const BatchTask task = P.tasks[tid];
        const int m = (int)task.text_len;
        const uint32_t* tx = reinterpret_cast<const uint32_t*>(P.arena + task.text_off);
        const uint32_t slot_a = task.slot0 + lane, slot_b = slot_a + 64;
        const uint32_t poff_a = P.slot_poff[slot_a], poff_b = P.slot_poff[slot_b];
        const int n_a = (int)P.slot_plen[slot_a], n_b = (int)P.slot_plen[slot_b];
        const uint32_t out_a = P.slot_out[slot_a], out_b = P.slot_out[slot_b];
        const int nblk = m >> 2, rem = m & 3;
        // the per-column v_perm table of text code c (codes 4..7 match no pattern code: every byte the mismatch's)
        auto table = [&](uint32_t c, uint32_t& lo, uint32_t& hi) {
            lo = P.lo16_base ^ (uint32_t)((uint64_t)P.lo16_diff << (8 * c));
            hi = P.hi16_base ^ (uint32_t)((uint64_t)P.hi16_diff << (8 * c));
        };

        half2_t best = h2_bits(0u);
        for (int s = 0; s < (int)task.n_strips; ++s) {
            const int row0 = s * R;
            // ---- the strip's row selectors (pA, pA + 4, pB, pB + 4); 12 past a pattern's end (byte 0x00: score +0.0)
            uint32_t sel[R];
            {
                const uint32_t* pa = reinterpret_cast<const uint32_t*>(P.arena + poff_a + row0);
                const uint32_t* pb = reinterpret_cast<const uint32_t*>(P.arena + poff_b + row0);
#pragma unroll
                for (int q = 0; q < R / 4; ++q) {
                    const uint32_t wa = pa[q], wb = pb[q];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int i = row0 + 4 * q + b;
                        const uint32_t ca = (wa >> (8 * b)) & 0xffu, cb = (wb >> (8 * b)) & 0xffu;
                        const uint32_t sa = i < n_a ? ca * 0x0101u + 0x0400u : 0x0c0cu;
                        const uint32_t sb = i < n_b ? cb * 0x0101u + 0x0400u : 0x0c0cu;
                        sel[4 * q + b] = sa | (sb << 16);
                    }
                }
            }
            half2_t H[R], Hs[R];
#pragma unroll
            for (int r = 0; r < R; ++r) H[r] = Hs[r] = h2_bits(0u);
            half2_t topprev = h2_bits(0u);

            // hand-off rows through a buffer descriptor per 4-column block (SGPRs): the lane's byte offset is the one VGPR of every
            // access -- no 64-bit VGPR addresses in the column loop.  The descriptor is rebuilt from a 64-bit wave-uniform block
            // pointer that advances block by block, so no offset grows with the text (a half is m * 256 bytes: a 32-bit block offset
            // would overflow from m = 2^23 on)
            auto rsrc = [](const char* p) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p), (short)0, 0x7fffffff, 0x00020000); };
            const char* hin_blk = reinterpret_cast<const char*>(hand + (size_t)((s + 1) & 1) * P.hand_half);   // block jb + 1 of strip s-1's row
            char* hout_blk = reinterpret_cast<char*>(hand + (size_t)(s & 1) * P.hand_half);                   // block jb of this strip's row
            const bool has_top = s > 0;
            const bool has_bot = s + 1 < (int)task.n_strips;
            const size_t in_stride = has_top ? 1024 : 0, out_stride = has_bot ? 1024 : 0;   // bytes per 4-column block; 0 parks on block 0
            const int lane16 = lane * 16;
            int4 tnext = make_int4(0, 0, 0, 0);
            if (MULTI) tnext = __builtin_bit_cast(int4, __builtin_amdgcn_raw_buffer_load_b128(rsrc(hin_blk), lane16, 0, 0));
            hin_blk += in_stride;
            uint32_t cwn = tx[0];
            // row 0 of the strip above the first is +0.0 (kept opaque like the int32 form's zero)
            uint32_t zero = 0;
            asm volatile("" : "+v"(zero));
            for (int jb = 0; jb < nblk; ++jb) {
                const uint32_t cw = __builtin_amdgcn_readfirstlane(cwn);   // (uniform: the tables below are scalar work)
                const int4 tcur = tnext;
                cwn = tx[jb + 1];   // arena slack makes the over-read safe
                if (MULTI) tnext = __builtin_bit_cast(int4, __builtin_amdgcn_raw_buffer_load_b128(rsrc(hin_blk), lane16, 0, 0));
                hin_blk += in_stride;
                uint32_t tlo[4], thi[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) table((cw >> (8 * k)) & 0xffu, tlo[k], thi[k]);
                half2_t top[4], bot[4];
                {
                    const uint32_t tl[4] = {(uint32_t)tcur.x, (uint32_t)tcur.y, (uint32_t)tcur.z, (uint32_t)tcur.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) top[k] = h2_bits(has_top ? tl[k] : (MULTI ? 0u : zero));
                }
                dp_block16<R, 4>(H, Hs, sel, tlo, thi, top, topprev, bot, best, g);
                if (MULTI) {
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    const u32x4 v = {h2_u32(bot[0]), h2_u32(bot[1]), h2_u32(bot[2]), h2_u32(bot[3])};
                    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc(hout_blk), lane16, 0, 0);
                }
                hout_blk += out_stride;
            }
            if (rem > 0) {
                uint32_t cw = __builtin_amdgcn_readfirstlane(cwn);
                uint32_t t0 = (uint32_t)tnext.x, t1 = (uint32_t)tnext.y, t2 = (uint32_t)tnext.z;
#pragma unroll 1
                for (int k = 0; k < rem; ++k) {
                    uint32_t tlo[1], thi[1];
                    table(cw & 0xffu, tlo[0], thi[0]);
                    cw >>= 8;
                    const half2_t top1[1] = {h2_bits(has_top ? t0 : (MULTI ? 0u : zero))};
                    t0 = t1;
                    t1 = t2;
                    half2_t bot1[1];
                    dp_block16<R, 1>(H, Hs, sel, tlo, thi, top1, topprev, bot1, best, g);
                    if (MULTI) __builtin_amdgcn_raw_buffer_store_b32(h2_u32(bot1[0]), rsrc(hout_blk), lane16 + 4 * k, 0, 0);   // (block nblk)
                }
            }
        }
        // best = k * 2^-11, exact: back to int32 once per task
        if (out_a != 0xffffffffu) P.scores[out_a] = (int)((float)best.x * 2048.0f);
        if (out_b != 0xffffffffu) P.scores[out_b] = (int)((float)best.y * 2048.0f);
    }
}

// ---------------------------------------------------------------------------------------------------
// PROF16: the profile form of the packed f16 local cells.  Same admission as CELL16, plus every text code in 0..3.  A wave task is
// ONE pattern (wave-uniform) against 128 texts: lane l runs text slot slot0 + l in the low halves and slot0 + 64 + l in the high
// halves, each lane streaming its own two texts (pad code 12 past a text's end, the LANES argument: local scores only decay).  The
// whole pattern is ONE strip of R rows: no hand-off.  Task fields: text_off / n_strips = the pattern's arena offset / length,
// text_len = the longest text of the task.
// Stored value per row: G = h + g (one register instead of CELL16's H and Hs).  With s' = s - g the cell is
//   t' = clamp(G_diag + s')         = max(0, h_diag + s)          v_pk_add_f16 clamp, s' read through VGPR index mode
//   h  = max3(t', G_up, G_left)      = max(0, diag, up + g, left + g), hw2.cpp:211
//   G  = h + g                                                     v_pk_add_f16
//   best = max3(best, h, h')         (half a v_pk_maximum3_f16 per row)
// = 3.5 VALU per lane row of two pairs (CELL16: 4.5).  Exactness as CELL16: every h, t' and G is k * 2^-11 with |k| <= 2047
// (G >= g >= -127), and h_diag + s <= longest pattern * match <= 2047 keeps t' below the clamp's 1.
// Per block of 8 columns the lane builds the profile: register 8 sigma + k holds f16x2(s'(sigma, c_A,k), s'(sigma, c_B,k)) (one
// v_perm per register from the pattern code's byte tables), sigma = 4 is +0.0 for the pad rows past the pattern's end (s = g: pad
// rows only decay).  The 40 registers are pinned (v216..v255) because a row step reads them relative to the row's code x 8: the 8
// diagonal adds sit between s_set_gpr_idx_on (SRC1) and s_set_gpr_idx_off, and nothing else does.  Then the 8 maxima and gap adds
// of the row step, a chain across the block's columns that the second wave on the SIMD covers ([gpu] tools/valu_issue.hip, rows
// "SW pk16 profile").
//
// INT = true, the integer-coded row (the host admits it when mismatch - gap >= 0 and match - gap >= 0, pwalign.hip): the stored
// value is H itself (>= 0) as the INTEGER k in each 16-bit half.  For 0 <= k < 0x7c00 the pattern k read as f16 is a non-negative
// finite number (a denormal below 0x0400; the kernel's mode keeps f16 denormals) whose f16 order is the integer order, so
// v_pk_maximum3_f16 is an exact packed unsigned max3 and the only f16 instruction left.  With gamma = -gap >= 0, s' = s + gamma:
//   t = H_diag + s'                   v_add_u32: ONE 32-bit add for both halves (t <= 2047 + 254: no carry), s' through index mode
//   m = max3(t, H_up, H_left)         = gamma + max(diag + s, up + g, left + g)
//   H = max(m - gamma, 0)             v_pk_sub_u16 clamp          = max(0, diag + s, up + g, left + g), hw2.cpp:211
//   best = max3(best, m, m')          score = max(best - gamma, 0) once per task, in integers
// Boundary row and column are 0, pad rows and pad columns take s' = 0 (s = g: they only decay; their m never exceeds a real
// cell's).  s' <= 254 is one byte: a profile register is one v_perm from the code's 4-byte table, the high byte of each half 0x00.
// The 8 adds issue at the full rate, the other 20 of the row step's 28 at the packed rate ([gpu] tools/valu_issue.hip, row
// "SW pk16 profile C=8 int").  The kernel's own shape -- no v_mov, the last column's subtract deferred into the next row's step -- is
// that tool's row "... int nomove" (DESIGN.md r05, r06).  Neither row runs the pad rows past the pattern's length rounded up to a pair of rows.
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

// The integer row's asm text in pieces (scores16p_body, INT = true).  P16I_ADDS: a row's profile offset and its 8 indexed adds, DIAG
// the first column's diagonal; P16I_CHAIN: its maxima and subtracts, LEFT the row's left neighbour and UPL the last column's "up";
// the forms ending in 0 are row 0's, whose diagonal and "up" operands are the boundary's constant 0 (it writes u0..u6 and pd without
// reading them); P16I_ROW1: the second row of a pair, whole.
#define P16I_ADDS(IDX, FLD, DIAG)                        \
    "s_bfe_u32 %[" IDX "], %[pw], %[" FLD "]\n\t"         \
    "s_set_gpr_idx_on %[" IDX "], gpr_idx(SRC1)\n\t"     \
    "v_add_u32 %[t0], " DIAG ", v216\n\t"                \
    "v_add_u32 %[t1], %[u0], v217\n\t"                   \
    "v_add_u32 %[t2], %[u1], v218\n\t"                   \
    "v_add_u32 %[t3], %[u2], v219\n\t"                   \
    "v_add_u32 %[t4], %[u3], v220\n\t"                   \
    "v_add_u32 %[t5], %[u4], v221\n\t"                   \
    "v_add_u32 %[t6], %[u5], v222\n\t"                   \
    "v_add_u32 %[t7], %[u6], v223\n\t"                   \
    "s_set_gpr_idx_off"
#define P16I_ADDS0(IDX, FLD)                             \
    "s_bfe_u32 %[" IDX "], %[pw], %[" FLD "]\n\t"         \
    "s_set_gpr_idx_on %[" IDX "], gpr_idx(SRC1)\n\t"     \
    "v_add_u32 %[t0], 0, v216\n\t"                       \
    "v_add_u32 %[t1], 0, v217\n\t"                       \
    "v_add_u32 %[t2], 0, v218\n\t"                       \
    "v_add_u32 %[t3], 0, v219\n\t"                       \
    "v_add_u32 %[t4], 0, v220\n\t"                       \
    "v_add_u32 %[t5], 0, v221\n\t"                       \
    "v_add_u32 %[t6], 0, v222\n\t"                       \
    "v_add_u32 %[t7], 0, v223\n\t"                       \
    "s_set_gpr_idx_off"
#define P16I_CHAIN(LEFT, UPL)                                    \
    "v_pk_maximum3_f16 %[t0], %[t0], %[u0], " LEFT "\n\t"        \
    "v_pk_sub_u16 %[u0], %[t0], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[t1], %[t1], %[u1], %[u0]\n\t"           \
    "v_pk_sub_u16 %[u1], %[t1], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[b0], %[b0], %[t0], %[t1]\n\t"           \
    "v_pk_maximum3_f16 %[t2], %[t2], %[u2], %[u1]\n\t"           \
    "v_pk_sub_u16 %[u2], %[t2], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[t3], %[t3], %[u3], %[u2]\n\t"           \
    "v_pk_sub_u16 %[u3], %[t3], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[b1], %[b1], %[t2], %[t3]\n\t"           \
    "v_pk_maximum3_f16 %[t4], %[t4], %[u4], %[u3]\n\t"           \
    "v_pk_sub_u16 %[u4], %[t4], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[t5], %[t5], %[u5], %[u4]\n\t"           \
    "v_pk_sub_u16 %[u5], %[t5], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[b2], %[b2], %[t4], %[t5]\n\t"           \
    "v_pk_maximum3_f16 %[t6], %[t6], %[u6], %[u5]\n\t"           \
    "v_pk_sub_u16 %[u6], %[t6], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[pd], %[t7], " UPL ", %[u6]\n\t"         \
    "v_pk_maximum3_f16 %[b3], %[b3], %[t6], %[pd]"
#define P16I_CHAIN0                                              \
    "v_pk_maximum3_f16 %[t0], %[t0], 0, %[c0]\n\t"               \
    "v_pk_sub_u16 %[u0], %[t0], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[t1], %[t1], 0, %[u0]\n\t"               \
    "v_pk_sub_u16 %[u1], %[t1], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[b0], %[b0], %[t0], %[t1]\n\t"           \
    "v_pk_maximum3_f16 %[t2], %[t2], 0, %[u1]\n\t"               \
    "v_pk_sub_u16 %[u2], %[t2], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[t3], %[t3], 0, %[u2]\n\t"               \
    "v_pk_sub_u16 %[u3], %[t3], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[b1], %[b1], %[t2], %[t3]\n\t"           \
    "v_pk_maximum3_f16 %[t4], %[t4], 0, %[u3]\n\t"               \
    "v_pk_sub_u16 %[u4], %[t4], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[t5], %[t5], 0, %[u4]\n\t"               \
    "v_pk_sub_u16 %[u5], %[t5], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[b2], %[b2], %[t4], %[t5]\n\t"           \
    "v_pk_maximum3_f16 %[t6], %[t6], 0, %[u5]\n\t"               \
    "v_pk_sub_u16 %[u6], %[t6], %[g] clamp\n\t"                  \
    "v_pk_maximum3_f16 %[pd], %[t7], 0, %[u6]\n\t"               \
    "v_pk_maximum3_f16 %[b3], %[b3], %[t6], %[pd]"
#define P16I_ROW1 P16I_ADDS("i1", "f1", "%[c0]") "\n\t" "v_pk_sub_u16 %[c0], %[pd], %[g] clamp\n\t" P16I_CHAIN("%[l1]", "%[c0]")
// ... and its operands (r, t, i0, i1, u, best, col, pw, g and the profile registers p0..p3, pz of the body)
#define P16I_TMPS                                                                                                                \
    [t0] "=&v"(t[0]), [t1] "=&v"(t[1]), [t2] "=&v"(t[2]), [t3] "=&v"(t[3]), [t4] "=&v"(t[4]), [t5] "=&v"(t[5]), [t6] "=&v"(t[6]), \
        [t7] "=&v"(t[7]), [i0] "=&s"(i0), [i1] "=&s"(i1)
#define P16I_UPS(CON) \
    [u0] CON(u[0]), [u1] CON(u[1]), [u2] CON(u[2]), [u3] CON(u[3]), [u4] CON(u[4]), [u5] CON(u[5]), [u6] CON(u[6])
#define P16I_BEST [b0] "+v"(best[0]), [b1] "+v"(best[1]), [b2] "+v"(best[2]), [b3] "+v"(best[3])
#define P16I_INS                                                                                                                    \
    [l1] "v"(col[r + 1 < R ? r + 1 : r]), [pw] "s"(pw[r >> 2]), [f0] "i"((8 * (r & 3)) | (8 << 16)), [f1] "i"((8 * ((r + 1) & 3)) | (8 << 16)), \
        [g] "s"(g), "{v[216:223]}"(p0), "{v[224:231]}"(p1), "{v[232:239]}"(p2), "{v[240:247]}"(p3), "{v[248:255]}"(pz)

// The leading column blocks of a PROF16 task that load their texts without word()'s clamp and pad merge: block jb prefetches bytes
// 8 jb + 8 .. 8 jb + 15 of every lane's two texts, which are whole words inside every text while 8 jb + 16 <= the task's shortest
__host__ __device__ constexpr int prof16_interior_blocks(int min_len) { return min_len >= 16 ? min_len / 8 - 1 : 0; }

template <int R, bool INT>
__device__ __forceinline__ void scores16p_body(const BatchParams& P) {
    constexpr int C = 8, NW = (R + 3) / 4;
    const int lane = threadIdx.x & 63;
    const uint32_t g = P.gap16x2;   // INT: gamma | gamma << 16
    // the pattern code sigma's byte tables (s' = s - g): bytes 0..3 = low / high bytes of f16(s'(sigma, c)) for text codes c = 0..3
    // (INT: the byte s' itself in tlo; no high bytes)
    uint32_t tlo[4], thi[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        tlo[s] = P.lo16_base ^ (P.lo16_diff << (8 * s));
        thi[s] = INT ? 0u : P.hi16_base ^ (P.hi16_diff << (8 * s));
    }
    u32x8 pz = {0, 0, 0, 0, 0, 0, 0, 0};   // sigma = 4: the pad rows' +0.0
    asm volatile("" : "+v"(pz));

    for (;;) {
        uint32_t tid = 0;
        {
            int elect = lane;   // (opaque, see batch_scores_kernel)
            asm volatile("" : "+v"(elect));
            if (elect == 0) tid = atomicAdd(P.queue, 1u);
        }
        tid = __builtin_amdgcn_readfirstlane(tid);
        if (tid >= P.n_tasks) break;

        const BatchTask task = P.tasks[tid];
        const int m = (int)task.text_len;
        const int n = (int)task.n_strips;
        // the pattern's codes x 8 (the row's profile offset), 4 to a word, 32 past the pattern's end; wave-uniform (SGPRs).  The
        // arena's slack covers the over-read of a pattern shorter than R.
        uint32_t pw[NW];
        {
            const uint32_t* pp = reinterpret_cast<const uint32_t*>(P.arena + task.text_off);
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                const int valid = n - 4 * q;
                const uint32_t keep = valid >= 4 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u));
                pw[q] = __builtin_amdgcn_readfirstlane(((pp[q] & keep) | (0x04040404u & ~keep)) << 3);
            }
        }
        const uint32_t slot_a = task.slot0 + lane, slot_b = slot_a + 64;
        const uint32_t toff_a = P.slot_toff[slot_a], toff_b = P.slot_toff[slot_b];
        const int ma = (int)P.slot_tlen[slot_a], mb = (int)P.slot_tlen[slot_b];
        // the lane's text word w (4 columns from column 4w), codes past the text's end replaced by the pad code 12; the load never
        // leaves the text (the arena's slack covers the rounding to whole dwords)
        auto word = [&](uint32_t toff, int ml, int w) -> uint32_t {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(P.arena + toff + 4u * (uint32_t)min(w, max((ml - 1) >> 2, 0)));
            const int valid = ml - 4 * w;
            const uint32_t keep = valid >= 4 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u));
            return (v & keep) | (0x0c0c0c0cu & ~keep);
        };

        // The leading column blocks whose prefetch needs neither the clamp nor the pad merge of word(): block jb loads bytes 8 jb + 8
        // .. 8 jb + 15 of both texts, whole words inside every text of the task up to its shortest one (the host gives an empty slot
        // the task's shortest text, pwalign.hip).  Wave-uniform, so the choice below is a scalar branch around the loads alone: both
        // kinds of block run the one copy of the row code.
        // (The f16 row keeps word() for every block: its register allocation is tight enough that the second kind of load moves it.)
        int nint = 0;
        if constexpr (INT) {
            int mn = min(ma, mb);
            for (int o = 32; o; o >>= 1) mn = min(mn, __shfl_xor(mn, o));
            nint = prof16_interior_blocks(__builtin_amdgcn_readfirstlane(mn));
        }

        // G of the left boundary column (H = 0): g in every row (INT: H = 0)
        const uint32_t edge = INT ? 0u : g;
        uint32_t col[R];
#pragma unroll
        for (int r = 0; r < R; ++r) col[r] = edge;
        uint32_t best[4] = {0, 0, 0, 0};
        const int nblk = (m + C - 1) / C;
        uint32_t na0 = word(toff_a, ma, 0), na1 = word(toff_a, ma, 1);
        uint32_t nb0 = word(toff_b, mb, 0), nb1 = word(toff_b, mb, 1);
        for (int jb = 0; jb < nblk; ++jb) {
            const uint32_t wa[2] = {na0, na1}, wb[2] = {nb0, nb1};
            if (INT && jb < nint) {
                const uint32_t* const qa = reinterpret_cast<const uint32_t*>(P.arena + (toff_a + 8u * (uint32_t)jb + 8u));
                const uint32_t* const qb = reinterpret_cast<const uint32_t*>(P.arena + (toff_b + 8u * (uint32_t)jb + 8u));
                na0 = qa[0];
                na1 = qa[1];
                nb0 = qb[0];
                nb1 = qb[1];
            } else {
                na0 = word(toff_a, ma, 2 * jb + 2);
                na1 = word(toff_a, ma, 2 * jb + 3);
                nb0 = word(toff_b, mb, 2 * jb + 2);
                nb1 = word(toff_b, mb, 2 * jb + 3);
            }
            // the block's profile: selector (cA, cA | 4, cB, cB | 4) per column, then one v_perm per code
            // (INT: selector (cA, 12, cB, 12) -- byte 12 selects 0x00 -- into the one table.  The 12 has to be a source byte of the
            // perm that makes the selector, and the two text words fill both sources: so one perm gathers two columns' codes
            // (cA, cA', cB, cB'), and each column's perm takes its two of them and the low byte of the inline constant 12: three
            // perms per two columns, no v_or)
            u32x8 p0, p1, p2, p3;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const uint32_t kk = (uint32_t)(k & 3);
                uint32_t sel;
                if constexpr (INT) {
                    const uint32_t two = __builtin_amdgcn_perm(wb[k >> 2], wa[k >> 2], kk < 2 ? 0x05040100u : 0x07060302u);
                    sel = __builtin_amdgcn_perm(12u, two, 0x04020400u + (kk & 1u) * 0x00010001u);
                } else {
                    sel = __builtin_amdgcn_perm(wb[k >> 2], wa[k >> 2], kk * 0x00000101u + (4u + kk) * 0x01010000u) | 0x04000400u;
                }
                p0[k] = __builtin_amdgcn_perm(thi[0], tlo[0], sel);
                p1[k] = __builtin_amdgcn_perm(thi[1], tlo[1], sel);
                p2[k] = __builtin_amdgcn_perm(thi[2], tlo[2], sel);
                p3[k] = __builtin_amdgcn_perm(thi[3], tlo[3], sel);
            }
            // row -1 (H = 0): G_up = g in every column, and the diagonal of row 0's first column (INT: row 0's text takes the
            // constant 0 for them and writes u[])
            uint32_t u[C];
            if constexpr (!INT) {
#pragma unroll
                for (int k = 0; k < C; ++k) u[k] = edge;
            }
            if constexpr (INT) {
                // The move-free row, two rows to an asm text.  The last column's subtract of a row is deferred into the next row's
                // step (pend = its m, still due): row r first reads the OLD col[r - 1] as its diagonal, then the deferred subtract
                // writes col[r - 1] in place, and the row's last column takes it as "up".  Row 0 has neither (its diagonal and its
                // last "up" are the boundary's 0).  28 VALU per row, no v_mov.
                // Pad rows are not run: a pair whose first row is past the pattern's end (its profile offset is 32 = the pad code
                // 4 x 8, exactly the rows r >= n; wave-uniform) branches over the rest of its text, so a task runs n rounded up to
                // 2 rows.  The test sits behind the pair's first adds and the deferred subtract, so the rows that run pay one s_cmp
                // and a not-taken branch per pair and no taken branch, and the first skipped pair has thereby done the pending
                // subtract of the last row that ran; a later skipped pair writes the col of a pad row, which no real row reads
                // (each costs 9 VALU and a taken branch instead of 56).  A branch in the C++ loop instead (an exit per pair) makes
                // the compiler copy u[] and best[] at every exit: 11 v_mov per pair.
                static_assert(R % 2 == 0, "the integer row runs its rows in pairs");
                uint32_t pend;
#pragma unroll
                for (int r = 0; r < R; r += 2) {
                    uint32_t t[C], i0, i1;
                    if (r == 0) {
                        asm volatile(P16I_ADDS0("i0", "f0") "\n\t" P16I_CHAIN0 "\n\t" P16I_ROW1
                                     : P16I_TMPS, P16I_UPS("=&v"), P16I_BEST, [pd] "=&v"(pend), [c0] "+v"(col[r])
                                     : P16I_INS
                                     : "m0", "scc");
                    } else {
                        asm volatile(P16I_ADDS("i0", "f0", "%[cp]") "\n\t"
                                     "v_pk_sub_u16 %[cp], %[pd], %[g] clamp\n\t"
                                     "s_cmp_eq_u32 %[i0], 32\n\t"
                                     "s_cbranch_scc1 .Lpad%=\n\t"
                                     P16I_CHAIN("%[c0]", "%[cp]") "\n\t" P16I_ROW1 "\n"
                                     ".Lpad%=:"
                                     : P16I_TMPS, P16I_UPS("+v"), P16I_BEST, [pd] "+v"(pend), [c0] "+v"(col[r]), [cp] "+v"(col[r > 0 ? r - 1 : 0])
                                     : P16I_INS
                                     : "m0", "scc");
                    }
                }
                // the last row's pending subtract, when no pair was skipped (otherwise col[R - 1] is a pad row's)
                asm volatile("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(col[R - 1]) : "v"(pend), "s"(g));
            } else {
                // the f16 row keeps its per-row v_mov of the block's last G; it skips the same pairs of pad rows, row by row
                uint32_t dprev = edge, tst = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // the row's profile offset on the scalar unit, right before its row step (left to the compiler, all 152 are
                    // computed ahead and spill to VGPR lanes: one v_readlane_b32 per row)
                    uint32_t idx;
                    asm volatile("s_bfe_u32 %0, %1, %2" : "=s"(idx) : "s"(pw[r >> 2]), "i"((8 * (r & 3)) | (8 << 16)) : "scc");
                    if ((r & 1) == 0) tst = idx;   // rows 2k and 2k + 1 go by row 2k's offset, rows 0 and 1 always run (33: no offset)
                    const uint32_t left = col[r];
                    uint32_t t[C];
                    asm volatile(
                        "s_cmp_eq_u32 %[tst], %[pc]\n\t"
                        "s_cbranch_scc1 .Lpad%=\n\t"
                        "s_set_gpr_idx_on %[idx], gpr_idx(SRC1)\n\t"
                        "v_pk_add_f16 %[t0], %[d], v216 clamp\n\t"
                        "v_pk_add_f16 %[t1], %[u0], v217 clamp\n\t"
                        "v_pk_add_f16 %[t2], %[u1], v218 clamp\n\t"
                        "v_pk_add_f16 %[t3], %[u2], v219 clamp\n\t"
                        "v_pk_add_f16 %[t4], %[u3], v220 clamp\n\t"
                        "v_pk_add_f16 %[t5], %[u4], v221 clamp\n\t"
                        "v_pk_add_f16 %[t6], %[u5], v222 clamp\n\t"
                        "v_pk_add_f16 %[t7], %[u6], v223 clamp\n\t"
                        "s_set_gpr_idx_off\n\t"
                        "v_pk_maximum3_f16 %[t0], %[t0], %[u0], %[l]\n\t"
                        "v_pk_add_f16 %[u0], %[t0], %[g]\n\t"
                        "v_pk_maximum3_f16 %[t1], %[t1], %[u1], %[u0]\n\t"
                        "v_pk_add_f16 %[u1], %[t1], %[g]\n\t"
                        "v_pk_maximum3_f16 %[b0], %[b0], %[t0], %[t1]\n\t"
                        "v_pk_maximum3_f16 %[t2], %[t2], %[u2], %[u1]\n\t"
                        "v_pk_add_f16 %[u2], %[t2], %[g]\n\t"
                        "v_pk_maximum3_f16 %[t3], %[t3], %[u3], %[u2]\n\t"
                        "v_pk_add_f16 %[u3], %[t3], %[g]\n\t"
                        "v_pk_maximum3_f16 %[b1], %[b1], %[t2], %[t3]\n\t"
                        "v_pk_maximum3_f16 %[t4], %[t4], %[u4], %[u3]\n\t"
                        "v_pk_add_f16 %[u4], %[t4], %[g]\n\t"
                        "v_pk_maximum3_f16 %[t5], %[t5], %[u5], %[u4]\n\t"
                        "v_pk_add_f16 %[u5], %[t5], %[g]\n\t"
                        "v_pk_maximum3_f16 %[b2], %[b2], %[t4], %[t5]\n\t"
                        "v_pk_maximum3_f16 %[t6], %[t6], %[u6], %[u5]\n\t"
                        "v_pk_add_f16 %[u6], %[t6], %[g]\n\t"
                        "v_pk_maximum3_f16 %[t7], %[t7], %[u7], %[u6]\n\t"
                        "v_pk_add_f16 %[u7], %[t7], %[g]\n\t"
                        "v_pk_maximum3_f16 %[b3], %[b3], %[t6], %[t7]\n"
                        ".Lpad%=:"
                        : [t0] "=&v"(t[0]), [t1] "=&v"(t[1]), [t2] "=&v"(t[2]), [t3] "=&v"(t[3]), [t4] "=&v"(t[4]), [t5] "=&v"(t[5]),
                          [t6] "=&v"(t[6]), [t7] "=&v"(t[7]), [u0] "+v"(u[0]), [u1] "+v"(u[1]), [u2] "+v"(u[2]), [u3] "+v"(u[3]),
                          [u4] "+v"(u[4]), [u5] "+v"(u[5]), [u6] "+v"(u[6]), [u7] "+v"(u[7]), [b0] "+v"(best[0]), [b1] "+v"(best[1]),
                          [b2] "+v"(best[2]), [b3] "+v"(best[3])
                        : [d] "v"(dprev), [l] "v"(left), [idx] "s"(idx), [tst] "s"(tst), [pc] "i"(r < 2 ? 33 : 32), [g] "s"(g),
                          "{v[216:223]}"(p0), "{v[224:231]}"(p1), "{v[232:239]}"(p2), "{v[240:247]}"(p3), "{v[248:255]}"(pz)
                        : "m0", "scc");
                    dprev = left;
                    col[r] = u[C - 1];
                }
            }
        }
        const uint32_t out_a = P.slot_out[slot_a], out_b = P.slot_out[slot_b];   // (read here: no VGPRs held over the column loop)
        if constexpr (INT) {
            // best = gamma + the score (or less than gamma where no cell is positive), an integer per half
            const int gamma = (int)(g & 0xffffu);
            const int ba = (int)max(max(best[0] & 0xffffu, best[1] & 0xffffu), max(best[2] & 0xffffu, best[3] & 0xffffu));
            const int bb = (int)max(max(best[0] >> 16, best[1] >> 16), max(best[2] >> 16, best[3] >> 16));
            if (out_a != 0xffffffffu) P.scores[out_a] = max(ba - gamma, 0);
            if (out_b != 0xffffffffu) P.scores[out_b] = max(bb - gamma, 0);
        } else {
            // best = k * 2^-11, exact: back to int32 once per task
            const half2_t b = __builtin_elementwise_maximum(__builtin_elementwise_maximum(h2_bits(best[0]), h2_bits(best[1])),
                                                            __builtin_elementwise_maximum(h2_bits(best[2]), h2_bits(best[3])));
            if (out_a != 0xffffffffu) P.scores[out_a] = (int)((float)b.x * 2048.0f);
            if (out_b != 0xffffffffu) P.scores[out_b] = (int)((float)b.y * 2048.0f);
        }
    }
}

// R = 152 rows at two waves per SIMD: R + 40 profile + the block's columns and temporaries fit in 256 VGPRs
template <int R, bool INT = false>
__global__ __launch_bounds__(256, 2) void batch_scores16p_kernel(const BatchParams P) {
    scores16p_body<R, INT>(P);
}

// MULTI = false: every task of the launch is a single strip -- the hand-off row accesses are compiled out
// (with them, each wave parks an unconditional 1 KiB load + store per 4 columns on an L2-resident dummy
// block: harmless for speed, but it shows up as ~45 MB of HBM traffic per C3 launch).
//
// LANES = true (local alignment only): the 64 pairs of a task do not share a text -- the shape of the reference's
// own loop, pattern i against reference i (hw2.cpp:328-338).  Every lane streams its own text (one dword per
// 4-column block, prefetched a block ahead), the symbol splat moves from the scalar unit to four v_perm_b32, and
// columns past a lane's own text are fed the symbol that matches nothing: local scores can then only decay, so
// the lane's maximum is already final (the same argument that pads short patterns).  ~+3 % VALU per cell
// against the shared-text form, against up to 64x fewer idle lanes on index-paired lists.
// Launch geometry: workgroups of ONE or of FOUR waves (the host's choice); every wave pulls its own tasks and owns its own hand-off region.
// Four-wave workgroups that each ask for a share of the CU's LDS are how the host gets a BALANCED placement -- the same number of
// waves on every SIMD -- whatever kernel ran before ([gpu, r03] tools/probes/simd_place2.hip: single-wave workgroups launched after
// another kernel double up on some SIMDs and leave others empty).
//
// CELL16 = true (BM_SWS, SC_PERM only): two pairs per lane in packed f16 cells (scores16_body above), 128 lane slots per task.
template <int R, int MODE, int SCORE, bool MULTI, bool LANES = false, bool CELL16 = false>
__global__ __launch_bounds__(256, strip_waves_per_simd(R, MODE)) void batch_scores_kernel(const BatchParams P) {
    static_assert(!CELL16 || (MODE == BM_SWS && SCORE == SC_PERM && !LANES), "packed f16 cells: the saturating SW form, shared texts");
    if constexpr (CELL16) {
        scores16_body<R, MULTI>(P);
        return;
    }
    // Global alignment, gap-shifted form, coded alphabets of <= 4 symbols: the texts of a task are RIGHT-aligned.  The
    // host stores every lane's text as a row of M = 4*ceil(max m / 4) codes, front-padded with code 4, which the
    // table scores like a gap (H-space g, here -g): with g <= 0 such a column reproduces column 0 exactly
    // (H[i][j] = i*g), so a lane's real matrix simply starts p = M - m columns late, every lane ends in the last
    // block, and H[n][m] = G'[n][M] + g(n + M).  Only row 0 differs per lane: H[0][j] = g * max(j - p, 0).
    static_assert(!LANES || MODE == BM_SWS || MODE == BM_SW || MODE == BM_NWG, "per-lane texts: SW forms and gap-shifted NW");
    static_assert(R % 4 == 0, "a strip is whole quads of rows (one packed symbol word each)");
    constexpr int Q = R / 4;
    const int lane = threadIdx.x & 63;
    int32_t* const hand = P.hand + ((size_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * P.hand_stride;

    for (;;) {
        uint32_t tid = 0;
        {
            // The electing lane id is made opaque on every trip: with a plain `lane == 0` hipcc threads
            // this branch together with a later `if (lane == 0)` of the previous trip, lane 0 then loops
            // apart from lanes 1..63 and the readfirstlane below no longer sees lane 0 (observed: hang).
            int elect = lane;
            asm volatile("" : "+v"(elect));
            if (elect == 0) tid = atomicAdd(P.queue, 1u);
        }
        tid = __builtin_amdgcn_readfirstlane(tid);
        if (tid >= P.n_tasks) break;

        const BatchTask task = P.tasks[tid];
        const int m = (int)task.text_len;
        const uint32_t* tx = reinterpret_cast<const uint32_t*>(P.arena + task.text_off);
        const uint32_t slot = task.slot0 + lane;
        const uint32_t poff = P.slot_poff[slot];
        const int n = (int)P.slot_plen[slot];
        const uint32_t outi = P.slot_out[slot];
        // LANES: task.text_len is the longest text of the task; all columns run as full, masked blocks
        const int nblk = LANES ? (m + 3) >> 2 : m >> 2, rem = LANES ? 0 : m & 3;
        const uint32_t* txl = tx;
        int ml = m, last_dw = 0;
        if (LANES) {
            txl = reinterpret_cast<const uint32_t*>((MODE == BM_NWG ? P.lane_text : P.arena) + P.slot_toff[slot]);
            ml = (int)P.slot_tlen[slot];
            last_dw = ml > 0 ? (ml - 1) >> 2 : 0;   // loads never leave the lane's own text (+ arena slack)
        }
        const int front_pad = LANES && MODE == BM_NWG ? 4 * nblk - ml : 0;   // p: columns ahead of the lane's own text
        // the lane's text word for block jb, symbols past the text replaced by the pad symbol
        auto lane_word = [&](int jb) -> uint32_t {
            if (MODE == BM_NWG) return txl[min(jb, nblk - 1)];   // pre-padded row of 4 * nblk codes
            const uint32_t w = txl[min(jb, last_dw)];
            const int valid = ml - 4 * jb;
            const uint32_t keep = valid >= 4 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u));
            return (w & keep) | (P.tpad_word & ~keep);
        };

        int best = 0;
        int nw_score = 0;

        for (int s = 0; s < (int)task.n_strips; ++s) {
            const int row0 = s * R;
            // ---- this strip's pattern symbols, padded past the pattern's end
            uint32_t pk[Q];
            {
                const uint32_t* pp = reinterpret_cast<const uint32_t*>(P.arena + poff + row0);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int valid = n - (row0 + 4 * q);   // symbols of this dword inside the pattern
                    uint32_t w = pp[q];
                    const uint32_t keep = valid >= 4 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u));
                    pk[q] = (w & keep) | (P.pad_word & ~keep);
                }
            }
            // ---- column 0 of the strip (hw2.cpp:125-130; SW: zeros, 193)
            int H[R], Hs[MODE == BM_SWS ? R : 1];
#pragma unroll
            for (int r = 0; r < R; ++r) H[r] = (MODE == BM_NW) ? mulw(row0 + r + 1, P.gap) : 0;
#pragma unroll
            for (int r = 0; r < (MODE == BM_SWS ? R : 1); ++r) Hs[r] = 0;
            int topprev = (MODE == BM_NW) ? mulw(row0, P.gap) : 0;

            const int32_t* hin = hand + (size_t)((s + 1) & 1) * P.hand_half;   // written by strip s-1
            int32_t* hout = hand + (size_t)(s & 1) * P.hand_half;
            const bool has_top = s > 0;
            const bool has_bot = s + 1 < (int)task.n_strips;

            const size_t in_stride = has_top ? 64 : 0, out_stride = has_bot ? 64 : 0;
            const int4* hin4 = reinterpret_cast<const int4*>(hin) + lane;
            int4* hout4 = reinterpret_cast<int4*>(hout) + lane;
            int4 tnext = make_int4(0, 0, 0, 0);
            if (MULTI) tnext = hin4[0];
            uint32_t cwn = LANES ? lane_word(0) : tx[0];
            // single-strip form: row 0 is 0, but as a literal it makes hipcc split the first row's v_max3_i32 into
            // unsigned/signed v_max pairs that no longer fuse (+0.7 VALU per cell, [asm]); keep the zero opaque
            int zero = 0;
            asm volatile("" : "+v"(zero));
            for (int jb = 0; jb < nblk; ++jb) {
                const uint32_t cw = cwn;
                const int4 tcur = tnext;
                cwn = LANES ? lane_word(jb + 1) : tx[jb + 1];   // arena slack makes the over-read safe
                if (MULTI) tnext = hin4[(size_t)(jb + 1) * in_stride];
                int top[4], bot[4];
                uint32_t cs[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (LANES && SCORE == SC_PERM) {
                        cs[k] = __builtin_amdgcn_perm(cw, cw, 0x01010101u * (uint32_t)k);   // byte k in all four bytes
                    } else {
                        const uint32_t c = (cw >> (8 * k)) & 0xffu;
                        cs[k] = (SCORE == SC_PERM) ? c * 0x01010101u : c;
                    }
                }
                {
                    const int tl[4] = {tcur.x, tcur.y, tcur.z, tcur.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        int row0v = (MODE == BM_NW) ? mulw(4 * jb + k + 1, P.gap) : (MULTI ? 0 : zero);   // hw2.cpp:131-136
                        if (LANES && MODE == BM_NWG) row0v = mulw(min(4 * jb + k + 1, front_pad), -P.gap);   // G' of H[0][j] = g*max(j-p,0)
                        top[k] = has_top ? tl[k] : row0v;
                    }
                }
                dp_block<R, 4, MODE, SCORE>(H, Hs, pk, cs, top, topprev, bot, best, P);
                if (MULTI) hout4[(size_t)jb * out_stride] = make_int4(bot[0], bot[1], bot[2], bot[3]);
            }
            if (rem > 0) {
                uint32_t cw = cwn;
                int t0 = tnext.x, t1 = tnext.y, t2 = tnext.z;
#pragma unroll 1
                for (int k = 0; k < rem; ++k) {
                    const uint32_t c = cw & 0xffu;
                    cw >>= 8;
                    const uint32_t cs1[1] = {(SCORE == SC_PERM) ? c * 0x01010101u : c};
                    const int top1[1] = {has_top ? t0 : ((MODE == BM_NW) ? mulw(4 * nblk + k + 1, P.gap) : (MULTI ? 0 : zero))};
                    t0 = t1;
                    t1 = t2;
                    int bot1[1];
                    dp_block<R, 1, MODE, SCORE>(H, Hs, pk, cs1, top1, topprev, bot1, best, P);
                    if (MULTI) hout[((size_t)nblk * out_stride + lane) * 4 + k] = bot1[0];
                }
            }
            // ---- NW: dp[n][m] sits in this strip for the lanes whose pattern ends here (hw2.cpp:186)
            if (MODE != BM_SW && MODE != BM_SWS) {
                const int rl = n - 1 - row0;
                if (rl >= 0 && rl < R) {
                    int v = 0;
#pragma unroll
                    for (int r = 0; r < R; ++r) v = (rl == r) ? H[r] : v;
                    nw_score = v;
                }
            }
        }
        if (outi != 0xffffffffu) {
            int sc = best;
            if (MODE == BM_NW) sc = nw_score;
            if (MODE == BM_NWG) sc = addw(nw_score, mulw(n + m, P.gap));
            P.scores[outi] = sc;
        }
    }
}

}  // namespace pwa
