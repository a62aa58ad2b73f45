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

// The table and the code map into LDS, once per workgroup, the table prescaled into key form (a code past the alphabet cannot come from
// the host: clamped all the same).  blob: kSubstMapWords words of code map, then n_sym rows of `stride` raw scores, row = text code.
template <int MODE>
__device__ __forceinline__ void subst_load(SubstLds& L, const PairParams& G, const uint32_t* const blob, const int n_sym, const int stride) {
    const int words = min(n_sym * stride, kSubstTabWords), kadd = 2 * GotohPrio<MODE>::D - gotoh_const<MODE>(G).cE;
    for (int x = (int)threadIdx.x; x < words; x += 64 * kMiniWaves) L.tab[x] = p_addw(p_mulw((int)blob[kSubstMapWords + x], 8), kadd);
    if (threadIdx.x < (unsigned)kSubstMapWords) L.map[threadIdx.x] = blob[threadIdx.x];
    __syncthreads();
}

// gotoh_body's scoring policy (gotoh_fill.hip.h) over a loaded table: the row-slot value is the pattern code's column byte offset, the
// travelling text value the byte offset of the text code's row.
struct SubstTableScore {
    const SubstLds& L;
    int code_max, row_bytes;
    __device__ __forceinline__ int slot(uint32_t byte, bool in) const {   // rows past n: code 0
        return in ? min((int)reinterpret_cast<const uint8_t*>(L.map)[byte], code_max) * 4 : 0;
    }
    __device__ __forceinline__ int text(uint32_t wv, int k) const {   // the lane's staged text byte -> its code -> that code's row
        return min((int)reinterpret_cast<const uint8_t*>(L.map)[(wv >> ((k & 3) * 8)) & 0xffu], code_max) * row_bytes;
    }
    __device__ __forceinline__ int diag(int tn, int po) const {   // s(cp, ct), as a key addend
        const char* const row = reinterpret_cast<const char*>(L.tab) + tn;
        return *reinterpret_cast<const int*>(row + po);
    }
};

// The fill and its band-less scores form: G.gap = gap_open, G.gap_extend = gap_extend, G.match / G.mismatch unused.
template <int RL, int MODE, int LN>
__global__ __launch_bounds__(64 * kMiniWaves) void subst_fill_kernel(const PairParams G, const uint32_t* blob, int n_sym, int stride) {
    __shared__ SubstLds L;
    subst_load<MODE>(L, G, blob, n_sym, stride);
    gotoh_body<RL, MODE, LN, true>(G, SubstTableScore{L, n_sym - 1, stride * 4});
}

template <int RL, int MODE, int LN>
__global__ __launch_bounds__(64 * kMiniWaves) void subst_scores_kernel(const PairParams G, const uint32_t* blob, int n_sym, int stride) {
    __shared__ SubstLds L;
    subst_load<MODE>(L, G, blob, n_sym, stride);
    gotoh_body<RL, MODE, LN, false>(G, SubstTableScore{L, n_sym - 1, stride * 4});
}

}  // namespace pwa
