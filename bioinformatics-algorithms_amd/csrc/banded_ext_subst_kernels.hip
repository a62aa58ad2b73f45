// banded_ext_subst_kernels.hip -- the EXT forms of the banded affine-gap fill and score pass under a caller-supplied substitution
// matrix, of pwa_extend_banded_subst_batch(_cigar) and pwa_scores_extend_banded_subst (include/pwalign.h has the semantics, DESIGN.md
// §3.17 the figures): extension from the anchor (0, 0) over NW's banded matrix, free end, given up at the first row that falls xdrop
// below the best, with the pattern-end record (the maximum of row n and its first column) beside the best cell.
//
// Nothing of the sweep is new: banded_body / banded_scores_body with MODE = kBandedExt (banded_fill.hip.h, banded_scores.hip.h) and
// the SubstTableScore policy over a static SubstLds that banded_subst_load<kBandedExt, KEYS> fills (banded_subst.hip.h).
// GotohPrio<kBandedExt> and gotoh_const<kBandedExt> are NW's (E = 1, F = 0), so the table holds s * 8 + 2 * D - cE for the fill and
// the plain s - oe for the pass exactly as it does for PWA_MODE_NW, and the walk is banded_walk_kernel<RL, 0>.
//
// The pattern-end record.  The two bodies are instantiated with PEND = true (the byte-compare EXT kernels leave it false and compile
// the record out).  PairDesc::rows (unused by the banded class otherwise) points at the pair's {score, j} record, which the host has
// set to "no value".  After the test of the stripe that holds row n has found no stop -- no earlier stripe did, or the wave
// would have left the loop --, and if row n has an in-band cell (n <= m - lo), the lane whose row slot is row n writes the row's own
// record there (banded_ext_pattern_end): once per pair, nothing per step.
//
// Every table read is in bounds: banded_subst.hip.h's argument, re-checked for the EXT form.
//   * diag() is still evaluated for every cell of every step regardless of the mask; what EXT changes in the chunk is the key of an
//     out-of-band cell (kBandedExtNone in place of 0) and the missing zero floor, neither of which is an operand of diag();
//   * po: rs[r] is sc.slot()'s result and nothing else; row slots past n are code 0, and banded_ext_stripe_end / banded_ext_pattern_end
//     keep them out of every record by their `i_first + r <= n` / `== n` tests;
//   * tn: built as before from the initial tch = 0 of each stripe and the lanes' tcv = sc.text()'s results, each
//     min(map[b], n_sym - 1) * stride * 4 with b a byte of the staged word.  The early `break` out of the stripe loop only ends the
//     sequence of stripes: a stripe that runs is run whole, with its own tch = 0 and its own staging (clamped to the text's last
//     16-byte block + 16 as before), so no tch / tcv value exists that the NW form could not have produced;
//   * so the word read is ct * stride + cp <= (n_sym - 1) (stride + 1) < n_sym * stride <= kSubstTabWords, with the kernels clamping
//     n_sym and stride to 1 <= n_sym <= stride <= 32 (banded_subst_clamp).
// The two sentinel arguments for this combination, with A = max(max |submat|, |gap_open| + |gap_extend|, 1) and the host admitting a
// pair only while (n + m + 2) A < 2^27:
//   * §3.15's, with A from the table: a real H, E or F is a sum of at most n + m + 1 steps of magnitude <= A, so |V| < 2^27 - A.  The
//     fill's sentinel key -2^31 + 8 A + 1 (banded_body derives it from G.match / G.mismatch = +- max |submat|) is below every key
//     V * 8 + 0..7 and meets at most one gap extension (>= -8 A) before the sum is compared and dropped; the pass's kBandedSent = -2^30
//     is below every V and V + oe.  The diagonal addend of an in-band cell is a table entry of magnitude <= A on a real dg.  Only |s|
//     enters the bound: asymmetric tables and positive off-diagonal entries change nothing.
//   * §3.16's kBandedExtNone: the row key is H * 16 + (15 - q) with H of either sign; |H| <= (n + m) A < 2^27 - 2 A keeps it strictly
//     inside int32 and above kBandedExtNone = INT_MIN, and kBandedExtNone >> 4 = -2^27 is below every real H.  best - xdrop cannot wrap:
//     0 <= best < 2^27, xdrop <= 2^27.  pend[0] = key >> 4 is that real H.
// One wave per pair, stripes of 64 x 4 or 64 x 8 rows.  Own translation unit.
#include "banded_subst.hip.h"

namespace pwa {

// The fill: G.gap = gap_open, G.gap_extend = gap_extend, G.match / G.mismatch = +- max |submat| (banded_body's sentinel reads them).
// Dynamic LDS: kBandedWaves * row_cap * 8 bytes, as banded_fill_kernel.
template <int RL>
__global__ __launch_bounds__(64 * kBandedWaves) void banded_ext_subst_fill_kernel(const PairParams G, const int row_cap, const int xdrop, const uint32_t* blob,
                                                                                 int n_sym, int stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_ext_subst_lds[];
    __shared__ SubstLds L;
    banded_subst_clamp(n_sym, stride);
    banded_subst_load<kBandedExt, true>(L, G, blob, n_sym, stride);
    banded_body<RL, kBandedExt, true>(G, row_cap, SubstTableScore{L, n_sym - 1, stride * 4}, (lds_bint2*)banded_ext_subst_lds, xdrop);
}

// The score pass: G.match / G.mismatch unused.
template <int RL>
__global__ __launch_bounds__(64 * kBandedWaves) void banded_ext_subst_scores_kernel(const PairParams G, const int row_cap, const int xdrop, const uint32_t* blob,
                                                                                   int n_sym, int stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_ext_subst_scores_lds[];
    __shared__ SubstLds L;
    banded_subst_clamp(n_sym, stride);
    banded_subst_load<kBandedExt, false>(L, G, blob, n_sym, stride);
    banded_scores_body<RL, kBandedExt, true>(G, row_cap, SubstTableScore{L, n_sym - 1, stride * 4}, (lds_bint2*)banded_ext_subst_scores_lds, xdrop);
}

// The host stub of the fill (band = true) or of the score pass; rl: 8, else 4 (resolve_banded_form is the only caller).  Both take
// (G, row_cap, xdrop, blob, n_sym, stride).
const void* banded_ext_subst_kernel_for(int rl, bool band) {
    void (*const fn)(const PairParams, const int, const int, const uint32_t*, int, int) =
        band ? (rl == 8 ? banded_ext_subst_fill_kernel<8> : banded_ext_subst_fill_kernel<4>)
             : (rl == 8 ? banded_ext_subst_scores_kernel<8> : banded_ext_subst_scores_kernel<4>);
    return reinterpret_cast<const void*>(fn);
}

}  // namespace pwa
