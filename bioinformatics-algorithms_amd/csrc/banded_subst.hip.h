// banded_subst.hip.h -- the banded affine-gap fills and score passes of LONG pairs under a caller-supplied substitution matrix
// (gfx950 / MI355X): pwa_align_banded_subst_batch(_cigar) and pwa_scores_banded_subst (include/pwalign.h has the semantics, DESIGN.md
// §3.15 the figures).
//
// Nothing of the sweep is new.  The alignment fill is banded_body (banded_fill.hip.h) and the score pass banded_scores_body
// (banded_scores.hip.h), unchanged and shared with the byte-compare kernels: stripes, column windows, scalar text staging, the (H, F)
// hand-off row in dynamic LDS, the mask, the end-cell records.  Both reach the diagonal score only through the Score policy hooks
// (gotoh_fill.hip.h), and the policy handed in here is SubstTableScore (subst_fill.hip.h) over a SubstLds that the workgroup fills
// before the sweep:
//   * alignment fill: the table prescaled into KEY form, tab[ct * stride + cp] = s(cp, ct) * 8 + 2 * PR::D - K.cE, as subst_load does;
//   * score pass: its cell adds diag() to H + oe, so the table holds the PLAIN values s(cp, ct) - oe (what BandedValueScore's sM / sX are
//     to match / mismatch);
//   * the loader strides by the banded workgroup's own size, 64 * kBandedWaves threads (subst_load strides by the mini-stripe
//     workgroup's), and copies the 256-byte code map with the same loop: neither constant is assumed to cover the map in one go.
// The row-slot value is the pattern code's column byte offset cp * 4, the travelling text value the byte offset ct * stride * 4 of the
// text code's row: per cell one add and one ds_read_b32 in place of a compare and a select.  The code byte and the band layout are
// banded_fill.hip.h's, so the walk is banded_walk_kernel itself.
//
// LDS.  The static SubstLds (4352 B) sits beside the dynamic hand-off rows (kBandedWaves * row_cap * 8 <= 128 KiB): 135 424 B at the
// widest band, under the CU's 160 KiB.  The launch gives the dynamic part alone to hipFuncSetAttribute and to the occupancy query; the
// runtime adds the kernel's static part itself.
//
// Every table read is in bounds, whatever the mask does with the cell.  With GotohByteScore a stale travelling text value or row slot
// only made a compare false; here both are byte offsets into L.tab, and diag() is evaluated for EVERY cell of every step -- the mask
// (`a`, `started`, `actl`) only selects among results afterwards, so no table read depends on it and none may rely on it.  The claim:
// every value that reaches diag(tn, po) is  tn in {ct * stride * 4 : 0 <= ct < n_sym}  and  po in {cp * 4 : 0 <= cp < n_sym}.  Then the
// word read is ct * stride + cp <= (n_sym - 1) (stride + 1) < n_sym * stride <= kSubstTabWords (stride >= n_sym, both <= 32: the
// kernels clamp the two launch arguments to that), a word the loader wrote.
//   po: rs[r] is sc.slot()'s result and nothing else: min(map[byte], n_sym - 1) * 4 for a row of the pattern, 0 (code 0) for a row past
//       n.  Rows past n feed only rows below them and are kept out of every record by the `i <= n` / `own` / `last` tests.
//   tn: the chunk forms tn from two sources only: lane 0 takes lane q's tcv, lanes 1..63 take lane k - 1's tch (wave_shr:1 never
//       brings in anything else: lane 0's dst is the picked value); and tch becomes tn.  So by induction every tch / tn is either the
//       initial tch, which the body sets to 0 = the offset of code 0's row at the start of every stripe, or some lane's tcv.  tcv is
//       sc.text()'s result and nothing else: min(map[b], n_sym - 1) * stride * 4, with b = one byte of the staged word masked to 0..255,
//       an index inside the 256-byte map.  That holds for whatever byte was staged:
//         - lanes that have not started (t0 + q < k) still shift: they receive lane k - 1's tch -- 0 or an earlier tcv;
//         - lane 0 past column m: the staged address is clamped to the text's last 16-byte block + 16, inside the arena (every sequence
//           is followed by padding); the bytes there are padding or another sequence's, and map + clamp make them a code all the same;
//         - the alignment columns c0a .. c0 - 1 before the window are real text bytes (c0a >= 1);
//         - a byte whose map entry is >= n_sym cannot come from the host (subst_prepare refuses the table) and is clamped regardless.
// The sentinel argument of the two sweeps holds with A = max(max |submat|, |gap_open| + |gap_extend|, 1), the range rule's A for these
// calls ((n + m + 2) A < 2^28).  Alignment fill: banded_body derives SENT = -2^31 + 8 A + 1 from G.match / G.mismatch, which the host
// sets to +- max |submat| for a table launch (they have no other reader here); a real value is a sum of at most n + m + 1 steps of at
// most A each, so its key is above SENT whatever its low bits, and one gap extension (>= -8 A) of SENT stays inside int32.  The diagonal
// addend of an IN-BAND cell is a table entry of magnitude <= A added to a real dg (the diagonal neighbour of an in-band cell is in the
// band), so that sum is real too; an asymmetric table or positive off-diagonal entries change nothing, the bound uses |s| only.  Score
// pass: kBandedSent = -2^30 is below every real value and every real value + oe, and (V + oe) + (s - oe) = V + s stays within
// (n + m + 2) A.  Sums of out-of-band cells may wrap (p_addw); the mask discards them.
#pragma once
#include "banded_scores.hip.h"
#include "subst_fill.hip.h"

namespace pwa {

// The table and the code map into LDS, once per workgroup of 64 * kBandedWaves threads.  KEYS: key form for banded_body, else the plain
// values s - oe for banded_scores_body.  blob: SubstTable's (kSubstMapWords words of code map, then n_sym rows of `stride` raw scores,
// row = text code).
template <int MODE, bool KEYS>
__device__ __forceinline__ void banded_subst_load(SubstLds& L, const PairParams& G, const uint32_t* const blob, const int n_sym, const int stride) {
    constexpr int kThreads = 64 * kBandedWaves;
    const int words = min(n_sym * stride, kSubstTabWords);
    const int kadd = 2 * GotohPrio<MODE>::D - gotoh_const<MODE>(G).cE, oe = p_addw(G.gap, G.gap_extend);
    for (int x = (int)threadIdx.x; x < words; x += kThreads) {
        const int s = (int)blob[kSubstMapWords + x];
        L.tab[x] = KEYS ? p_addw(p_mulw(s, 8), kadd) : p_addw(s, -oe);
    }
    for (int x = (int)threadIdx.x; x < kSubstMapWords; x += kThreads) L.map[x] = blob[x];
    __syncthreads();
}

// n_sym and stride as the policy and the loader may use them: 1 <= n_sym <= stride <= 32 (the host's always are)
__device__ __forceinline__ void banded_subst_clamp(int& n_sym, int& stride) {
    n_sym = min(max(n_sym, 1), kSubstMaxSym);
    stride = min(max(stride, n_sym), kSubstMaxSym);
}

// The fill: G.gap = gap_open, G.gap_extend = gap_extend, G.match / G.mismatch = +- max |submat| (banded_body's sentinel reads them).
// Dynamic LDS: kBandedWaves * row_cap * 8 bytes, as banded_fill_kernel.
template <int RL, int MODE>
__global__ __launch_bounds__(64 * kBandedWaves) void banded_subst_fill_kernel(const PairParams G, const int row_cap, const uint32_t* blob, int n_sym, int stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_subst_lds[];
    __shared__ SubstLds L;
    banded_subst_clamp(n_sym, stride);
    banded_subst_load<MODE, true>(L, G, blob, n_sym, stride);
    banded_body<RL, MODE>(G, row_cap, SubstTableScore{L, n_sym - 1, stride * 4}, (lds_bint2*)banded_subst_lds);
}

// The score pass: G.match / G.mismatch unused.
template <int RL, int MODE>
__global__ __launch_bounds__(64 * kBandedWaves) void banded_subst_scores_kernel(const PairParams G, const int row_cap, const uint32_t* blob, int n_sym, int stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_subst_scores_lds[];
    __shared__ SubstLds L;
    banded_subst_clamp(n_sym, stride);
    banded_subst_load<MODE, false>(L, G, blob, n_sym, stride);
    banded_scores_body<RL, MODE>(G, row_cap, SubstTableScore{L, n_sym - 1, stride * 4}, (lds_bint2*)banded_subst_scores_lds);
}

}  // namespace pwa
