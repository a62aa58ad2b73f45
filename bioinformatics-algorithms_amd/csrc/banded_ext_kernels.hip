// banded_ext_kernels.hip -- the EXT forms of the banded affine-gap fill and score pass, of pwa_extend_banded_batch(_cigar) and
// pwa_scores_extend_banded (banded_fill.hip.h, banded_scores.hip.h: MODE = kBandedExt): extension from the anchor (0, 0) over NW's
// banded matrix, free end, given up at the first row that falls xdrop below the best.  One wave per pair, stripes of 64 x 4 or
// 64 x 8 rows.  The walk is banded_walk_kernel<RL, 0> (banded_kernels.hip): the band is NW's.  Own translation unit.
#include "banded_scores.hip.h"

namespace pwa {

template <int RL>
__global__ __launch_bounds__(64 * kBandedWaves) void banded_ext_fill_kernel(const PairParams G, const int row_cap, const int xdrop) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_ext_lds[];
    banded_body<RL, kBandedExt>(G, row_cap, GotohByteScore<0>(G), (lds_bint2*)banded_ext_lds, xdrop);
}

template <int RL>
__global__ __launch_bounds__(64 * kBandedWaves) void banded_ext_scores_kernel(const PairParams G, const int row_cap, const int xdrop) {
    extern __shared__ __attribute__((aligned(16))) uint8_t banded_ext_lds[];
    banded_scores_body<RL, kBandedExt>(G, row_cap, BandedValueScore(G), (lds_bint2*)banded_ext_lds, xdrop);
}

// The host stub of the fill (band = true) or of the score pass; rl: 8, else 4 (resolve_banded_form is the only caller).  Both take
// (G, row_cap, xdrop).
const void* banded_ext_kernel_for(int rl, bool band) {
    void (*const fn)(const PairParams, const int, const int) = band ? (rl == 8 ? banded_ext_fill_kernel<8> : banded_ext_fill_kernel<4>)
                                                                     : (rl == 8 ? banded_ext_scores_kernel<8> : banded_ext_scores_kernel<4>);
    return reinterpret_cast<const void*>(fn);
}

}  // namespace pwa
