// banded_subst_kernels.hip -- the banded affine-gap fills and score passes under a substitution matrix, of pwa_align_banded_subst_batch
// and pwa_scores_banded_subst (banded_subst.hip.h): one wave per pair, stripes of 64 x 4 or 64 x 8 rows; modes PWA_MODE_NW,
// PWA_MODE_SW, PWA_MODE_SG.  The walk is banded_walk_kernel (banded_kernels.hip).  Own translation unit.
#include "banded_subst.hip.h"

namespace pwa {

template <int RL>
static const void* banded_subst_pick(int mode, bool band) {
    void (*const fill)(const PairParams, const int, const uint32_t*, int, int) =
        mode == 1 ? banded_subst_fill_kernel<RL, 1> : mode == 2 ? banded_subst_fill_kernel<RL, 2> : banded_subst_fill_kernel<RL, 0>;
    void (*const pass)(const PairParams, const int, const uint32_t*, int, int) =
        mode == 1 ? banded_subst_scores_kernel<RL, 1> : mode == 2 ? banded_subst_scores_kernel<RL, 2> : banded_subst_scores_kernel<RL, 0>;
    return reinterpret_cast<const void*>(band ? fill : pass);
}

// The host stub of the fill (band = true) or of the score pass (banded_kernel_for's conventions; resolve_banded_form is the only
// caller).  Both take (G, row_cap, blob, n_sym, stride).
const void* banded_subst_kernel_for(int rl, int mode, bool band) { return rl == 8 ? banded_subst_pick<8>(mode, band) : banded_subst_pick<4>(mode, band); }

}  // namespace pwa
