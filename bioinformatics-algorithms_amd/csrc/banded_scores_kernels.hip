// banded_scores_kernels.hip -- the scores-only banded affine-gap passes of pwa_scores_banded (banded_scores.hip.h): one wave per pair,
// stripes of 64 x 4 or 64 x 8 rows; modes PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG.  Own translation unit.
#include "banded_scores.hip.h"

namespace pwa {

template <int RL>
static const void* banded_scores_pick(int mode) {
    void (*const pass)(const PairParams, const int) = mode == 1 ? banded_scores_kernel<RL, 1> : mode == 2 ? banded_scores_kernel<RL, 2> : banded_scores_kernel<RL, 0>;
    return reinterpret_cast<const void*>(pass);
}

// The host stub of the score pass (banded_kernel_for's conventions; resolve_banded_form is the only caller).
const void* banded_scores_kernel_for(int rl, int mode) { return rl == 8 ? banded_scores_pick<8>(mode) : banded_scores_pick<4>(mode); }

}  // namespace pwa
