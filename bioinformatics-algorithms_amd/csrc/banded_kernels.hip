// banded_kernels.hip -- the banded affine-gap fills and walks of pwa_align_banded_batch (banded_fill.hip.h): one wave per pair, stripes
// of 64 x 4 or 64 x 8 rows; modes PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG.  Own translation unit.
#include "banded_fill.hip.h"

namespace pwa {

template <int RL>
static const void* banded_pick(int mode, bool walk) {
    void (*const fill)(const PairParams, const int) = mode == 1 ? banded_fill_kernel<RL, 1> : mode == 2 ? banded_fill_kernel<RL, 2> : banded_fill_kernel<RL, 0>;
    void (*const wk)(const PairParams) = mode == 1 ? banded_walk_kernel<RL, 1> : mode == 2 ? banded_walk_kernel<RL, 2> : banded_walk_kernel<RL, 0>;
    return walk ? reinterpret_cast<const void*>(wk) : reinterpret_cast<const void*>(fill);
}

// The host stub of the fill, or of the walk over its band (one wave per pair).  rl: 8, else 4; mode: SW, SG, else NW --
// resolve_banded_form (pwalign_ctx.hip) is the only caller and refuses everything else.
const void* banded_kernel_for(int rl, int mode, bool walk) { return rl == 8 ? banded_pick<8>(mode, walk) : banded_pick<4>(mode, walk); }

}  // namespace pwa
