// pair_dist_kernels.hip -- the stripe engine's hw4 distance fill (pair_dist.hip.h).  Own translation unit: compiles next to
// pair_kernels.hip and the strip units.
#include "kernel_table.h"
#include "pair_dist.hip.h"

namespace pwa {

pair_kernel_t pair_dist_kernel_for(int rl, int w) {
    if (rl == 2) return w == 1 ? pair_dist_kernel<2, 1> : pair_dist_kernel<2, 4>;
    if (rl == 4) return w == 1 ? pair_dist_kernel<4, 1> : pair_dist_kernel<4, 4>;
    return nullptr;
}

}  // namespace pwa
