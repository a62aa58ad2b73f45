// pair_affine_kernels.hip -- the stripe engine's hw3 affine score fill (pair_affine.hip.h).  Own translation unit: compiles next to
// pair_kernels.hip, pair_dist_kernels.hip and the strip units.
#include "kernel_table.h"
#include "pair_affine.hip.h"

namespace pwa {

pair_kernel_t pair_affine_kernel_for(int rl, int w) {
    if (rl == 2) return w == 1 ? pair_affine_kernel<2, 1> : pair_affine_kernel<2, 4>;
    if (rl == 4) return w == 1 ? pair_affine_kernel<4, 1> : pair_affine_kernel<4, 4>;
    return nullptr;
}

}  // namespace pwa
