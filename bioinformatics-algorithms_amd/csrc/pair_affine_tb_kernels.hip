// pair_affine_tb_kernels.hip -- the stripe engine's hw3 affine alignment: fill with a traceback band and the walk
// (pair_affine_tb.hip.h).  Own translation unit: compiles next to pair_affine_kernels.hip and the strip units.
#include "kernel_table.h"
#include "pair_affine_tb.hip.h"

namespace pwa {

pair_kernel_t pair_affine_tb_kernel_for(int rl, int w) {
    if (rl == 4) return w == 1 ? pair_affine_tb_kernel<4, 1> : pair_affine_tb_kernel<4, 4>;
    return nullptr;
}
pair_kernel_t pair_affine_walk_kernel_for(int rl) { return rl == 4 ? pair_affine_walk_kernel<4> : nullptr; }

}  // namespace pwa
