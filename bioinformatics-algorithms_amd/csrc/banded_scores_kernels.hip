// banded_scores_kernels.hip -- the scores-only banded affine-gap passes of pwa_scores_banded (banded_scores.hip.h): one wave per pair,
// stripes of 64 x 4 or 64 x 8 rows; modes PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG.  Own translation unit.
#include "banded_scores.hip.h"

#include <algorithm>

namespace pwa {

typedef void (*banded_scores_t)(const PairParams, const int);

template <int RL>
static banded_scores_t banded_scores_pick(int mode) {
    return mode == 0 ? banded_scores_kernel<RL, 0> : mode == 1 ? banded_scores_kernel<RL, 1> : mode == 2 ? banded_scores_kernel<RL, 2> : nullptr;
}

banded_scores_t banded_scores_kernel_for(int rl, int mode) { return rl == 4 ? banded_scores_pick<4>(mode) : rl == 8 ? banded_scores_pick<8>(mode) : nullptr; }

// The scores pass on `st`, nothing after it.  row_cap: the launch's widest band.  The grid is banded_launch's: what the runtime's
// occupancy figure says is resident at once with this launch's hand-off rows in LDS, and no more (pairs are dealt statically, longest
// first).
hipError_t banded_scores_launch(const PairParams& G, int rl, int mode, int row_cap, int num_cu, hipStream_t st) {
    const banded_scores_t fill = banded_scores_kernel_for(rl, mode);
    if (!fill || row_cap < 1 || row_cap > kBandedMaxWidth || !G.n_pairs || num_cu < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)kBandedWaves * (size_t)row_cap * sizeof(bint2);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fill), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fill), 64 * kBandedWaves, lds)) != hipSuccess) return e;
    const uint32_t n_wg = (G.n_pairs + kBandedWaves - 1) / kBandedWaves;
    const uint32_t grid = std::min<uint32_t>(n_wg, (uint32_t)num_cu * (uint32_t)std::max(per_cu, 1));
    hipLaunchKernelGGL(fill, dim3(grid), dim3(64 * kBandedWaves), lds, st, G, row_cap);
    return hipGetLastError();
}

}  // namespace pwa
