// banded_kernels.hip -- the banded affine-gap fills and walks of pwa_align_banded_batch (banded_fill.hip.h): one wave per pair, stripes
// of 64 x 4 or 64 x 8 rows; modes PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG.  Own translation unit.
#include "banded_fill.hip.h"

#include <algorithm>

namespace pwa {

typedef void (*banded_fill_t)(const PairParams, const int);
typedef void (*banded_walk_t)(const PairParams);

template <int RL>
static banded_fill_t banded_fill_pick(int mode) {
    return mode == 0 ? banded_fill_kernel<RL, 0> : mode == 1 ? banded_fill_kernel<RL, 1> : mode == 2 ? banded_fill_kernel<RL, 2> : nullptr;
}
template <int RL>
static banded_walk_t banded_walk_pick(int mode) {
    return mode == 0 ? banded_walk_kernel<RL, 0> : mode == 1 ? banded_walk_kernel<RL, 1> : mode == 2 ? banded_walk_kernel<RL, 2> : nullptr;
}

banded_fill_t banded_fill_kernel_for(int rl, int mode) { return rl == 4 ? banded_fill_pick<4>(mode) : rl == 8 ? banded_fill_pick<8>(mode) : nullptr; }
banded_walk_t banded_walk_kernel_for(int rl, int mode) { return rl == 4 ? banded_walk_pick<4>(mode) : rl == 8 ? banded_walk_pick<8>(mode) : nullptr; }

// Fill, then the walk (one wave per pair), on `st`; `after_fill` is recorded between them.  row_cap: the launch's widest band.
// The fill's grid is what is resident at once -- the runtime's occupancy figure for this kernel (its VGPRs: 79 .. 248, two to six
// waves per SIMD) with this launch's hand-off rows in LDS -- and no more: pairs are dealt statically, longest first, so a workgroup
// that had to wait for a slot would run its whole share behind the others.
hipError_t banded_launch(const PairParams& G, int rl, int mode, int row_cap, int num_cu, hipStream_t st, hipEvent_t after_fill) {
    const banded_fill_t fill = banded_fill_kernel_for(rl, mode);
    const banded_walk_t walk = banded_walk_kernel_for(rl, mode);
    if (!fill || !walk || row_cap < 1 || row_cap > kBandedMaxWidth || !G.n_pairs || num_cu < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)kBandedWaves * (size_t)row_cap * sizeof(bint2);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fill), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fill), 64 * kBandedWaves, lds)) != hipSuccess) return e;
    const uint32_t n_wg = (G.n_pairs + kBandedWaves - 1) / kBandedWaves;
    const uint32_t grid = std::min<uint32_t>(n_wg, (uint32_t)num_cu * (uint32_t)std::max(per_cu, 1));
    hipLaunchKernelGGL(fill, dim3(grid), dim3(64 * kBandedWaves), lds, st, G, row_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (after_fill && (e = hipEventRecord(after_fill, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(walk, dim3(G.n_pairs), dim3(64), 0, st, G);
    return hipGetLastError();
}

}  // namespace pwa
