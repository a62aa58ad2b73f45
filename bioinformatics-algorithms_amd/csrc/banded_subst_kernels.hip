// banded_subst_kernels.hip -- the banded affine-gap fills and score passes under a substitution matrix, of pwa_align_banded_subst_batch
// and pwa_scores_banded_subst (banded_subst.hip.h): one wave per pair, stripes of 64 x 4 or 64 x 8 rows; modes PWA_MODE_NW,
// PWA_MODE_SW, PWA_MODE_SG.  The walk is banded_walk_kernel (banded_kernels.hip).  Own translation unit.
#include "banded_subst.hip.h"

#include <algorithm>

namespace pwa {

typedef void (*banded_subst_t)(const PairParams, const int, const uint32_t*, int, int);
typedef void (*banded_walk_t)(const PairParams);
banded_walk_t banded_walk_kernel_for(int rl, int mode);   // banded_kernels.hip

template <int RL>
static banded_subst_t banded_subst_pick(int mode, bool band) {
    if (!band) return mode == 0 ? banded_subst_scores_kernel<RL, 0> : mode == 1 ? banded_subst_scores_kernel<RL, 1> : mode == 2 ? banded_subst_scores_kernel<RL, 2> : nullptr;
    return mode == 0 ? banded_subst_fill_kernel<RL, 0> : mode == 1 ? banded_subst_fill_kernel<RL, 1> : mode == 2 ? banded_subst_fill_kernel<RL, 2> : nullptr;
}

static banded_subst_t banded_subst_kernel_for(int rl, int mode, bool band) {
    return rl == 4 ? banded_subst_pick<4>(mode, band) : rl == 8 ? banded_subst_pick<8>(mode, band) : nullptr;
}

// Fill (walk = true: then banded_walk_kernel, one wave per pair; `after_fill` is recorded between them) or score pass on `st`.
// row_cap: the launch's widest band.  The grid is banded_launch's: what the runtime's occupancy figure says is resident at once, and no
// more (pairs are dealt statically, longest first).  Only the dynamic LDS -- the hand-off rows -- is named to the runtime; it counts the
// kernel's static table (SubstLds) itself, both for the attribute's limit and for the occupancy figure.
hipError_t banded_subst_launch(const PairParams& G, int rl, int mode, int row_cap, int num_cu, hipStream_t st, hipEvent_t after_fill, bool walk,
                               const uint32_t* blob, int n_sym, int stride) {
    const banded_subst_t fill = banded_subst_kernel_for(rl, mode, walk);
    const banded_walk_t wk = walk ? banded_walk_kernel_for(rl, mode) : nullptr;
    if (!fill || (walk && !wk) || row_cap < 1 || row_cap > kBandedMaxWidth || !G.n_pairs || num_cu < 1) return hipErrorInvalidValue;
    if (!blob || n_sym < 1 || n_sym > kSubstMaxSym || stride < n_sym || stride > kSubstMaxSym) return hipErrorInvalidValue;
    const size_t lds = (size_t)kBandedWaves * (size_t)row_cap * sizeof(bint2);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fill), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fill), 64 * kBandedWaves, lds)) != hipSuccess) return e;
    const uint32_t n_wg = (G.n_pairs + kBandedWaves - 1) / kBandedWaves;
    const uint32_t grid = std::min<uint32_t>(n_wg, (uint32_t)num_cu * (uint32_t)std::max(per_cu, 1));
    hipLaunchKernelGGL(fill, dim3(grid), dim3(64 * kBandedWaves), lds, st, G, row_cap, blob, n_sym, stride);
    if ((e = hipGetLastError()) != hipSuccess || !walk) return e;
    if (after_fill && (e = hipEventRecord(after_fill, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(wk, dim3(G.n_pairs), dim3(64), 0, st, G);
    return hipGetLastError();
}

}  // namespace pwa
