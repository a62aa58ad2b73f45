// banded_ext_kernels.hip -- the EXT forms of the banded affine-gap fill and score pass, of pwa_extend_banded_batch(_cigar) and
// pwa_scores_extend_banded (banded_fill.hip.h, banded_scores.hip.h: MODE = kBandedExt): extension from the anchor (0, 0) over NW's
// banded matrix, free end, given up at the first row that falls xdrop below the best.  One wave per pair, stripes of 64 x 4 or
// 64 x 8 rows.  The walk is banded_walk_kernel<RL, 0> (banded_kernels.hip): the band is NW's.  Own translation unit.
#include "banded_scores.hip.h"

#include <algorithm>

namespace pwa {

typedef void (*banded_ext_t)(const PairParams, const int, const int);
typedef void (*banded_walk_t)(const PairParams);
banded_walk_t banded_walk_kernel_for(int rl, int mode);   // banded_kernels.hip

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

static banded_ext_t banded_ext_kernel_for(int rl, bool band) {
    if (!band) return rl == 4 ? banded_ext_scores_kernel<4> : rl == 8 ? banded_ext_scores_kernel<8> : nullptr;
    return rl == 4 ? banded_ext_fill_kernel<4> : rl == 8 ? banded_ext_fill_kernel<8> : nullptr;
}

// The grid is banded_launch's: what the runtime's occupancy figure says is resident at once with this launch's hand-off rows in LDS,
// and no more (pairs are dealt statically, longest first).
static hipError_t banded_ext_fill_launch(banded_ext_t fill, const PairParams& G, int row_cap, int num_cu, hipStream_t st, int xdrop) {
    if (!fill || row_cap < 1 || row_cap > kBandedMaxWidth || !G.n_pairs || num_cu < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)kBandedWaves * (size_t)row_cap * sizeof(bint2);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fill), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fill), 64 * kBandedWaves, lds)) != hipSuccess) return e;
    const uint32_t n_wg = (G.n_pairs + kBandedWaves - 1) / kBandedWaves;
    const uint32_t grid = std::min<uint32_t>(n_wg, (uint32_t)num_cu * (uint32_t)std::max(per_cu, 1));
    hipLaunchKernelGGL(fill, dim3(grid), dim3(64 * kBandedWaves), lds, st, G, row_cap, xdrop);
    return hipGetLastError();
}

// Fill, then NW's walk from the end cells the fill left (one wave per pair), on `st`; `after_fill` is recorded between them.
// row_cap: the launch's widest band.
hipError_t banded_ext_launch(const PairParams& G, int rl, int row_cap, int num_cu, hipStream_t st, hipEvent_t after_fill, int xdrop) {
    const banded_walk_t walk = banded_walk_kernel_for(rl, 0);
    if (!walk) return hipErrorInvalidValue;
    hipError_t e = banded_ext_fill_launch(banded_ext_kernel_for(rl, true), G, row_cap, num_cu, st, xdrop);
    if (e != hipSuccess) return e;
    if (after_fill && (e = hipEventRecord(after_fill, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(walk, dim3(G.n_pairs), dim3(64), 0, st, G);
    return hipGetLastError();
}

// The score pass on `st`, nothing after it.
hipError_t banded_ext_scores_launch(const PairParams& G, int rl, int row_cap, int num_cu, hipStream_t st, int xdrop) {
    return banded_ext_fill_launch(banded_ext_kernel_for(rl, false), G, row_cap, num_cu, st, xdrop);
}

}  // namespace pwa
