// strip_kernels_gotoh.hip -- instantiations of the affine-gap (gotoh) score strip kernels (batch_gotoh.hip.h).
#include "kernel_table.h"

namespace pwa {

extern const BatchKernelEntry kStripKernelsGotoh[] = {
#define GK(R, M, S) {R, M, S, nullptr, "batch_gotoh_kernel<R=" #R "," #M "," #S ">", batch_gotoh_kernel<R, S, M>}
    GK(32, BM_GNWS, SC_PERM), GK(52, BM_GNWS, SC_PERM), GK(32, BM_GNWS, SC_CMP), GK(52, BM_GNWS, SC_CMP),
    GK(32, BM_GNW, SC_PERM),  GK(52, BM_GNW, SC_PERM),  GK(32, BM_GNW, SC_CMP),  GK(52, BM_GNW, SC_CMP),
    GK(32, BM_GSW, SC_PERM),  GK(52, BM_GSW, SC_PERM),  GK(32, BM_GSW, SC_CMP),  GK(52, BM_GSW, SC_CMP),
#undef GK
};
extern const size_t kStripKernelsGotohCount = sizeof(kStripKernelsGotoh) / sizeof(kStripKernelsGotoh[0]);

}  // namespace pwa
