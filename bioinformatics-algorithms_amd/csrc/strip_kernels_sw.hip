// strip_kernels_sw.hip -- instantiations of the local-alignment strip kernels (plain, saturating, LANES, packed f16).
#include "kernel_table.h"

namespace pwa {

#define BK(R, M, S) {R, M, S, batch_scores_kernel<R, M, S, true>, "batch_scores_kernel<R=" #R "," #M "," #S ">", nullptr, nullptr, \
                     batch_scores_kernel<R, M, S, false>}
#define BKL(R, M, S) {R, M, S, batch_scores_kernel<R, M, S, true>, "batch_scores_kernel<R=" #R "," #M "," #S ">", nullptr, nullptr, \
                      batch_scores_kernel<R, M, S, false>, \
                      batch_scores_kernel<R, M, S, true, true>, batch_scores_kernel<R, M, S, false, true>}
// BKL + the packed f16 form (CELL16) and its profile form (PROF16): the reported name stays the int32 form's, like fn_single's
#define BKL16(R, M, S) {R, M, S, batch_scores_kernel<R, M, S, true>, "batch_scores_kernel<R=" #R "," #M "," #S ">", nullptr, nullptr, \
                        batch_scores_kernel<R, M, S, false>, \
                        batch_scores_kernel<R, M, S, true, true>, batch_scores_kernel<R, M, S, false, true>, \
                        batch_scores_kernel<R, M, S, true, false, true>, batch_scores_kernel<R, M, S, false, false, true>, \
                        batch_scores16p_kernel<152>, batch_scores16p_kernel<152, true>}
extern const BatchKernelEntry kStripKernelsSW[] = {
    BK(76, BM_SW, SC_PERM),   BK(104, BM_SW, SC_PERM),
    BKL(40, BM_SWS, SC_PERM), BKL16(52, BM_SWS, SC_PERM), BKL16(76, BM_SWS, SC_PERM), BKL(96, BM_SWS, SC_PERM),
    BKL(40, BM_SWS, SC_CMP),  BKL(52, BM_SWS, SC_CMP),  BKL(76, BM_SWS, SC_CMP),  BKL(96, BM_SWS, SC_CMP),
    BK(64, BM_SW, SC_PERM),   BK(128, BM_SW, SC_PERM),  BK(152, BM_SW, SC_PERM),
    BK(64, BM_SW, SC_CMP),    BK(128, BM_SW, SC_CMP),   BK(152, BM_SW, SC_CMP),
};
extern const size_t kStripKernelsSWCount = sizeof(kStripKernelsSW) / sizeof(kStripKernelsSW[0]);

}  // namespace pwa
