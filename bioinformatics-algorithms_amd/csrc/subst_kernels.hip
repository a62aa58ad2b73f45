// subst_kernels.hip -- the substitution-matrix fills of pwa_align_subst_batch and their band-less form for pwa_subst_batch_create
// (subst_fill.hip.h): the gotoh classes -- 16 lanes per pair for rl in kMiniRL, 64 lanes per pair for rl = 8 | 16 -- in modes
// PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG.  The walk is gotoh_walk_kernel (gotoh_kernels.hip).  Own translation unit.
#include "subst_fill.hip.h"

namespace pwa {

typedef void (*subst_kernel_t)(const PairParams, const uint32_t*, int, int);

template <int RL, int LN>
static subst_kernel_t subst_pick(int mode, bool band) {
    if (!band) return mode == 0 ? subst_scores_kernel<RL, 0, LN> : mode == 1 ? subst_scores_kernel<RL, 1, LN> : mode == 2 ? subst_scores_kernel<RL, 2, LN> : nullptr;
    return mode == 0 ? subst_fill_kernel<RL, 0, LN> : mode == 1 ? subst_fill_kernel<RL, 1, LN> : mode == 2 ? subst_fill_kernel<RL, 2, LN> : nullptr;
}

static subst_kernel_t subst_kernel_for(int rl, int mode, int ln, bool band) {
    return gotoh_for_class(rl, ln, [&](auto rlc, auto lnc) { return subst_pick<decltype(rlc)::value, decltype(lnc)::value>(mode, band); });
}

subst_kernel_t subst_fill_kernel_for(int rl, int mode, int ln) { return subst_kernel_for(rl, mode, ln, true); }
subst_kernel_t subst_scores_kernel_for(int rl, int mode, int ln) { return subst_kernel_for(rl, mode, ln, false); }

}  // namespace pwa
