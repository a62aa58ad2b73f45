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
    if (ln == 64) return rl == 8 ? subst_pick<8, 64>(mode, band) : rl == 16 ? subst_pick<16, 64>(mode, band) : nullptr;
    if (ln != 16) return nullptr;
    switch (rl) {
        case 4: return subst_pick<4, 16>(mode, band);
        case 6: return subst_pick<6, 16>(mode, band);
        case 8: return subst_pick<8, 16>(mode, band);
        case 10: return subst_pick<10, 16>(mode, band);
        case 12: return subst_pick<12, 16>(mode, band);
        case 16: return subst_pick<16, 16>(mode, band);
        default: return nullptr;
    }
}

subst_kernel_t subst_fill_kernel_for(int rl, int mode, int ln) { return subst_kernel_for(rl, mode, ln, true); }
subst_kernel_t subst_scores_kernel_for(int rl, int mode, int ln) { return subst_kernel_for(rl, mode, ln, false); }

}  // namespace pwa
