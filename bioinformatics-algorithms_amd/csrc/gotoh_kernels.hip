// gotoh_kernels.hip -- the affine-gap (Gotoh) fills and walks of pwa_align_gotoh_batch (gotoh_fill.hip.h): 16 lanes per pair for
// rl in kMiniRL, 64 lanes per pair for rl = 8 | 16; modes PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG; and the fills' band-less form for
// pwa_gotoh_batch_create (gotoh_scores_kernel, same classes).  Own translation unit.
#include "gotoh_fill.hip.h"

namespace pwa {

typedef void (*gotoh_kernel_t)(const PairParams);

enum { GK_FILL = 0, GK_WALK = 1, GK_SCORES = 2 };

template <int RL, int LN>
static gotoh_kernel_t gotoh_pick(int mode, int walk) {
    if (walk == GK_SCORES)
        return mode == 0 ? gotoh_scores_kernel<RL, 0, LN> : mode == 1 ? gotoh_scores_kernel<RL, 1, LN> : mode == 2 ? gotoh_scores_kernel<RL, 2, LN> : nullptr;
    if (walk)
        return mode == 0 ? gotoh_walk_kernel<RL, 0, LN> : mode == 1 ? gotoh_walk_kernel<RL, 1, LN> : mode == 2 ? gotoh_walk_kernel<RL, 2, LN> : nullptr;
    return mode == 0 ? gotoh_fill_kernel<RL, 0, LN> : mode == 1 ? gotoh_fill_kernel<RL, 1, LN> : mode == 2 ? gotoh_fill_kernel<RL, 2, LN> : nullptr;
}

static gotoh_kernel_t gotoh_kernel_for(int rl, int mode, int ln, int walk) {
    return gotoh_for_class(rl, ln, [&](auto rlc, auto lnc) { return gotoh_pick<decltype(rlc)::value, decltype(lnc)::value>(mode, walk); });
}

gotoh_kernel_t gotoh_fill_kernel_for(int rl, int mode, int ln) { return gotoh_kernel_for(rl, mode, ln, GK_FILL); }
gotoh_kernel_t gotoh_walk_kernel_for(int rl, int mode, int ln) { return gotoh_kernel_for(rl, mode, ln, GK_WALK); }
gotoh_kernel_t gotoh_scores_kernel_for(int rl, int mode, int ln) { return gotoh_kernel_for(rl, mode, ln, GK_SCORES); }

}  // namespace pwa
