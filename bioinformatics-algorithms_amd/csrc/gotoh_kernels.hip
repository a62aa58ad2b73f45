// gotoh_kernels.hip -- the affine-gap (Gotoh) fills and walks of pwa_align_gotoh_batch (gotoh_fill.hip.h): 16 lanes per pair for
// rl in kMiniRL, 64 lanes per pair for rl = 8 | 16; modes PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG.  Own translation unit.
#include "gotoh_fill.hip.h"

namespace pwa {

typedef void (*gotoh_kernel_t)(const PairParams);

template <int RL, int LN>
static gotoh_kernel_t gotoh_pick(int mode, bool walk) {
    if (walk)
        return mode == 0 ? gotoh_walk_kernel<RL, 0, LN> : mode == 1 ? gotoh_walk_kernel<RL, 1, LN> : mode == 2 ? gotoh_walk_kernel<RL, 2, LN> : nullptr;
    return mode == 0 ? gotoh_fill_kernel<RL, 0, LN> : mode == 1 ? gotoh_fill_kernel<RL, 1, LN> : mode == 2 ? gotoh_fill_kernel<RL, 2, LN> : nullptr;
}

static gotoh_kernel_t gotoh_kernel_for(int rl, int mode, int ln, bool walk) {
    if (ln == 64) return rl == 8 ? gotoh_pick<8, 64>(mode, walk) : rl == 16 ? gotoh_pick<16, 64>(mode, walk) : nullptr;
    if (ln != 16) return nullptr;
    switch (rl) {
        case 4: return gotoh_pick<4, 16>(mode, walk);
        case 6: return gotoh_pick<6, 16>(mode, walk);
        case 8: return gotoh_pick<8, 16>(mode, walk);
        case 10: return gotoh_pick<10, 16>(mode, walk);
        case 12: return gotoh_pick<12, 16>(mode, walk);
        case 16: return gotoh_pick<16, 16>(mode, walk);
        default: return nullptr;
    }
}

gotoh_kernel_t gotoh_fill_kernel_for(int rl, int mode, int ln) { return gotoh_kernel_for(rl, mode, ln, false); }
gotoh_kernel_t gotoh_walk_kernel_for(int rl, int mode, int ln) { return gotoh_kernel_for(rl, mode, ln, true); }

}  // namespace pwa
