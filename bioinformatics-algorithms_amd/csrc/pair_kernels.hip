// pair_kernels.hip -- every instantiation of the wavefront (pair) engine: fill kernels and traceback walks.
// Own translation unit: compiles next to pwalign.hip and strip_kernels.hip.
#include "kernel_table.h"

namespace pwa {

template <int RL, int W>
static pair_kernel_t pair_fill_pick(bool local, bool tb, bool sband, bool perm) {
    if (tb && perm) {   // coded sequences: byte-table scoring
        if (local) return sband ? pair_fill_kernel<RL, W, true, true, true, true> : pair_fill_kernel<RL, W, true, true, false, true>;
        return sband ? pair_fill_kernel<RL, W, false, true, true, true> : pair_fill_kernel<RL, W, false, true, false, true>;
    }
    if (local) {
        if (tb) return sband ? pair_fill_kernel<RL, W, true, true, true> : pair_fill_kernel<RL, W, true, true, false>;
        return pair_fill_kernel<RL, W, true, false, false>;
    }
    if (tb) return sband ? pair_fill_kernel<RL, W, false, true, true> : pair_fill_kernel<RL, W, false, true, false>;
    return pair_fill_kernel<RL, W, false, false, false>;
}
// traceback fill in plain int32 (compare-and-select chains, no packed keys): any scores the reference's `int` holds.
// Rare (scores x lengths beyond 2^28), so only the RL = 4 geometry is instantiated.
template <int W>
static pair_kernel_t pair_fill_pick_plain_tb(bool local, bool sband) {
    if (local) return sband ? pair_fill_kernel<4, W, true, true, true, false, false> : pair_fill_kernel<4, W, true, true, false, false, false>;
    return sband ? pair_fill_kernel<4, W, false, true, true, false, false> : pair_fill_kernel<4, W, false, true, false, false, false>;
}
// the keyed chunk without a band: scores (and end cells) of long pairs over a coded arena (pwalign.hip, batch_create_impl)
template <int RL, int W>
static pair_kernel_t pair_fill_pick_noband(bool local, bool gap0) {
    if (local) return pair_fill_kernel<RL, W, true, true, false, true, true, false, false>;
    return gap0 ? pair_fill_kernel<RL, W, false, true, false, true, true, true, false> : pair_fill_kernel<RL, W, false, true, false, true, true, false, false>;
}
// semi-global (PWA_MODE_SG) fills: every form NW has except the gap-shifted one -- keyed with and without table scoring (and score band),
// keyed without a band (scores), the plain int32 traceback form (RL = 4) and the plain form without a band
template <int RL, int W>
static pair_kernel_t pair_fill_pick_semi(bool tb, bool sband, bool perm, bool keyed, bool band) {
    if (!band) return (tb && keyed && perm && !sband) ? pair_fill_kernel<RL, W, false, true, false, true, true, false, false, true> : nullptr;
    if (!tb) return sband ? nullptr : pair_fill_kernel<RL, W, false, false, false, false, true, false, true, true>;
    if (!keyed) {
        if constexpr (RL == 4) return sband ? pair_fill_kernel<4, W, false, true, true, false, false, false, true, true> : pair_fill_kernel<4, W, false, true, false, false, false, false, true, true>;
        return nullptr;
    }
    if (perm) return sband ? pair_fill_kernel<RL, W, false, true, true, true, true, false, true, true> : pair_fill_kernel<RL, W, false, true, false, true, true, false, true, true>;
    return sband ? pair_fill_kernel<RL, W, false, true, true, false, true, false, true, true> : pair_fill_kernel<RL, W, false, true, false, false, true, false, true, true>;
}
pair_kernel_t pair_fill_kernel_for(int rl, int w, bool local, bool tb, bool sband, bool perm, bool keyed, bool gap0, bool band, bool semi) {
    if (semi) {
        if (local || gap0) return nullptr;
        if (rl == 2) return w == 1 ? pair_fill_pick_semi<2, 1>(tb, sband, perm, keyed, band) : pair_fill_pick_semi<2, 4>(tb, sband, perm, keyed, band);
        return w == 1 ? pair_fill_pick_semi<4, 1>(tb, sband, perm, keyed, band) : pair_fill_pick_semi<4, 4>(tb, sband, perm, keyed, band);
    }
    if (!band) {
        if (!tb || sband || !perm || !keyed) return nullptr;
        if (rl == 2) return w == 1 ? pair_fill_pick_noband<2, 1>(local, gap0) : pair_fill_pick_noband<2, 4>(local, gap0);
        return w == 1 ? pair_fill_pick_noband<4, 1>(local, gap0) : pair_fill_pick_noband<4, 4>(local, gap0);
    }
    if (gap0) {   // gap-shifted global fills: table scoring, keyed, no score band
        if (local || !tb || sband || !perm || !keyed) return nullptr;
        if (rl == 2) return w == 1 ? pair_fill_kernel<2, 1, false, true, false, true, true, true> : pair_fill_kernel<2, 4, false, true, false, true, true, true>;
        return w == 1 ? pair_fill_kernel<4, 1, false, true, false, true, true, true> : pair_fill_kernel<4, 4, false, true, false, true, true, true>;
    }
    if (tb && !keyed) return rl != 4 ? nullptr : (w == 1 ? pair_fill_pick_plain_tb<1>(local, sband) : pair_fill_pick_plain_tb<4>(local, sband));
    if (rl == 2) return w == 1 ? pair_fill_pick<2, 1>(local, tb, sband, perm) : pair_fill_pick<2, 4>(local, tb, sband, perm);
    return w == 1 ? pair_fill_pick<4, 1>(local, tb, sband, perm) : pair_fill_pick<4, 4>(local, tb, sband, perm);
}
template <int RL>
static pair_kernel_t pair_tb_pick(bool local, int walk) {
    if (local)
        return walk == WALK_OPS ? pair_traceback_kernel<RL, true, WALK_OPS>
               : walk == WALK_OVERLAP ? pair_traceback_kernel<RL, true, WALK_OVERLAP> : pair_traceback_kernel<RL, true, WALK_NONE>;
    return walk == WALK_OPS ? pair_traceback_kernel<RL, false, WALK_OPS>
           : walk == WALK_OVERLAP ? pair_traceback_kernel<RL, false, WALK_OVERLAP> : pair_traceback_kernel<RL, false, WALK_NONE>;
}
pair_kernel_t pair_traceback_kernel_for(int rl, bool local, int walk, bool semi) {
    if (semi) {   // (no overlap walk: pwa_overlaps is hw2 -g's selection, global or local)
        if (local || walk == WALK_OVERLAP) return nullptr;
        if (rl == 2) return walk == WALK_OPS ? pair_traceback_kernel<2, false, WALK_OPS, 64, true> : pair_traceback_kernel<2, false, WALK_NONE, 64, true>;
        return walk == WALK_OPS ? pair_traceback_kernel<4, false, WALK_OPS, 64, true> : pair_traceback_kernel<4, false, WALK_NONE, 64, true>;
    }
    return rl == 2 ? pair_tb_pick<2>(local, walk) : pair_tb_pick<4>(local, walk);
}

}  // namespace pwa
