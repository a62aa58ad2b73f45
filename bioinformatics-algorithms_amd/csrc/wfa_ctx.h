// wfa_ctx.h -- what the wavefront-alignment unit (wfa_kernels.hip) needs of a pwa_ctx, whose layout lives in pwalign_internal.h.
#pragma once
#include "side_unit.h"

namespace pwa {
// the last pwa_scores_wfa / pwa_align_wfa_batch(_cigar) or one of their codes and semi-global forms: device ms of the sweeps and of the walks (events, summed over the ranges), the
// wavefront cells of its pairs up to each pair's penalty (or bound), the bytes of the largest range's wavefront workspace
struct WfaStats {
    float sweep_ms = 0.f, walk_ms = 0.f;
    uint64_t cells = 0, workspace_bytes = 0;
};
struct WfaCtxView : UnitCtx {
    uint64_t range_bytes = 0;        // PWA_RANGE_BYTES (0: the library's budget)
    WfaStats* stats = nullptr;
};
WfaCtxView wfa_ctx_view(pwa_ctx* c);
const WfaStats& wfa_stats_of(const pwa_ctx* c);
}  // namespace pwa

#pragma GCC visibility push(hidden)
namespace pwa {
// defined in wfa_kernels.hip, behind the range planner it checks; pwa_selftest_host ends with it
int selftest_wfa_plan(uint64_t x, int check);
}  // namespace pwa
#pragma GCC visibility pop
