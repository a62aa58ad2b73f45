// chain_ctx.h -- what the chaining unit (chain_kernels.hip) needs of a pwa_ctx, whose layout lives in pwalign_internal.h.
#pragma once
#include "side_unit.h"

namespace pwa {
// the last pwa_chain_anchors: device ms of the chain kernel (events, summed over the ranges), the anchors it chained, the ranges it ran
struct ChainStats {
    float chain_ms = 0.f;
    uint64_t anchors = 0, ranges = 0;
};
// the last pwa_chain_top: device ms of its chain kernel and of what follows it (keys, sort, selection), the anchors, the rounds of
// the selection (walks begun), the ranges
struct ChainTopStats {
    float chain_ms = 0.f, top_ms = 0.f;
    uint64_t anchors = 0, rounds = 0, ranges = 0;
};
struct ChainCtxView : UnitCtx {
    uint64_t range_bytes = 0;        // PWA_RANGE_BYTES (0: the library's budget)
    ChainStats* stats = nullptr;
};
ChainCtxView chain_ctx_view(pwa_ctx* c);
const ChainStats& chain_stats_of(const pwa_ctx* c);
ChainTopStats* chain_top_stats_of(pwa_ctx* c);
}  // namespace pwa
