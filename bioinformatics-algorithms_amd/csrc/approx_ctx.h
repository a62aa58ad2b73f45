// approx_ctx.h -- what the approximate-search unit (approx_kernels.hip) needs of a pwa_ctx, whose layout lives in pwalign_internal.h.
#pragma once
#include "side_unit.h"

namespace pwa {
// the last pwa_approx_find / pwa_approx_occurrences: device ms of the count and the fill pass (events), tasks, text columns scanned
struct ApproxStats {
    float count_ms = 0.f, fill_ms = 0.f;
    uint64_t tasks = 0, columns = 0;
};
// the last pwa_approx_starts: device ms of the pass (events), the hits it ran, the text columns they scanned
struct ApproxStartsStats {
    float ms = 0.f;
    uint64_t hits = 0, columns = 0;
};
struct ApproxCtxView : UnitCtx {
    uint32_t chunk = 0;              // PWA_APPROX_CHUNK: most text columns a task reports
    uint64_t occ_chunk_hits = 0;     // PWA_OCC_CHUNK_HITS (0: the library's budget)
    ApproxStats* stats = nullptr;
    ApproxStartsStats* starts_stats = nullptr;
};
ApproxCtxView approx_ctx_view(pwa_ctx* c);
const ApproxStats& approx_stats_of(const pwa_ctx* c);
const ApproxStartsStats& approx_starts_stats_of(const pwa_ctx* c);
// The arena's table kernel (pwalign_ctx.hip), enqueued on s: every byte of the n16 blocks of 16 bytes at p through table[256].
hipError_t recode_bytes(hipStream_t s, uint8_t* p, size_t n16, const uint8_t* table);
}  // namespace pwa
