// sufarr_ctx.h -- what the suffix-array unit (sufarr_kernels.hip) needs of a pwa_ctx, whose layout lives in pwalign_internal.h, and the
// scan of that unit that pwalign_align.hip borrows.
#pragma once
#include "side_unit.h"

namespace pwa {
struct SaCtxView : UnitCtx {
    uint64_t occ_chunk_hits = 0;     // PWA_OCC_CHUNK_HITS (0: the library's budget)
};
SaCtxView sa_ctx_view(pwa_ctx* c);
// The suffix-array unit's reduce-then-scan over uint32 (sufarr_kernels.hip), enqueued on s: x[0 .. len) := its exclusive prefix
// sums, in place; part is a device workspace of scan_part_words(len) words.
void scan_excl(hipStream_t s, uint32_t* x, size_t len, uint32_t* part);
size_t scan_part_words(size_t len);
}  // namespace pwa
