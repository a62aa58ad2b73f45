// sufarr_ctx.h -- what the suffix-array unit (sufarr_kernels.hip) needs of a pwa_ctx, whose layout lives in pwalign_internal.h, the
// scan of that unit that pwalign_align.hip borrows, and its radix sort of (uint64 key, uint32 value) pairs that chain_kernels.hip borrows.
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
// Scratch of the unit's radix sort for up to n elements: the digit-major histogram, the scan's chunk sums, the key-bit partials.
struct SortScratch {
    Dev hist, part, bits;
    void alloc(Poison* po, size_t n);
};
// The suffix-array unit's stable LSD radix sort (sufarr_kernels.hip) of n (uint64 key, uint32 value) pairs by key, enqueued on s (it
// waits once on s for the key bits that decide which 8-bit passes run).  key2 and val2 hold 2 n entries each: the input in the first
// n, the other n a workspace.  Returns which half (0 or 1) holds the sorted pairs.
int sort_pairs(hipStream_t s, uint64_t* key2, uint32_t* val2, size_t n, SortScratch& sc);
}  // namespace pwa
