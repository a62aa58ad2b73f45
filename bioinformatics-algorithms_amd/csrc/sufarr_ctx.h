// sufarr_ctx.h -- what the suffix-array unit (sufarr_kernels.hip) needs of a pwa_ctx, whose layout lives in pwalign_internal.h, and the
// scan of that unit that pwalign_align.hip borrows.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "poison.h"

struct pwa_ctx;

namespace pwa {
struct SaCtxView {
    int device = 0;
    hipStream_t stream = nullptr;
    bool debug = false;              // PWA_DEBUG
    uint64_t occ_chunk_hits = 0;     // PWA_OCC_CHUNK_HITS (0: the library's budget)
    std::string* err = nullptr;      // the context's last-error text
    Poison* poison = nullptr;        // the context's PWA_POISON state: every device allocation of the unit goes through poison_device
};
SaCtxView sa_ctx_view(pwa_ctx* c);
// The suffix-array unit's reduce-then-scan over uint32 (sufarr_kernels.hip), enqueued on s: x[0 .. len) := its exclusive prefix
// sums, in place; part is a device workspace of scan_part_words(len) words.
void scan_excl(hipStream_t s, uint32_t* x, size_t len, uint32_t* part);
size_t scan_part_words(size_t len);
}  // namespace pwa
