// sufarr_ctx.h -- what the suffix-array unit (sufarr_kernels.hip) needs of a pwa_ctx, whose layout lives in pwalign.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

struct pwa_ctx;

namespace pwa {
struct SaCtxView {
    int device = 0;
    hipStream_t stream = nullptr;
    bool debug = false;              // PWA_DEBUG
    uint64_t occ_chunk_hits = 0;     // PWA_OCC_CHUNK_HITS (0: the library's budget)
    std::string* err = nullptr;      // the context's last-error text
};
SaCtxView sa_ctx_view(pwa_ctx* c);
}  // namespace pwa
