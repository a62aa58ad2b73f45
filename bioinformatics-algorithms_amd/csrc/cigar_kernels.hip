// cigar_kernels.hip -- the count and write passes of pwa_align_batch_cigar (cigar.hip.h), launched by align_batch_impl
// (pwalign_align.hip) between a range's walks and its copy back.  Own translation unit.
#include "cigar.hip.h"

namespace pwa {

hipError_t cigar_launch(const CigarParams& p, bool write, hipStream_t s) {
    if (!p.nc) return hipSuccess;
    const uint32_t blocks = (p.nc + cigar::kWaves - 1) / cigar::kWaves;
    if (write)
        cigar_kernel<true><<<blocks, 64 * cigar::kWaves, 0, s>>>(p);
    else
        cigar_kernel<false><<<blocks, 64 * cigar::kWaves, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace pwa
