// format_ops.h -- the one host writer of CIGAR and MD:Z (postprocess.cpp), behind pwa_format_alignment and pwa_align_wfa_batch_cigar.
#pragma once
#include <cstdint>

#pragma GCC visibility push(hidden)
namespace pwa {
struct FormatLen {
    uint64_t cigar, mdz;
};
// ops in traceback order (last column first); pattern and text point at the alignment's start cell; any byte value may appear and no
// terminator is written.  cigar needs pwa_cigar_bound(n_ops) bytes, mdz pwa_mdz_bound(n_ops); either may be null (length 0).
FormatLen format_ops(const uint8_t* pattern, const uint8_t* text, const uint8_t* ops, uint64_t n_ops, char* cigar, char* mdz);
}  // namespace pwa
#pragma GCC visibility pop
