// subst_table.h -- the sizes the substitution-matrix kernels (subst_fill.hip.h) and the host units (pwalign_internal.h) share.
#pragma once

namespace pwa {

constexpr int kSubstMaxSym = 32;                              // codes 0 .. 31
constexpr int kSubstTabWords = kSubstMaxSym * kSubstMaxSym;   // the table in LDS: n_sym rows of `stride` <= 32 entries
constexpr int kSubstMapWords = 64;                            // the device blob: the 256-byte code map, then the table [text code][pattern code]

}  // namespace pwa
