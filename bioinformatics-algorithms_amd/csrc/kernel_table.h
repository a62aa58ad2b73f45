// kernel_table.h -- the instantiated strip kernels (strip_kernels.hip) and pair-engine kernels (pair_kernels.hip) as
// seen by the host units (pwalign*.hip).  Three translation units so that the device code compiles in parallel.
#pragma once
#include "batch_scores.hip.h"
#include "batch_affine.hip.h"
#include "batch_gotoh.hip.h"
#include "batch_nwdist.hip.h"
#include "pair_fill.hip.h"
#include "mini_fill.hip.h"

namespace pwa {

typedef void (*batch_kernel_t)(const BatchParams);
typedef void (*affine_kernel_t)(const AffineParams);
typedef void (*nwdist_kernel_t)(const NwDistParams);
typedef void (*pair_kernel_t)(const PairParams);
enum { BM_AFF = 3, BM_AFFS = 4, BM_DIST = 5, BM_DISTP = 7 };   // affine (hw3) plain / shifted, hw4 NW + distance, its packed-key form; 0..2, 6: batch_scores.hip.h; 8..10: batch_gotoh.hip.h
struct BatchKernelEntry {
    int R, mode, score;
    batch_kernel_t fn;       // multi-strip form (strip hand-off rows through HBM)
    const char* name;
    affine_kernel_t afn = nullptr;            // hw3's affine kernels, and the gotoh score kernels (BM_GNW, BM_GNWS, BM_GSW)
    nwdist_kernel_t dfn = nullptr;
    batch_kernel_t fn_single = nullptr;   // every task a single strip: no hand-off accesses at all
    batch_kernel_t fn_lanes = nullptr;         // every lane its own text (index-paired lists), multi-strip
    batch_kernel_t fn_lanes_single = nullptr;  // ... every task a single strip
    batch_kernel_t fn_cell16 = nullptr;        // two pairs per lane in packed f16 cells (BM_SWS, SC_PERM), multi-strip
    batch_kernel_t fn_cell16_single = nullptr; // ... every task a single strip
    batch_kernel_t fn_prof16 = nullptr;        // ... their profile form: one pattern against 128 texts per task (PROF16, single strip)
    batch_kernel_t fn_prof16_int = nullptr;    // ... with the integer-coded row (mismatch >= gap and match >= gap)
};
// strip_kernels.hip
const BatchKernelEntry* batch_kernel_table(size_t* count);
const BatchKernelEntry* find_batch_kernel(int R, int mode, int score);
// pair_kernels.hip
// perm: coded sequences, table scoring (keyed tb only); keyed = false: the plain int32 traceback form (RL = 4 only)
// gap0: global fill in gap-shifted coordinates (the host passes gap 0 and scores s - 2 gap): perm && keyed && !sband only
// semi = true: the semi-global form of the same fills and walks (local = false, no gap0, no overlap walk; pair_fill.hip.h, SEMI)
pair_kernel_t pair_fill_kernel_for(int rl, int w, bool local, bool tb, bool sband, bool perm, bool keyed = true, bool gap0 = false, bool band = true,
                                   bool semi = false);   // band = false: keyed, table scoring, no band at all
pair_kernel_t pair_traceback_kernel_for(int rl, bool local, int walk, bool semi = false);   // walk: WALK_NONE / WALK_OPS / WALK_OVERLAP
// pair_dist_kernels.hip -- hw4's NW distance on the stripe engine (rl = 2 | 4, w = 1 | 4): no band, no walk, D[n][m] straight into
// PairParams::scores_out
pair_kernel_t pair_dist_kernel_for(int rl, int w);
// pair_affine_kernels.hip -- hw3's affine score on the stripe engine (rl = 2 | 4, w = 1 | 4): no band, no walk, M[n][m] straight
// into PairParams::scores_out; PairParams::gap = gap opening, gap_extend = gap extension
pair_kernel_t pair_affine_kernel_for(int rl, int w);
// pair_affine_tb_kernels.hip -- hw3's affine alignment on the stripe engine (rl = 4, w = 1 | 4): the fill writes the traceback band
// (one code byte per cell, batch_affine_tb.hip.h's code) and M[n][m] into PairParams::scores_out; the walk (one wave per pair) the
// op list into PairDesc::ops and its length into PairResult::n_ops
pair_kernel_t pair_affine_tb_kernel_for(int rl, int w);
pair_kernel_t pair_affine_walk_kernel_for(int rl);
// mini_kernels*.hip -- the mini-stripe engine (16 lanes per pair, 4 pairs per wave; keyed cells, table scoring): fills for
// rl in kMiniRL; gap0 only global without score band; the walks over its band geometry (BandGeo<16, rl>)
constexpr int kMiniRL[] = {4, 6, 8, 10, 12, 16};
// ln = 16: four pairs per wave (rl in kMiniRL); ln = 64: one pair per wave, rl = 8 | 16 (single stripes of 512 / 1024 rows; band only)
pair_kernel_t mini_fill_kernel_for(int rl, bool local, bool sband, bool gap0, bool band = true, int ln = 16, bool semi = false);   // band = false: scores (+ end cells) only
pair_kernel_t mini_traceback_kernel_for(int rl, bool local, int walk, int ln = 16, bool semi = false);

}  // namespace pwa
