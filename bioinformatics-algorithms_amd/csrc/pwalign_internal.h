// pwalign_internal.h -- what the host units of libpwalign.so share (pwalign_ctx.hip: context and memory; pwalign.hip: score
// batches; pwalign_affine_tb.hip: hw3's affine alignments; pwalign_align.hip: alignment batches), declared once.  Not installed; the
// functions of namespace pwa are defined in pwalign_ctx.hip unless noted and have hidden visibility: the library exports the C ABI only.
#pragma once
#include "../../include/pwalign.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "approx_ctx.h"
#include "chain_ctx.h"
#include "dev_mem.h"
#include "kernel_table.h"
#include "poison.h"
#include "subst_table.h"
#include "wfa_ctx.h"

// Host-side source / destination of the library's own host <-> device copies: page-locked, grow-only, kept in the context.
// hipMemcpy from a short-lived pageable vector works, but the runtime registers its pages with the driver for the DMA, and
// when the vector is freed the unmap notifier evicts the process's GPU queues: the NEXT kernel submission then takes 14-24 ms
// [gpu, r02: tools/cold_start.py, PWA_PROBE] -- which is what made the first run of every fresh batch 25 ms late.
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    pwa::Poison* poison = nullptr;   // the owning context's PWA_POISON state (pwa_ctx_create)
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t reserve(size_t n) {   // contents are NOT kept
        if (n > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
            n = (n + (n >> 2) + 4095) & ~(size_t)4095;   // 25 % headroom: few regrowths
            const hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
            if (e != hipSuccess) {
                p = nullptr;
                return e;
            }
            cap = n;
        }
        pwa::poison_host(poison, p, cap);   // PWA_POISON: every reserve, regrown or not
        return hipSuccess;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Test / diagnostic switches (include/pwalign.h, "Environment switches"): environment variables read ONCE, by
// pwa_ctx_create, into the context.  No entry point consults the environment afterwards; a test that wants another
// setting creates a fresh context.
struct Knobs {
    bool debug = false, probe = false;          // PWA_DEBUG, PWA_PROBE: host-side phase times on stderr, nop-kernel probes
    int force_rl = 0, force_w = 0;              // PWA_FORCE_RL (2 | 3 | 4), PWA_FORCE_W (1 | 4): geometry of the stripe engine
    int wg_per_cu = 0;                          // PWA_WG_PER_CU: workgroups per CU of a stripe-engine launch
    bool no_lds_pad = false;                    // PWA_NO_LDS_PAD
    std::string stamps;                         // PWA_STAMPS=<file>: per-stripe time stamps of the fill
    int trace_stripe = -1;                      // PWA_TRACE_STRIPE
    bool no_packed_dist = false;                // PWA_NO_PACKED_DIST: hw4 pass in its two-value form
    int force_lanes = -1;                       // PWA_FORCE_LANES=0: never the per-lane-text kernels
    int force_r = 0, force_mode = -1;           // PWA_FORCE_R, PWA_FORCE_MODE: strip height / kernel form of the strip engine
    uint64_t arena_limit = 0;                   // PWA_ARENA_LIMIT: bytes of sequence arena per run of the one-shot calls (tests)
    uint64_t lane_rows_limit = 0;               // PWA_LANE_ROWS_LIMIT: bytes of per-lane text rows per batch object (tests)
    int mini_per_cu = 0;                        // PWA_MINI_PER_CU: most four-wave workgroups of a mini-stripe fill per CU (experiments; default 2)
    uint64_t range_bytes = 0;                   // PWA_RANGE_BYTES: band + op bytes per range of pwa_align_batch / pwa_overlaps (tests: several ranges on small lists)
    bool no_pair_table = false;                 // PWA_NO_PAIR_TABLE: traceback fills on raw bytes (compare + select)
    bool no_keyed_tb = false;                   // PWA_NO_KEYED_TB: traceback fills in the plain int32 form
    bool no_gap_shift = false;                  // PWA_NO_GAP_SHIFT: global traceback fills in H, not G = H - gap (i + j)
    bool no_tiled_ops = false;                  // PWA_NO_TILED_OPS: op lists through the staging copy
    bool no_pipeline = false;                   // PWA_NO_PIPELINE: the runs of a one-shot score call are processed strictly one after the other
    int pipe_runs = 0;                          // PWA_PIPE_RUNS=N: cut a list that fits one arena into N pipelined runs (experiment; measured slower)
    int scores_route = -1;                      // PWA_SCORES_ROUTE: 0 = every pair on the strip engine, 1 = every pair on the stripe
                                                // engine, unset = by estimated cost (batch_create_impl)
    int affine_tb_route = -1;                   // PWA_AFFINE_TB_ROUTE: pwa_align_affine_batch: 0 = every pair on the strips, 1 = every eligible
                                                // pair on the stripe engine, unset = by estimated cost and band size
    int cell16 = -1;                            // PWA_CELL16: 0 = never the packed f16 cells (two pairs per lane), 1 = always where the batch
                                                // admits them, unset = by estimated cost (batch_create_impl)
    int prof16 = -1;                            // PWA_PROF16: 0 = never the profile form of the packed cells (one pattern against 128
                                                // texts), 1 = always where the batch admits it, unset = by estimated cost
    int prof16_int = -1;                        // PWA_PROF16_INT: 0 = never the profile form's integer-coded row, 1 or unset = wherever the
                                                // scoring admits it (mismatch >= gap and match >= gap)
    uint64_t occ_chunk_hits = 0;                // PWA_OCC_CHUNK_HITS: most raw hits per chunk of pwa_sa_occurrences, most staged hits per slice
                                                // of tasks of pwa_approx_occurrences, most worst-case hits per range of reads of pwa_sa_seed
                                                // (tests: several chunks)
    uint32_t approx_chunk = 4096;               // PWA_APPROX_CHUNK: most text columns one task of pwa_approx_* reports
    int tb_engine = -1;                         // PWA_TB_ENGINE: 0 = stripe engine only, 2 = mini-stripe kernels wherever they exist (also one
                                                // pair per wave for 257 .. 1024 rows, however few such pairs), unset = by pattern length and count
    int banded_rl = 0;                          // PWA_BANDED_RL: 4 | 8 = every banded pair (alignments and scores) on stripes of 64 x 4 / 64 x 8 rows (tests), unset = by band width
    int poison = -1;                            // PWA_POISON=<byte>: every buffer handed to a call reads as that byte until the call writes it (poison.h);
                                                // -2: a value that does not parse, pwa_ctx_create fails
    void read();   // (pwalign_ctx.hip)
};

// Device ms of the fills / walks of a batch of full alignments (event-timed, summed over its launches) and the band bytes they wrote;
// a scores-only banded call: no walk and no band, the in-band cells of its pairs instead
struct AlignStats {
    float fill_ms = 0.f, tb_ms = 0.f;
    uint64_t band_bytes = 0;
    uint64_t cells = 0;
};

// pwa_align_affine_batch: pairs it ran on the stripe engine, device ms of their fills / walks, band bytes written
struct AffineAlignStats {
    uint64_t stripe_pairs = 0, band_bytes = 0;
    float fill_ms = 0.f, walk_ms = 0.f;
};

// ------------------------------------------------------------------------------------ context
struct pwa_ctx {
    Knobs knobs;
    pwa::Poison poison;   // PWA_POISON: the byte and the running totals of pwa_ctx_poison_stats; every acquisition site passes &poison
    int device = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    std::string err;
    AlignStats align_stats, gotoh_stats;   // the last pwa_align_batch / _cigar / pwa_overlaps, the last pwa_align_gotoh_batch(_cigar)
    AlignStats subst_stats;                // the last pwa_align_subst_batch(_cigar)
    AlignStats banded_stats;               // the last pwa_align_banded_batch(_cigar) or pwa_align_banded_subst_batch(_cigar)
    AlignStats banded_scores_stats;        // the last pwa_scores_banded or pwa_scores_banded_subst
    AlignStats ext_stats;                  // the last pwa_extend_banded_batch(_cigar), pwa_scores_extend_banded or a _subst form of them (cells: the sum of rows_out)
    AffineAlignStats aff_stats;            // the last pwa_align_affine_batch
    pwa::ApproxStats approx_stats;         // the last pwa_approx_find / pwa_approx_occurrences
    pwa::ApproxStartsStats approx_starts_stats;   // the last pwa_approx_starts
    pwa::WfaStats wfa_stats;               // the last pwa_scores_wfa / pwa_align_wfa_batch(_cigar)
    pwa::ChainStats chain_stats;           // the last pwa_chain_anchors
    pwa::ChainTopStats chain_top_stats;    // the last pwa_chain_top
    bool score_band = false;   // pwa_ctx_set_score_band: also materialise the int32 score band in HBM
    // pwa_pair_forms: pair_form_name of every form PairLaunch::build / build_mini resolved on this context (a batch object's launches:
    // on the context that created it), distinct, in first-seen order; only pwa_pair_forms_reset empties it
    std::vector<std::string> pair_forms;
    pwa::DevMem mem;   // every device buffer the context keeps between calls: the pwa_align* slots, the parked hand-off buffer, the free list
    hipStream_t aux_stream = nullptr;                  // pwa_batch_run: the mini-stripe launches of a split batch run next to its stripe launch
    hipEvent_t aux_ev[2] = {nullptr, nullptr};         // fork / join of that
    hipStream_t copy_stream = nullptr;                 // uploads that overlap host work (build_arena)
    hipEvent_t copy_ev[2] = {nullptr, nullptr};
    // page-locked staging of everything the library itself uploads or reads back (see PinnedBuf)
    enum { PIN_ARENA, PIN_ARENA2, PIN_TASKS, PIN_SLOT0, PIN_SLOT1, PIN_SLOT2, PIN_SLOT3, PIN_SLOT4, PIN_DESC, PIN_TL, PIN_RES, PIN_BOUNCE, PIN_STR, PIN_N };
    PinnedBuf pin[PIN_N];
};

__global__ void pwa_nop_kernel(int* p);   // (pwalign_ctx.hip; PWA_PROBE / PWA_DEBUG launch it to time a submission)

#pragma GCC visibility push(hidden)
namespace pwa {

// RAII device buffer of a batch object or of one call, from ctx->mem; with `pool` set, released buffers go to the context's free list
// and come back from it
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    pwa_ctx* pool = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release();
    hipError_t alloc(pwa_ctx* ctx, size_t n);   // ctx: whose memory and PWA_POISON (never null; `pool` only says where released buffers go)
    // the strip hand-off workspace: the one an earlier batch of ctx parked if it holds n bytes, else alloc; and parking it (pooled buffers only)
    hipError_t alloc_hand(pwa_ctx* ctx, size_t n);
    void park_hand();
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// A caller's substitution table (include/pwalign.h, pwa_align_subst_batch) as the subst kernels read it (subst_fill.hip.h): the
// 256-byte code map, then n_sym rows of `stride` raw scores with the TEXT code as the row; max_abs = max |submat|
struct SubstTable {
    std::vector<uint32_t> blob;
    int n_sym = 0, stride = 0;
    int64_t max_abs = 0;
    DevBuf dev;   // the blob on the device (subst_upload)
};

// ---- defined in pwalign_ctx.hip (the comments are at the definitions)
int subst_prepare(pwa_ctx* ctx, const uint8_t* code, int n_sym, const int32_t* submat, SubstTable& t);
int subst_upload(pwa_ctx* ctx, SubstTable& t);
void radix_sort_by_key(std::vector<uint64_t>& key, std::vector<uint32_t>& idx);
void scan_bytes(const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const std::vector<uint8_t>& in, bool out[256],
                uint64_t bytes_per_thread);
int64_t max_abs(std::initializer_list<int64_t> vals);
bool tb_range_ok(uint64_t n_plus_m, int match, int mismatch, int gap, int bits = 28);
bool diag_keys_fit(int match, int mismatch, int gap);
bool gap0_ok(uint64_t n_plus_m, int match, int mismatch, int gap);
bool code_alphabet(const bool seen[256], uint8_t code_of[256], int match, int mismatch, int gap, const Knobs& knobs);
int mini_rl_for(uint64_t n);
int wide_rl_for(uint64_t n);
hipError_t workspace(pwa_ctx* ctx, DevMem::Slot slot, size_t bytes, Lease& out);
hipError_t upload_via_bounce(pwa_ctx* c, void* dst, const void* src, size_t bytes);
hipError_t build_arena(pwa_ctx* c, void* d_arena, uint64_t arena_bytes, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                       const std::vector<uint8_t>& is_used, const std::vector<uint64_t>& aoff, const uint8_t* table, bool nul_free = false);
int fail(pwa_ctx* c, int code, const std::string& msg);
int check_pair_list(pwa_ctx* ctx, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, uint32_t n_seq);
uint64_t layout_arena(const uint64_t* seq_off, uint32_t n_seq, const std::vector<uint8_t>& is_used, uint64_t tail_pad, std::vector<uint64_t>& aoff);
// ---- defined in pwalign_align.hip, behind the planner it checks; pwa_selftest_host ends with it
int selftest_align_plan(uint64_t x, int check);

// Stable counting sort of `idx` by key(idx[i]) in [0, n_buckets): two linear passes.
template <class KeyFn>
void counting_sort(std::vector<uint32_t>& idx, std::vector<uint32_t>& tmp, size_t n_buckets, KeyFn key) {
    const size_t n = idx.size();
    if (n >= (1u << 18) && n_buckets <= (1u << 16)) {
        // a million pairs: both passes are scattered memory accesses -- on a few threads, each with its own histogram over its own
        // contiguous part of idx (thread t's elements of a bucket go behind those of the threads before it: still stable)
        const int T = (int)std::min<size_t>({8, std::max(1u, std::thread::hardware_concurrency()), n >> 16});
        std::vector<std::vector<uint32_t>> cnt((size_t)T, std::vector<uint32_t>(n_buckets, 0));
        auto part = [&](int t) { return std::make_pair(n * (size_t)t / (size_t)T, n * (size_t)(t + 1) / (size_t)T); };
        auto run = [&](auto&& fn) {
            std::vector<std::thread> th;
            for (int t = 1; t < T; ++t) th.emplace_back(fn, t);
            fn(0);
            for (auto& x : th) x.join();
        };
        run([&](int t) {
            const auto [a, z] = part(t);
            uint32_t* const c = cnt[(size_t)t].data();
            for (size_t o = a; o < z; ++o) ++c[key(idx[o])];
        });
        uint32_t at = 0;
        for (size_t bkt = 0; bkt < n_buckets; ++bkt)
            for (int t = 0; t < T; ++t) {
                const uint32_t c = cnt[(size_t)t][bkt];
                cnt[(size_t)t][bkt] = at;
                at += c;
            }
        tmp.resize(n);
        run([&](int t) {
            const auto [a, z] = part(t);
            uint32_t* const c = cnt[(size_t)t].data();
            for (size_t o = a; o < z; ++o) tmp[c[key(idx[o])]++] = idx[o];
        });
        idx.swap(tmp);
        return;
    }
    std::vector<uint32_t> cnt(n_buckets + 1, 0);
    for (const uint32_t v : idx) ++cnt[key(v) + 1];
    for (size_t b = 0; b < n_buckets; ++b) cnt[b + 1] += cnt[b];
    tmp.resize(idx.size());
    for (const uint32_t v : idx) tmp[cnt[key(v)]++] = v;
    idx.swap(tmp);
}

// idx by DESCENDING length, stable (equal lengths keep their order): linear passes instead of std::stable_sort's n log n compares
// through two indirections ([cpu] 16 384 pairs of random lengths: 0.95 ms for the merge sort)
template <class LenFn>
void sort_by_length_desc(std::vector<uint32_t>& idx, LenFn len_of) {
    if (idx.size() < 2) return;
    uint64_t lmin = ~0ull, lmax = 0;
    for (const uint32_t v : idx) {
        const uint64_t l = len_of(v);
        lmin = std::min(lmin, l);
        lmax = std::max(lmax, l);
    }
    if (lmin == lmax) return;
    if (lmax - lmin <= 4 * (uint64_t)idx.size() + 65536) {
        std::vector<uint32_t> tmp;
        counting_sort(idx, tmp, (size_t)(lmax - lmin + 1), [&](uint32_t v) { return (size_t)(lmax - len_of(v)); });
    } else {
        std::vector<uint64_t> key(idx.size());
        for (size_t o = 0; o < idx.size(); ++o) key[o] = lmax - len_of(idx[o]);
        radix_sort_by_key(key, idx);
    }
}

#define HIPC(ctx, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            return fail((ctx), e_ == hipErrorOutOfMemory ? PWA_E_NOMEM : PWA_E_HIP,                  \
                        std::string(#call) + ": " + hipGetErrorString(e_));                          \
        }                                                                                            \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int32_t wrap_mul(int64_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }

// Geometry of the wavefront (pair) engine: RL rows per lane (stripe = 64*RL rows) and W compute waves
// per workgroup (a workgroup task = W consecutive stripes + one helper wave).  Pairs of a single
// stripe use W = 1; short multi-stripe pairs get RL = 2 (twice the stripes = twice the waves in flight).
struct PairGeom {
    int rl, w;
};
PairGeom choose_geom(const Knobs& kn, uint64_t max_n, bool keyed = true, bool keyed_tb = false);
size_t tb_band_bytes(uint64_t n, uint64_t m, int rl);

// What a launch of the wavefront (pair) engine IS, as one value.  resolve_pair_form (pwalign_ctx.hip) maps it to PairKernels, or says
// that there are none: build() / build_mini() refuse such a form with PWA_E_INVALID.
enum PairFamily {
    PF_STRIPE_FILL,        // pair_fill.hip.h: the linear-gap fills of the stripe engine and their walks
    PF_STRIPE_DIST,        // pair_dist.hip.h: hw4's NW distance -- two values per hand-off column, no band, no walk
    PF_STRIPE_AFFINE,      // pair_affine.hip.h: hw3's affine score, likewise; build() takes go as gap, and ge
    PF_STRIPE_AFFINE_TB,   // pair_affine_tb.hip.h: hw3's affine alignment -- the fill writes a band, a walk follows
    PF_MINI_FILL,          // mini_fill.hip.h: the mini-stripe engine, w lanes per pair, rl rows per lane, 64 / w pairs per wave
    PF_MINI_GOTOH,         // gotoh_fill.hip.h: its affine-gap kernels (gap = gap_open); without a band the fill writes score and end cell itself: no walk
    PF_MINI_SUBST          // subst_fill.hip.h: ... with the diagonal score from the table PairForm::subst; the walk is gotoh's
};
enum PairBand { BAND_NONE, BAND_TB, BAND_TB_SCORES };   // what the fill materialises: nothing, the traceback band, the band + the int32 score band
enum PairCells {
    CELLS_PLAIN,   // int32 compare-and-select on raw bytes: anything the reference's int holds (traceback fills: RL = 4 only)
    CELLS_KEYED,   // H * 4 + priority (needs |H| < 2^28) on raw bytes; the gotoh families' cells
    CELLS_CODED,   // ... on sequences coded 0..6 (pad 7), the key constants fit a byte: table scoring
    CELLS_GAP0     // ... global, in gap-shifted coordinates: the caller gives build() gap 0 and the scores s - 2 gap
};
struct SubstRef {   // SubstTable::dev and its layout
    const uint32_t* tab = nullptr;
    int n_sym = 0, stride = 0;
};
struct PairForm {
    PairFamily family;
    int mode;          // PWA_MODE_NW | SW | SG (the hw3 / hw4 families: NW)
    PairBand band;
    int walk;          // WALK_NONE (end cells only; the only walk without a band) / WALK_OPS / WALK_OVERLAP
    PairCells cells;   // the fill families' choice; hw3 / hw4: CELLS_PLAIN, gotoh / subst: CELLS_KEYED
    int rl, w;         // rows per lane; stripe families: compute waves per workgroup (PairGeom), mini families: lanes per pair (16 | 64)
    SubstRef subst = {};   // PF_MINI_SUBST only
    bool mini() const { return family >= PF_MINI_FILL; }
};
// family/mode/band/walk/cells/rl<n>/w<n> (mini families: ln<n>), e.g. stripe_fill/NW/tb/ops/coded/rl2/w4: the only place a form becomes a
// name (pwa_pair_forms, pwa_pair_form_table); a field outside its enum reads "?"
std::string pair_form_name(const PairForm& f);
// The forms the seven call sites of PairLaunch can build, each once (DESIGN.md 3.23 derives the list from their expressions); the
// PF_MINI_SUBST entries carry a one-word host table, enough for resolve_pair_form.  pwa_selftest_host and pwa_pair_form_table walk it.
const std::vector<PairForm>& pair_form_listing();
typedef void (*subst_kernel_t)(const PairParams, const uint32_t*, int, int);
struct PairKernels {
    pair_kernel_t fill = nullptr, walk = nullptr;   // the fill, `block` threads per workgroup; the walk, one wave per pair, when `walks`
    subst_kernel_t sfill = nullptr;                 // PF_MINI_SUBST: launched in the fill's place, with the table
    unsigned block = 0;
    bool walks = false;
};

// What a launch of the banded class (banded_fill.hip.h: one wave per pair, stripes of 64 rl rows over a diagonal band) IS, as one value.
// resolve_banded_form (pwalign_ctx.hip) maps it to the kernels' host stubs, or says that there are none.
struct BandedForm {
    int rl, mode;   // rows per lane (4 | 8); PWA_MODE_NW | SW | SG (EXT: NW)
    bool ext;       // extension from (0, 0) with an X-drop: the kernels take xdrop behind row_cap
    bool subst;     // the diagonal score from a table: the kernels end with (blob, n_sym, stride)
    bool walk;      // false: the score pass (no band, no walk kernel)
};
struct BandedKernels {
    const void *fill = nullptr, *walk = nullptr;   // the fill or score pass, 64 * kBandedWaves threads per workgroup; the walk, one wave per pair
};
bool resolve_banded_form(const BandedForm& f, BandedKernels& k);
// Fill or score pass, then the form's walk, on `st`; `after_fill` is recorded behind the fill in every form.  row_cap: the launch's
// widest band; xdrop and tab: read by the forms that have them.
hipError_t banded_launch(const BandedForm& f, const PairParams& G, int row_cap, int xdrop, const SubstRef& tab, int num_cu, hipStream_t st,
                         hipEvent_t after_fill);

// Device-side state of one launch of the wavefront (pair) engine: pair descriptors, the global
// stripe-task list, hand-off rows, progress counters, per-stripe bests.
struct PairLaunch {
    Lease desc, tasks, rows, progress, best, queue;
    // where the six come from, said once before build(): buffers of the launch's own (pwa_align_matrices), the context's slots (one
    // launch at a time per context: the other pwa_align* calls), or the free list (a batch object's launches)
    enum { MEM_OWN, MEM_SLOTS, MEM_FREE_LIST } mem = MEM_OWN;
    size_t progress_bytes = 0;
    PairParams G{};
    PairForm form{};   // set and resolved by build() / build_mini()
    PairKernels k;
    uint32_t grid = 0;
    uint64_t row_bytes = 0;
    uint64_t n_stripes = 0;
    DevBuf stamps;   // PWA_STAMPS=<file>: per-stripe time stamps of the fill (debugging the stripe pipeline)

    // pd[q].{pat,txt,n,m,tb,sband,res,ops,ops_cap} filled by the caller; this adds the pipeline fields
    int build(pwa_ctx* ctx, std::vector<PairDesc>& pd, const PairForm& f, int match, int mismatch, int gap, int gap_extend = 0);
    int build_mini(pwa_ctx* ctx, std::vector<PairDesc>& pd, uint32_t n_real, const PairForm& f, int match, int mismatch, int gap);
    int upload_desc(pwa_ctx* ctx, const std::vector<PairDesc>& pd);
    void set_params(uint32_t n_pairs, uint32_t n_tasks, int match, int mismatch, int gap, int gap_extend);
    // enqueue: zero the queue / progress words, fill, then the walk (or only the end-cell pick)
    int launch(pwa_ctx* ctx, hipStream_t st, hipEvent_t after_fill);
    // after the stream has been synchronised: did a bounded spin give up?
    int check(pwa_ctx* ctx);
};

}  // namespace pwa
#pragma GCC visibility pop
