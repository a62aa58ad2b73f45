// pwalign_ctx.hip -- contexts, device memory management (buffers, workspaces, uploads, the sequence arena) and the launches of
// the wavefront (pair) engine.  The schedulers of the entry points are in pwalign.hip (score batches), pwalign_affine_tb.hip and
// pwalign_align.hip.  gfx950 only; there is no CPU path.
#include "pwalign_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "banded_fill.hip.h"
#include "sufarr_ctx.h"

using namespace pwa;

namespace pwa {
// gotoh_kernels.hip: the affine-gap (Gotoh) fills and walks, mode = PWA_MODE_NW | SW | SG; ln = 16 (rl in kMiniRL) or 64 (rl = 8 | 16)
void (*gotoh_fill_kernel_for(int rl, int mode, int ln))(const PairParams);
void (*gotoh_walk_kernel_for(int rl, int mode, int ln))(const PairParams);
void (*gotoh_scores_kernel_for(int rl, int mode, int ln))(const PairParams);   // the fills without a band (no walk follows)
// subst_kernels.hip: the same classes and modes under a substitution table (device blob, n_sym, row stride); the walk is gotoh's
subst_kernel_t subst_fill_kernel_for(int rl, int mode, int ln);
subst_kernel_t subst_scores_kernel_for(int rl, int mode, int ln);
// banded_kernels.hip, banded_scores_kernels.hip, banded_subst_kernels.hip, banded_ext_kernels.hip, banded_ext_subst_kernels.hip: the
// banded class's fills (band = true) and score passes, and the walk over the fills' band; rl = 8, else 4; mode = SW, SG, else NW
const void* banded_kernel_for(int rl, int mode, bool walk);
const void* banded_scores_kernel_for(int rl, int mode);
const void* banded_subst_kernel_for(int rl, int mode, bool band);
const void* banded_ext_kernel_for(int rl, bool band);
const void* banded_ext_subst_kernel_for(int rl, bool band);
}

__global__ void pwa_nop_kernel(int* p) {
    if (p && threadIdx.x == 12345) *p = 0;
}

// Symbols -> codes on the device (build_arena): n16 blocks of 16 bytes at p, every byte through the 256-entry table.  The host then only
// copies raw bytes into the upload buffers (a memcpy instead of a table lookup per byte, which was what bounded a 570 MB arena).
struct RecodeTable {
    uint8_t t[256];
};
__global__ __launch_bounds__(256) void pwa_recode_kernel(uint8_t* p, size_t n16, const RecodeTable tab) {
    __shared__ uint8_t lut[256];
    lut[threadIdx.x] = tab.t[threadIdx.x];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        uint4 v = reinterpret_cast<const uint4*>(p)[i];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; ++d)
            w[d] = (uint32_t)lut[w[d] & 0xffu] | (uint32_t)lut[(w[d] >> 8) & 0xffu] << 8 | (uint32_t)lut[(w[d] >> 16) & 0xffu] << 16 | (uint32_t)lut[w[d] >> 24] << 24;
        reinterpret_cast<uint4*>(p)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

void Knobs::read() {
    auto flag = [](const char* n) { return std::getenv(n) != nullptr; };
    auto num = [](const char* n, int dflt) { const char* e = std::getenv(n); return e ? std::atoi(e) : dflt; };
    debug = flag("PWA_DEBUG");
    probe = flag("PWA_PROBE");
    force_rl = num("PWA_FORCE_RL", 0);
    force_w = num("PWA_FORCE_W", 0);
    wg_per_cu = num("PWA_WG_PER_CU", 0);
    no_lds_pad = flag("PWA_NO_LDS_PAD");
    if (const char* e = std::getenv("PWA_STAMPS")) stamps = e;
    trace_stripe = num("PWA_TRACE_STRIPE", -1);
    no_packed_dist = flag("PWA_NO_PACKED_DIST");
    force_lanes = num("PWA_FORCE_LANES", -1);
    force_r = num("PWA_FORCE_R", 0);
    force_mode = num("PWA_FORCE_MODE", -1);
    if (const char* e = std::getenv("PWA_ARENA_LIMIT")) arena_limit = std::max<uint64_t>(1024, std::strtoull(e, nullptr, 10));
    if (const char* e = std::getenv("PWA_LANE_ROWS_LIMIT")) lane_rows_limit = std::max<uint64_t>(1024, std::strtoull(e, nullptr, 10));
    mini_per_cu = num("PWA_MINI_PER_CU", 0);
    if (const char* e = std::getenv("PWA_RANGE_BYTES")) range_bytes = std::max<uint64_t>(4096, std::strtoull(e, nullptr, 10));
    no_pair_table = flag("PWA_NO_PAIR_TABLE");
    no_keyed_tb = flag("PWA_NO_KEYED_TB");
    no_gap_shift = flag("PWA_NO_GAP_SHIFT");
    no_tiled_ops = flag("PWA_NO_TILED_OPS");
    no_pipeline = flag("PWA_NO_PIPELINE");
    pipe_runs = num("PWA_PIPE_RUNS", 0);
    scores_route = num("PWA_SCORES_ROUTE", -1);
    tb_engine = num("PWA_TB_ENGINE", -1);
    banded_rl = num("PWA_BANDED_RL", 0);
    if (banded_rl != 4 && banded_rl != 8) banded_rl = 0;
    cell16 = num("PWA_CELL16", -1);
    prof16 = num("PWA_PROF16", -1);
    prof16_int = num("PWA_PROF16_INT", -1);
    affine_tb_route = num("PWA_AFFINE_TB_ROUTE", -1);
    if (const char* e = std::getenv("PWA_OCC_CHUNK_HITS")) occ_chunk_hits = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    poison = parse_poison(std::getenv("PWA_POISON"));
    if (const char* e = std::getenv("PWA_APPROX_CHUNK")) approx_chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)), 1u << 30);
}

pwa::UnitCtx pwa::unit_ctx(pwa_ctx* c) {
    UnitCtx v;
    v.device = c->device;
    v.stream = c->stream;
    v.debug = c->knobs.debug;
    v.err = &c->err;
    v.poison = &c->poison;
    return v;
}

pwa::SaCtxView pwa::sa_ctx_view(pwa_ctx* c) {
    SaCtxView v{unit_ctx(c)};
    v.occ_chunk_hits = c->knobs.occ_chunk_hits;
    return v;
}

pwa::ApproxCtxView pwa::approx_ctx_view(pwa_ctx* c) {
    ApproxCtxView v{unit_ctx(c)};
    v.chunk = c->knobs.approx_chunk;
    v.occ_chunk_hits = c->knobs.occ_chunk_hits;
    v.stats = &c->approx_stats;
    v.starts_stats = &c->approx_starts_stats;
    return v;
}
const pwa::ApproxStats& pwa::approx_stats_of(const pwa_ctx* c) { return c->approx_stats; }
const pwa::ApproxStartsStats& pwa::approx_starts_stats_of(const pwa_ctx* c) { return c->approx_starts_stats; }

pwa::WfaCtxView pwa::wfa_ctx_view(pwa_ctx* c) {
    WfaCtxView v{unit_ctx(c)};
    v.range_bytes = c->knobs.range_bytes;
    v.stats = &c->wfa_stats;
    return v;
}
const pwa::WfaStats& pwa::wfa_stats_of(const pwa_ctx* c) { return c->wfa_stats; }

pwa::ChainCtxView pwa::chain_ctx_view(pwa_ctx* c) {
    ChainCtxView v{unit_ctx(c)};
    v.range_bytes = c->knobs.range_bytes;
    v.stats = &c->chain_stats;
    return v;
}
const pwa::ChainStats& pwa::chain_stats_of(const pwa_ctx* c) { return c->chain_stats; }
pwa::ChainTopStats* pwa::chain_top_stats_of(pwa_ctx* c) { return &c->chain_top_stats; }

hipError_t pwa::recode_bytes(hipStream_t s, uint8_t* p, size_t n16, const uint8_t* table) {
    if (!n16) return hipSuccess;
    RecodeTable rt;
    std::memcpy(rt.t, table, 256);
    hipLaunchKernelGGL(pwa_recode_kernel, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 4096)), dim3(256), 0, s, p, n16, rt);
    return hipGetLastError();
}

namespace {

bool key_byte(int64_t k) { return k <= 127 && k >= -126; }   // (diag_keys_fit, gap0_ok)

// Runs fn(first_seq, last_seq, thread) over the sequences, split into byte-balanced contiguous ranges, on up to
// 16 host threads (one per >= 8 MiB): the host passes over the input (alphabet scan, symbol coding into the
// arena) are memory-bound loops that otherwise dominate the call for inputs of hundreds of MB.
template <class F>
void for_seq_ranges(const uint64_t* seq_off, uint32_t n_seq, F&& fn, int* n_threads_out = nullptr, uint64_t bytes_per_thread = 8ull << 20) {
    const uint64_t total = n_seq ? seq_off[n_seq] - seq_off[0] : 0;
    int T = (int)std::min<uint64_t>({16, total / bytes_per_thread + 1, std::max(1u, std::thread::hardware_concurrency())});
    T = std::max(1, std::min<int>(T, (int)std::max<uint32_t>(n_seq, 1)));
    if (n_threads_out) *n_threads_out = T;
    std::vector<uint32_t> cut((size_t)T + 1, n_seq);
    cut[0] = 0;
    for (int t = 1; t < T; ++t) {
        const uint64_t want = seq_off[0] + total / (uint64_t)T * (uint64_t)t;
        cut[(size_t)t] = (uint32_t)(std::lower_bound(seq_off, seq_off + n_seq, want) - seq_off);
    }
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back([&, t] { fn(cut[(size_t)t], cut[(size_t)t + 1], t); });
    fn(cut[0], cut[1], 0);
    for (auto& x : th) x.join();
}

}  // namespace

namespace pwa {

void DevBuf::release() {
    if (pool) pool->mem.keep(p, bytes);
    else if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}
// PWA_POISON (poison.h).  The fill is a test mode: the device is drained before it, so that nothing enqueued earlier on any of the
// context's (non-blocking) streams still uses the buffer, and after it, so that nothing enqueued later can overtake it.
int parse_poison(const char* s) {
    if (!s) return -1;
    const bool hex = s[0] == '0' && (s[1] == 'x' || s[1] == 'X');
    const char* d = hex ? s + 2 : s;
    if (!*d) return -2;
    unsigned v = 0;
    for (; *d; ++d) {
        const int c = (unsigned char)*d;
        const int digit = c >= '0' && c <= '9' ? c - '0' : hex && c >= 'a' && c <= 'f' ? c - 'a' + 10 : hex && c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (digit < 0) return -2;
        v = v * (hex ? 16u : 10u) + (unsigned)digit;
        if (v > 255) return -2;
    }
    return (int)v;
}
hipError_t poison_device(Poison* po, void* p, size_t cap) {
    if (!po || po->byte < 0) return hipSuccess;
    if (!p || !cap) return hipSuccess;
    hipError_t e = hipSetDevice(po->device);   // (hipDeviceSynchronize and hipMemset act on the current device)
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemset(p, po->byte, cap);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) ++po->buffers, po->bytes += cap;
    return e;
}
void poison_host(Poison* po, void* p, size_t cap) {
    if (!po || po->byte < 0 || !p || !cap) return;
    std::memset(p, po->byte, cap);
    ++po->buffers, po->bytes += cap;
}

hipError_t DevBuf::alloc(pwa_ctx* ctx, size_t n) {
    release();
    const hipError_t e = ctx->mem.buffer(n ? n : 16, pool != nullptr, &p, &bytes);
    return e == hipSuccess ? poison_device(&ctx->poison, p, bytes) : e;
}
hipError_t DevBuf::alloc_hand(pwa_ctx* ctx, size_t n) {
    release();
    if (!ctx->mem.take_hand(n, &p, &bytes)) return alloc(ctx, n);
    return poison_device(&ctx->poison, p, bytes);
}
void DevBuf::park_hand() {
    if (!pool) return;
    pool->mem.park_hand(p, bytes);
    p = nullptr;
    bytes = 0;
}

// Stable LSD radix sort of `idx` by 64-bit keys (16-bit digits; passes whose digit is constant are skipped).
// Sorting a million pairs with std::sort and a comparator that looks lengths up cost ~95 ms per batch [gpu box].
void radix_sort_by_key(std::vector<uint64_t>& key, std::vector<uint32_t>& idx) {
    const size_t n = idx.size();
    std::vector<uint64_t> key2(n);
    std::vector<uint32_t> idx2(n);
    std::vector<size_t> cnt(65536);
    for (int pass = 0; pass < 4; ++pass) {
        const int sh = 16 * pass;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (size_t i = 0; i < n; ++i) ++cnt[(key[i] >> sh) & 0xffff];
        if (n && cnt[(key[0] >> sh) & 0xffff] == n) continue;
        size_t run = 0;
        for (size_t d = 0; d < 65536; ++d) {
            const size_t c = cnt[d];
            cnt[d] = run;
            run += c;
        }
        for (size_t i = 0; i < n; ++i) {
            const size_t o = cnt[(key[i] >> sh) & 0xffff]++;
            key2[o] = key[i];
            idx2[o] = idx[i];
        }
        key.swap(key2);
        idx.swap(idx2);
    }
}

// out[v]: does byte v occur in a sequence s with in[s] != 0?  One pass over those sequences, on a thread per bytes_per_thread of input
void scan_bytes(const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq, const std::vector<uint8_t>& in, bool out[256],
                uint64_t bytes_per_thread) {
    bool part[16][256] = {};
    for_seq_ranges(seq_off, n_seq, [&](uint32_t s0, uint32_t s1, int t) {
        bool* mine = part[t];
        for (uint32_t s = s0; s < s1; ++s)
            if (in[s])
                for (uint64_t o = seq_off[s]; o < seq_off[s + 1]; ++o) mine[seq_bytes[o]] = true;
    }, nullptr, bytes_per_thread);
    for (int v = 0; v < 256; ++v) {
        out[v] = false;
        for (int t = 0; t < 16; ++t) out[v] |= part[t][v];
    }
}

// the largest magnitude among scoring values (a trailing 1 where the result divides)
int64_t max_abs(std::initializer_list<int64_t> vals) {
    int64_t r = 0;
    for (const int64_t v : vals) r = std::max<int64_t>(r, std::llabs((long long)v));
    return r;
}

// The traceback kernels keep H * 4 + priority in int32 (pair_fill.hip.h): |H| has to stay below 2^28.
// (bits = 26: local fills of the mini-stripe kernels, whose first-maximum records hold H * 16 + a step index, mini_fill.hip.h)
bool tb_range_ok(uint64_t n_plus_m, int match, int mismatch, int gap, int bits) {
    return (n_plus_m + 2) <= (1ull << bits) / (uint64_t)max_abs({match, mismatch, gap, 1});
}

// The keyed fills score four rows with one byte-table lookup (pair_fill.hip.h, PERM): the table holds the two diagonal key
// constants, and both must fit a signed byte (key_byte).
bool diag_keys_fit(int match, int mismatch, int gap) {
    return key_byte(((int64_t)match - gap) * 4 + 2) && key_byte(((int64_t)mismatch - gap) * 4 + 2);
}
// Global fills in gap-shifted coordinates G = H - gap (i + j) (GAP0): |G| <= |H| + |gap| (n + m), twice the range, and both shifted
// diagonal constants (s - 2 gap) * 4 + prio(diag) - prio(left) in the byte table
bool gap0_ok(uint64_t n_plus_m, int match, int mismatch, int gap) {
    return key_byte(((int64_t)match - 2 * (int64_t)gap) * 4 + 1) && key_byte(((int64_t)mismatch - 2 * (int64_t)gap) * 4 + 1) &&
           tb_range_ok(n_plus_m, match, mismatch, gap, 27);
}
// Alphabets of at most 7 symbols (DNA, DNA + N, ...) are stored as codes 0..6 -- equality is all the recurrence ever asks of a symbol
// (hw2.cpp:142, 208) -- so that the fill can score four rows with one byte-table lookup.  Fills code_of; true when the fills may use it.
bool code_alphabet(const bool seen[256], uint8_t code_of[256], int match, int mismatch, int gap, const Knobs& knobs) {
    int n_alpha = 0;
    for (int v = 0; v < 256; ++v) {
        code_of[v] = (uint8_t)std::min(n_alpha, 7);
        if (seen[v]) ++n_alpha;
    }
    return n_alpha <= 7 && diag_keys_fit(match, mismatch, gap) && !knobs.no_pair_table;
}
// rows per lane of the four-pair mini-stripe class that holds an n-row pattern, 0: none (n > 256)
int mini_rl_for(uint64_t n) {
    for (const int rl : kMiniRL)
        if (n <= (uint64_t)(16 * rl)) return rl;
    return 0;
}
// ... and of the one-pair-per-wave class (64 lanes) for 257 .. 1024 rows
int wide_rl_for(uint64_t n) { return n <= 384 ? 6 : n <= 512 ? 8 : n <= 768 ? 12 : 16; }

// `bytes` of the context's slot (DevMem::workspace: reused when big enough, regrown otherwise, a buffer of the lease's own beyond
// kBandCacheMax), PWA_POISON over the whole capacity on every acquisition
hipError_t workspace(pwa_ctx* ctx, DevMem::Slot slot, size_t bytes, Lease& out) {
    const hipError_t e = ctx->mem.workspace(slot, bytes, out);
    return e == hipSuccess ? poison_device(&ctx->poison, out.get(), out.cap()) : e;
}

// pageable memory that the library does not own (or that is too large to mirror in page-locked memory): through a bounce buffer
hipError_t upload_via_bounce(pwa_ctx* c, void* dst, const void* src, size_t bytes) {
    constexpr size_t kChunk = 8u << 20;
    hipError_t e = c->pin[pwa_ctx::PIN_BOUNCE].reserve(std::min(bytes, kChunk));
    for (size_t o = 0; e == hipSuccess && o < bytes; o += kChunk) {
        const size_t n = std::min(kChunk, bytes - o);
        std::memcpy(c->pin[pwa_ctx::PIN_BOUNCE].p, static_cast<const uint8_t*>(src) + o, n);
        e = hipMemcpy(static_cast<uint8_t*>(dst) + o, c->pin[pwa_ctx::PIN_BOUNCE].p, n, hipMemcpyHostToDevice);
    }
    return e;
}

// The device arena of a call: every used sequence s at aoff[s] (16-byte aligned) as symbols -- through `table` (256 entries) or
// copied when table == nullptr -- and zeros everywhere else.  It goes up in pieces of ~32 MiB: while piece k is on its way
// (copy stream, from one of two page-locked buffers of the context) piece k + 1 is being coded by several host threads into the
// other -- readFasta's blob is never repacked into a second host copy, and a 570 MB arena costs 2 x 32 MiB of pinned memory.
// r03: arenas of a MiB and more are coded ON THE DEVICE when no sequence holds a NUL byte (`nul_free`: the padding between sequences is
// zeros and has to stay zeros, so the device table maps 0 to 0): the host threads then only copy raw bytes into the pieces and a small
// kernel behind every piece's copy turns them into codes in place.
hipError_t build_arena(pwa_ctx* c, void* d_arena, uint64_t arena_bytes, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seq,
                       const std::vector<uint8_t>& is_used, const std::vector<uint64_t>& aoff, const uint8_t* table, bool nul_free) {
    constexpr uint64_t kPiece = 32ull << 20;
    const bool on_device = table && nul_free && arena_bytes >= (1ull << 20) && arena_bytes % 16 == 0;
    RecodeTable rt;
    if (on_device) {
        std::memcpy(rt.t, table, 256);
        rt.t[0] = 0;
        table = nullptr;   // the pieces take raw bytes
    }
    std::vector<uint32_t> used;
    for (uint32_t s = 0; s < n_seq; ++s)
        if (is_used[s]) used.push_back(s);
    if (used.empty()) return hipMemset(d_arena, 0, arena_bytes);
    hipError_t e = hipSuccess;
    int piece = 0;
    for (size_t u0 = 0; u0 < used.size() && e == hipSuccess; ++piece) {
        size_t u1 = u0 + 1;
        const uint64_t a0 = u0 == 0 ? 0 : aoff[used[u0]];
        auto end_of = [&](size_t u) { return u < used.size() ? aoff[used[u]] : arena_bytes; };
        while (u1 < used.size() && end_of(u1 + 1) - a0 <= kPiece) ++u1;
        const uint64_t a1 = end_of(u1), bytes = a1 - a0;
        PinnedBuf& pb = c->pin[pwa_ctx::PIN_ARENA + (piece & 1)];
        if (piece >= 2) e = hipEventSynchronize(c->copy_ev[piece & 1]);   // the copy that last read this buffer
        if (e == hipSuccess) e = pb.reserve(bytes);
        if (e != hipSuccess) break;
        uint8_t* const host = pb.as<uint8_t>();
        // sequences u0 .. u1-1 of the piece over a few threads, byte-balanced
        const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>({16, bytes / (1ull << 20) + 1, std::max(1u, std::thread::hardware_concurrency()), (uint64_t)(u1 - u0)}));
        auto work = [&](int t) {
            const uint64_t lo = a0 + bytes / T * t, hi = t + 1 == T ? a1 : a0 + bytes / T * (t + 1);
            // first sequence whose region starts at or after lo (regions are [aoff[s], aoff[next]))
            size_t u = std::lower_bound(used.begin() + u0, used.begin() + u1, lo, [&](uint32_t sidx, uint64_t v) { return aoff[sidx] < v; }) - used.begin();
            if (t == 0) {
                u = u0;
                if (a0 < aoff[used[u0]]) std::memset(host, 0, aoff[used[u0]] - a0);
            }
            for (; u < u1 && aoff[used[u]] < hi; ++u) {
                const uint32_t sidx = used[u];
                const uint64_t len = seq_off[sidx + 1] - seq_off[sidx], r0 = aoff[sidx], r1 = end_of(u + 1);
                uint8_t* dst = host + (r0 - a0);
                const uint8_t* src = seq_bytes + seq_off[sidx];
                if (table)
                    for (uint64_t o = 0; o < len; ++o) dst[o] = table[src[o]];
                else if (len)
                    std::memcpy(dst, src, len);
                std::memset(dst + len, 0, r1 - r0 - len);
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
        e = hipMemcpyAsync(static_cast<uint8_t*>(d_arena) + a0, host, bytes, hipMemcpyHostToDevice, c->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(c->copy_ev[piece & 1], c->copy_stream);
        if (e == hipSuccess && on_device && a0 % 16 == 0 && bytes % 16 == 0) {   // (pieces start and end on sequence regions: multiples of 16)
            const size_t n16 = (size_t)(bytes / 16);
            hipLaunchKernelGGL(pwa_recode_kernel, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 4096)), dim3(256), 0, c->copy_stream,
                               static_cast<uint8_t*>(d_arena) + a0, n16, rt);
            e = hipGetLastError();
        } else if (e == hipSuccess && on_device) {
            e = hipErrorInvalidValue;   // cannot happen: regions are 16-byte aligned
        }
        u0 = u1;
    }
    const hipError_t e2 = hipStreamSynchronize(c->copy_stream);
    return e != hipSuccess ? e : e2;
}

int fail(pwa_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

PairGeom choose_geom(const Knobs& kn, uint64_t max_n, bool keyed, bool keyed_tb) {
    // (W = 3 -- three stripes + the helper = one wave per SIMD -- was measured in r02: no gain over W = 4, the stripes behind the
    // first workgroup run ~5-9 % slower than the first either way: they run at the edge of what their producer has posted.)
    // RL = 2 up to 32k rows (twice the stripes = twice the waves of a pair in flight), RL = 4 beyond.  (The choice was measured in r01 --
    // 10k x 10k: RL = 2 10 % ahead; 100k x 100k: RL = 4 5 % ahead -- and has held since; today's fills: 1.65 ms / 11.8 - 12.2 ms)
    PairGeom g{max_n <= 32768 ? 2 : 4, 4};
    // 129..256 rows: ONE 256-row stripe (W = 1) instead of two 128-row stripes in a 4-stripe workgroup with two idle waves.  (Since r03
    // only what the mini-stripe engine cannot take comes here with such patterns: alphabets of more than 7 symbols, scores beyond the keys.)
    if (max_n > 128 && max_n <= 256) g.rl = 4;
    if (kn.force_rl) g.rl = kn.force_rl == 2 ? 2 : 4;   // experiments only
    if (!keyed) g.rl = 4;   // the plain int32 traceback form exists for RL = 4 only (pair_kernels.hip)
    if ((max_n + 64 * g.rl - 1) / (64 * g.rl) <= 1) g.w = 1;
    // (W = 8 was built and measured in r02: nine waves on a CU's four SIMDs share issue slots, a step goes from 197 to 317
    // cycles -- a workgroup lives on one CU, so four compute waves is the most that keeps one stripe per SIMD)
    (void)keyed_tb;
    if (kn.force_w) g.w = kn.force_w == 1 ? 1 : 4;
    return g;
}

size_t tb_band_bytes(uint64_t n, uint64_t m, int rl) {
    const uint64_t stripes = (n + 64 * rl - 1) / (64 * rl);
    return (size_t)(stripes * band_steps(m) * 64 * rl);
}

// ---- PairForm -> kernels: the only caller of the kernel units' pickers.  Those take a geometry they have no instantiation for as
// the nearest one and a flag that does not apply as unset, so everything a form may not combine is refused here.
static bool resolve_pair_form(const PairForm& f, PairKernels& k) {   // false: no such kernel
    k = PairKernels{};
    const bool local = f.mode == PWA_MODE_SW, semi = f.mode == PWA_MODE_SG, tb = f.band != BAND_NONE, sband = f.band == BAND_TB_SCORES;
    const bool coded = f.cells >= CELLS_CODED, gap0 = f.cells == CELLS_GAP0;
    if (f.mode != PWA_MODE_NW && !local && !semi) return false;
    if (!tb && f.walk != WALK_NONE) return false;                            // no band: only the end-cell pick
    if (gap0 && (local || semi || sband)) return false;                      // the gap shift is global, and the score band holds H itself
    if ((f.subst.tab != nullptr) != (f.family == PF_MINI_SUBST)) return false;
    if (f.mini() ? f.w != 16 && f.w != 64 : (f.rl != 2 && f.rl != 4) || (f.w != 1 && f.w != 4)) return false;
    k.walks = tb || f.family == PF_STRIPE_FILL || f.family == PF_MINI_FILL;   // (the linear-gap fills leave the end-cell pick to a walk)
    switch (f.family) {
        case PF_STRIPE_FILL:
            // without a band: the keyed chunk over a coded arena, or the plain step (there is no keyed form on raw bytes)
            if (!tb && f.cells == CELLS_KEYED) return false;
            k.fill = tb       ? pair_fill_kernel_for(f.rl, f.w, local, true, sband, coded, f.cells != CELLS_PLAIN, gap0, true, semi)
                     : coded ? pair_fill_kernel_for(f.rl, f.w, local, true, false, true, true, gap0, false, semi)
                             : pair_fill_kernel_for(f.rl, f.w, local, false, false, false, true, false, true, semi);
            k.walk = pair_traceback_kernel_for(f.rl, local, f.walk, semi);
            break;
        case PF_STRIPE_DIST:
        case PF_STRIPE_AFFINE:   // the fill writes D[n][m] / M[n][m] into the score vector itself
        case PF_STRIPE_AFFINE_TB: {
            const bool atb = f.family == PF_STRIPE_AFFINE_TB;
            if (f.mode != PWA_MODE_NW || f.cells != CELLS_PLAIN || f.band != (atb ? BAND_TB : BAND_NONE) || f.walk != (atb ? WALK_OPS : WALK_NONE)) return false;
            k.fill = atb ? pair_affine_tb_kernel_for(f.rl, f.w) : f.family == PF_STRIPE_DIST ? pair_dist_kernel_for(f.rl, f.w) : pair_affine_kernel_for(f.rl, f.w);
            if (atb) k.walk = pair_affine_walk_kernel_for(f.rl);
            break;
        }
        case PF_MINI_FILL:
            if (!coded) return false;
            k.fill = mini_fill_kernel_for(f.rl, local, sband, gap0, tb, f.w, semi);
            k.walk = mini_traceback_kernel_for(f.rl, local, f.walk, f.w, semi);
            break;
        case PF_MINI_GOTOH:
        case PF_MINI_SUBST:
            if (f.cells != CELLS_KEYED || sband || f.walk != (tb ? WALK_OPS : WALK_NONE)) return false;
            if (f.family == PF_MINI_SUBST) k.sfill = tb ? subst_fill_kernel_for(f.rl, f.mode, f.w) : subst_scores_kernel_for(f.rl, f.mode, f.w);
            else k.fill = tb ? gotoh_fill_kernel_for(f.rl, f.mode, f.w) : gotoh_scores_kernel_for(f.rl, f.mode, f.w);
            if (tb) k.walk = gotoh_walk_kernel_for(f.rl, f.mode, f.w);
            break;
    }
    k.block = f.mini() ? 64 * kMiniWaves : 64 * (unsigned)(f.w + 1);   // stripe engine: W compute waves + the helper wave
    return (k.fill || k.sfill) && (k.walk || !k.walks);
}

std::string pair_form_name(const PairForm& f) {
    static const char* const kFamily[] = {"stripe_fill", "stripe_dist", "stripe_affine", "stripe_affine_tb", "mini_fill", "mini_gotoh", "mini_subst"};
    static const char* const kMode[] = {"NW", "SW", "SG"}, * const kBand[] = {"none", "tb", "tb+scores"}, * const kWalk[] = {"none", "ops", "overlap"};
    static const char* const kCells[] = {"plain", "keyed", "coded", "gap0"};
    auto of = [](const char* const* t, size_t n, int v) { return v >= 0 && (size_t)v < n ? t[v] : "?"; };
    return std::string(of(kFamily, 7, f.family)) + "/" + of(kMode, 3, f.mode) + "/" + of(kBand, 3, f.band) + "/" + of(kWalk, 3, f.walk) + "/" + of(kCells, 4, f.cells) +
           "/rl" + std::to_string(f.rl) + (f.mini() ? "/ln" : "/w") + std::to_string(f.w);
}

// What the call sites can build, one loop nest per site, each condition the site's own (DESIGN.md 3.23 quotes the expressions):
//   run_launch (pwalign_align.hip)            walk = OPS | OVERLAP (no SG overlap: validate_align), band = TB | TB_SCORES; stripes: PLAIN at
//                                             RL = 4, KEYED, CODED, GAP0 (NW, BAND_TB); mini classes (16 lanes x kMiniRL, 64 lanes x
//                                             wide_rl_for): CODED, GAP0; gotoh / subst: BAND_TB, OPS, KEYED on TbPlan::class_of's gotoh classes
//   pwa_align_matrices                        BAND_TB_SCORES, WALK_NONE; stripes KEYED | PLAIN (RL = 4), mini classes CODED
//   setup_off_strips (pwalign.hip)            BAND_NONE, WALK_NONE; stripes PLAIN | CODED | GAP0 (NW), hw4's and hw3's families; mini (16 lanes)
//                                             CODED | GAP0 (NW)
//   setup_gotoh_mini                          BAND_NONE, WALK_NONE, KEYED on the gotoh classes
//   affine_tb_on_stripes (pwalign_affine_tb.hip)   RL = 4, W = 1 | 4
const std::vector<PairForm>& pair_form_listing() {
    static const uint32_t tab_word = 0;
    static const std::vector<PairForm> listing = [] {
        const SubstRef tab{&tab_word, 1, 1};
        const std::vector<PairGeom> stripe = {{2, 1}, {2, 4}, {4, 1}, {4, 4}};
        std::vector<PairGeom> mini16, mini, gotoh;
        for (const int rl : kMiniRL) mini16.push_back({rl, 16});
        mini = gotoh = mini16;
        for (const int rl : {6, 8, 12, 16}) mini.push_back({rl, 64});   // (wide_rl_for)
        for (const int rl : {8, 16}) gotoh.push_back({rl, 64});         // (TbPlan::class_of, setup_gotoh_mini)
        std::vector<PairForm> v;
        auto add = [&](PairFamily fam, int mode, PairBand band, int walk, PairCells cells, PairGeom g) {
            v.push_back(PairForm{fam, mode, band, walk, cells, g.rl, g.w, fam == PF_MINI_SUBST ? tab : SubstRef{}});
        };
        for (const int mode : {PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG}) {
            const bool nw = mode == PWA_MODE_NW;
            for (const PairGeom g : stripe)   // setup_off_strips
                for (const PairCells c : {CELLS_PLAIN, CELLS_CODED, CELLS_GAP0})
                    if (c != CELLS_GAP0 || nw) add(PF_STRIPE_FILL, mode, BAND_NONE, WALK_NONE, c, g);
            for (const PairGeom g : mini16)
                for (const PairCells c : {CELLS_CODED, CELLS_GAP0})
                    if (c != CELLS_GAP0 || nw) add(PF_MINI_FILL, mode, BAND_NONE, WALK_NONE, c, g);
            for (const PairBand band : {BAND_TB, BAND_TB_SCORES})   // run_launch
                for (const int walk : {WALK_OPS, WALK_OVERLAP}) {
                    if (walk == WALK_OVERLAP && mode == PWA_MODE_SG) continue;
                    for (const PairGeom g : stripe)
                        for (const PairCells c : {CELLS_PLAIN, CELLS_KEYED, CELLS_CODED, CELLS_GAP0})
                            if ((c != CELLS_PLAIN || g.rl == 4) && (c != CELLS_GAP0 || (nw && band == BAND_TB))) add(PF_STRIPE_FILL, mode, band, walk, c, g);
                    for (const PairGeom g : mini)
                        for (const PairCells c : {CELLS_CODED, CELLS_GAP0})
                            if (c != CELLS_GAP0 || (nw && band == BAND_TB)) add(PF_MINI_FILL, mode, band, walk, c, g);
                }
            for (const PairGeom g : stripe)   // pwa_align_matrices
                for (const PairCells c : {CELLS_PLAIN, CELLS_KEYED})
                    if (c != CELLS_PLAIN || g.rl == 4) add(PF_STRIPE_FILL, mode, BAND_TB_SCORES, WALK_NONE, c, g);
            for (const PairGeom g : mini) add(PF_MINI_FILL, mode, BAND_TB_SCORES, WALK_NONE, CELLS_CODED, g);
            for (const PairGeom g : gotoh)   // setup_gotoh_mini, run_launch
                for (const PairFamily fam : {PF_MINI_GOTOH, PF_MINI_SUBST}) {
                    add(fam, mode, BAND_NONE, WALK_NONE, CELLS_KEYED, g);
                    add(fam, mode, BAND_TB, WALK_OPS, CELLS_KEYED, g);
                }
        }
        for (const PairGeom g : stripe) {   // setup_off_strips (hw4, hw3), affine_tb_on_stripes
            add(PF_STRIPE_DIST, PWA_MODE_NW, BAND_NONE, WALK_NONE, CELLS_PLAIN, g);
            add(PF_STRIPE_AFFINE, PWA_MODE_NW, BAND_NONE, WALK_NONE, CELLS_PLAIN, g);
            if (g.rl == 4) add(PF_STRIPE_AFFINE_TB, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_PLAIN, g);
        }
        return v;
    }();
    return listing;
}

// build() / build_mini(): the resolved form into the context's record (pwa_pair_forms)
static void note_pair_form(pwa_ctx* ctx, const PairForm& f) {
    std::string name = pair_form_name(f);
    if (std::find(ctx->pair_forms.begin(), ctx->pair_forms.end(), name) != ctx->pair_forms.end()) return;
    if (ctx->pair_forms.size() < pair_form_listing().size()) ctx->pair_forms.push_back(std::move(name));   // (bounded by the listing's size)
}

// ---- PairLaunch (pwalign_internal.h)
// one of a launch's six buffers, from where PairLaunch::mem says
static hipError_t take(pwa_ctx* ctx, const PairLaunch& pl, Lease& out, DevMem::Slot slot, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (pl.mem == PairLaunch::MEM_SLOTS) return workspace(ctx, slot, bytes, out);
    const hipError_t e = ctx->mem.lease(bytes, pl.mem == PairLaunch::MEM_FREE_LIST, out);
    return e == hipSuccess ? poison_device(&ctx->poison, out.get(), out.cap()) : e;
}
int PairLaunch::upload_desc(pwa_ctx* ctx, const std::vector<PairDesc>& pd) {
    const size_t bytes = pd.size() * sizeof(PairDesc);
    HIPC(ctx, take(ctx, *this, desc, DevMem::DESC, bytes));
    HIPC(ctx, ctx->pin[pwa_ctx::PIN_DESC].reserve(bytes));
    std::memcpy(ctx->pin[pwa_ctx::PIN_DESC].p, pd.data(), bytes);
    HIPC(ctx, hipMemcpy(desc.get(), ctx->pin[pwa_ctx::PIN_DESC].p, bytes, hipMemcpyHostToDevice));
    return PWA_OK;
}
// the fields of G that every launch sets (the callers add scores_out, dash, gap_extend of the gotoh families)
void PairLaunch::set_params(uint32_t n_pairs, uint32_t n_tasks, int match, int mismatch, int gap, int gap_extend) {
    G = PairParams{};
    G.pairs = desc.as<PairDesc>();
    G.n_pairs = n_pairs;
    G.n_tasks = n_tasks;
    G.queue = queue.as<uint32_t>();
    G.best = best.as<StripeBest>();
    G.match = match;
    G.mismatch = mismatch;
    G.gap = gap;
    G.gap_extend = gap_extend;
    G.dash = 0x100;   // no symbol: set by the callers that walk for overlaps
    G.trace_stripe = -1;
}
// pd[q].{pat,txt,n,m,tb,sband,res,ops,ops_cap} filled by the caller; this adds the pipeline fields
int PairLaunch::build(pwa_ctx* ctx, std::vector<PairDesc>& pd, const PairForm& f, int match, int mismatch, int gap, int gap_extend) {
    if (f.mini() || !resolve_pair_form(f, k)) return fail(ctx, PWA_E_INVALID, "internal: no stripe kernel for this form");
    form = f;
    note_pair_form(ctx, f);
    const uint64_t vals = f.family == PF_STRIPE_FILL ? 1 : 2;   // int32 values per hand-off column
    const uint64_t rows_per_stripe = 64ull * f.rl;
    std::vector<StripeTask> tl;
    uint64_t rows_i32 = 0, n_stripes_total = 0;
    for (size_t q = 0; q < pd.size(); ++q) {
        const uint64_t ns = ((uint64_t)pd[q].n + rows_per_stripe - 1) / rows_per_stripe;
        const uint64_t nsup = (ns + f.w - 1) / f.w;
        if (tl.size() + nsup >= 0xffffffffull || n_stripes_total + ns >= 0xffffffffull)
            return fail(ctx, PWA_E_CAPACITY, "too many stripe tasks in one launch");
        pd[q].first_task = (uint32_t)tl.size();
        pd[q].first_stripe = (uint32_t)n_stripes_total;
        pd[q].n_stripes = (uint32_t)ns;
        pd[q].row_stride = (uint32_t)align_up((uint64_t)pd[q].m + 64, 64);
        for (uint64_t st = 0; st < nsup; ++st) tl.push_back({(uint32_t)q, (uint32_t)st});
        rows_i32 += (nsup - 1) * pd[q].row_stride * vals;
        n_stripes_total += ns;
    }
    row_bytes = rows_i32 * sizeof(int32_t);
    HIPC(ctx, take(ctx, *this, rows, DevMem::ROWS, row_bytes));
    uint64_t ro = 0;
    for (auto& d : pd) {
        d.rows = rows.as<int32_t>() + ro;
        const uint64_t nsup = ((uint64_t)d.n_stripes + f.w - 1) / f.w;
        ro += (nsup - 1) * d.row_stride * vals;
    }
    if (const int rc = upload_desc(ctx, pd)) return rc;
    HIPC(ctx, take(ctx, *this, tasks, DevMem::TASKS, tl.size() * sizeof(StripeTask)));
    HIPC(ctx, ctx->pin[pwa_ctx::PIN_TL].reserve(tl.size() * sizeof(StripeTask)));
    std::memcpy(ctx->pin[pwa_ctx::PIN_TL].p, tl.data(), tl.size() * sizeof(StripeTask));
    HIPC(ctx, hipMemcpy(tasks.get(), ctx->pin[pwa_ctx::PIN_TL].p, tl.size() * sizeof(StripeTask), hipMemcpyHostToDevice));
    progress_bytes = align_up(tl.size() * sizeof(uint32_t), 16);
    HIPC(ctx, take(ctx, *this, progress, DevMem::PROGRESS, progress_bytes));
    HIPC(ctx, take(ctx, *this, best, DevMem::BEST, std::max<uint64_t>(n_stripes_total, 1) * sizeof(StripeBest)));
    HIPC(ctx, take(ctx, *this, queue, DevMem::QUEUE, 64));
    set_params((uint32_t)pd.size(), (uint32_t)tl.size(), match, mismatch, gap, gap_extend);
    G.tasks = tasks.as<StripeTask>();
    G.progress = progress.as<uint32_t>();
    n_stripes = n_stripes_total;
    // Tasks come off the queue in global order, so correctness does not depend on how many workgroups
    // are resident.  One workgroup = W compute waves + 1 helper wave.
    // [gpu] single-stripe batches (4096 pairs 150 x 10k, NW + band): 8 workgroups per CU 4.11 ms, 12 or 16: 3.76 ms (three
    // compute waves per SIMD fill the issue slots two leave open); the HBM-bound SW + score-band batch does not care
    int per_cu = f.w == 1 ? 12 : 3;
    if (ctx->knobs.wg_per_cu > 0) per_cu = ctx->knobs.wg_per_cu;   // experiments only
    grid = (uint32_t)std::min<uint64_t>(tl.size(), (uint64_t)ctx->num_cu * per_cu);
    return PWA_OK;
}
// mini-stripe engine: pd = the real pairs first (n_real of them), then empty patterns up to a multiple of four; task t = the
// pairs 4t .. 4t+3 (the caller orders them so that a task's texts are about equally long)
int PairLaunch::build_mini(pwa_ctx* ctx, std::vector<PairDesc>& pd, uint32_t n_real, const PairForm& f, int match, int mismatch, int gap) {
    if (!f.mini() || !resolve_pair_form(f, k)) return fail(ctx, PWA_E_INVALID, "internal: no mini-stripe kernel for this form");
    form = f;
    note_pair_form(ctx, f);
    const size_t ppw = (size_t)(64 / f.w);   // pairs per wave: 4, or 1 (one pair per wave: 512- / 1024-row single stripes)
    if (pd.empty() || pd.size() % ppw || pd.size() >= 0xffffffffull || n_real > pd.size() || n_real + ppw - 1 < pd.size())
        return fail(ctx, PWA_E_INVALID, "internal: mini-stripe task list");
    for (size_t q = 0; q < pd.size(); ++q) {
        pd[q].first_task = (uint32_t)(q / ppw);
        pd[q].first_stripe = (uint32_t)q;
        pd[q].n_stripes = 1;
        pd[q].row_stride = 0;
        pd[q].rows = nullptr;
    }
    if (const int rc = upload_desc(ctx, pd)) return rc;
    HIPC(ctx, take(ctx, *this, best, DevMem::BEST, pd.size() * sizeof(StripeBest)));
    HIPC(ctx, take(ctx, *this, queue, DevMem::QUEUE, 64));
    progress_bytes = 0;
    row_bytes = 0;
    set_params(n_real, (uint32_t)(pd.size() / ppw), match, mismatch, gap, 0);
    n_stripes = pd.size();
    grid = G.n_tasks;   // (clamped to what the chip holds at launch time, where the kernel is known)
    return PWA_OK;
}
// enqueue: zero the queue / progress words, fill, then the walk (or only the end-cell pick)
int PairLaunch::launch(pwa_ctx* ctx, hipStream_t st, hipEvent_t after_fill) {
    HIPC(ctx, hipMemsetAsync(queue.get(), 0, 16, st));
    const void* const fill_fn = k.sfill ? reinterpret_cast<const void*>(k.sfill) : reinterpret_cast<const void*>(k.fill);
    uint32_t g = grid;
    size_t pad_lds = 0;
    if (form.mini()) {
        // Workgroups of four waves (one task each per round); `per_cu` of them per CU, enforced through the dynamic LDS request, so
        // that no CU gets more than its share whatever ran before (mini_fill.hip.h): with ceil(tasks / 4) workgroups for 256 CUs,
        // per_cu = ceil(workgroups / CUs), at most 2; longer task lists run in rounds ([gpu] pairs 150 x 10k: 8192 of them at two
        // waves per SIMD 2.68 ms, 16384 at four 6.61 ms -- 16 k concurrent write streams get 4.0 instead of 4.9 TB/s out of HBM).
        const uint32_t n_wg = (G.n_tasks + kMiniWaves - 1) / kMiniWaves;
        // (band-less fills have no write streams to thin out: four per CU -- [gpu] scores with end cells 2 - 3 % faster than at two)
        const uint32_t cap_per_cu = ctx->knobs.mini_per_cu > 0 ? (uint32_t)std::min(ctx->knobs.mini_per_cu, 5) : (form.band != BAND_NONE ? 2u : 4u);
        const uint32_t per_cu = std::min<uint32_t>(cap_per_cu, (n_wg + (uint32_t)ctx->num_cu - 1) / (uint32_t)ctx->num_cu);
        static const uint32_t kPadKiB[6] = {0, 96, 64, 48, 36, 30};   // more than 160 KiB / (per_cu + 1), at most 160 KiB / per_cu
        // (the subst fills hold 4.25 KiB of LDS of their own: 5 KiB less padding keeps every per_cu inside the same two bounds)
        pad_lds = (size_t)(kPadKiB[per_cu] - (k.sfill ? 5 : 0)) * 1024;
        g = std::min<uint32_t>(n_wg, (uint32_t)ctx->num_cu * per_cu);
        if (ctx->knobs.debug) std::fprintf(stderr, "[pwa] mini fill: %u tasks, %u workgroups of %d waves, %u per CU (%zu KiB of LDS each)\n", G.n_tasks, g, kMiniWaves, per_cu, pad_lds >> 10);
    } else {
        HIPC(ctx, hipMemsetAsync(progress.get(), 0, progress_bytes, st));
        if (!ctx->knobs.stamps.empty()) {
            HIPC(ctx, stamps.alloc(ctx, n_stripes * 32 + 4 * 8192 * 8));
            HIPC(ctx, hipMemsetAsync(stamps.p, 0, n_stripes * 32 + 4 * 8192 * 8, st));
            G.stamps = stamps.as<unsigned long long>();
            G.trace_base = (uint32_t)(n_stripes * 4);
            G.trace_stripe = ctx->knobs.trace_stripe;
        }
        // A launch with no more multi-stripe workgroups than CUs asks for enough (unused) dynamic LDS that only ONE workgroup
        // fits a CU: a stripe is one wave alone on its SIMD, and every stripe of a pair moves at the pace of the slowest --
        // two workgroups sharing a CU's four SIMDs would slow the whole pipeline
        if (form.w > 1 && grid <= (uint32_t)ctx->num_cu && !ctx->knobs.no_lds_pad) pad_lds = 96 * 1024;   // static (<= 16 KiB) + 96 KiB > half of the CU's 160 KiB
    }
    // (the attribute is the kernel's, not this launch's: another live launch of the same kernel may have asked for another padding)
    if (form.mini() || pad_lds) HIPC(ctx, hipFuncSetAttribute(fill_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad_lds));
    if (k.sfill) hipLaunchKernelGGL(k.sfill, dim3(g), dim3(k.block), pad_lds, st, G, form.subst.tab, form.subst.n_sym, form.subst.stride);
    else hipLaunchKernelGGL(k.fill, dim3(g), dim3(k.block), pad_lds, st, G);
    HIPC(ctx, hipGetLastError());
    if (after_fill) HIPC(ctx, hipEventRecord(after_fill, st));
    if (!k.walks) return PWA_OK;
    hipLaunchKernelGGL(k.walk, dim3(G.n_pairs), dim3(64), 0, st, G);   // one wave per pair
    HIPC(ctx, hipGetLastError());
    return PWA_OK;
}
// after the stream has been synchronised: did a bounded spin give up?
int PairLaunch::check(pwa_ctx* ctx) {
    if (const char* path = ctx->knobs.stamps.c_str(); !ctx->knobs.stamps.empty() && stamps.p) {
        std::vector<unsigned long long> h(n_stripes * 4);
        HIPC(ctx, hipMemcpy(h.data(), stamps.p, n_stripes * 32, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(path, "w")) {
            for (uint64_t k = 0; k < n_stripes; ++k)
                std::fprintf(f, "%llu %llu %llu %llu %llu\n", (unsigned long long)k, h[4 * k] - h[0], h[4 * k + 3] - h[0], h[4 * k + 1] - h[0], h[4 * k + 2] - h[0]);
            std::fclose(f);
        }
        if (G.trace_stripe >= 0) {
            std::vector<unsigned long long> tr(4 * 8192);
            HIPC(ctx, hipMemcpy(tr.data(), stamps.as<unsigned long long>() + G.trace_base, tr.size() * 8, hipMemcpyDeviceToHost));
            if (FILE* f = std::fopen((std::string(path) + ".trace").c_str(), "w")) {
                for (int c = 0; c < 8192; ++c)
                    std::fprintf(f, "%d %llu %llu %llu %llu\n", c, tr[c] - h[0], tr[8192 + c] - h[0], tr[2 * 8192 + c] - h[0], tr[3 * 8192 + c] - h[0]);
                std::fclose(f);
            }
        }
    }
    uint32_t q[2] = {0, 0};
    HIPC(ctx, hipMemcpy(q, queue.get(), sizeof q, hipMemcpyDeviceToHost));
    if (q[1] != 0) return fail(ctx, PWA_E_HIP, "stripe pipeline timed out waiting for the stripe above");
    return PWA_OK;
}

// ---- BandedForm -> kernels: the only caller of the banded units' pickers, which read any rl as 4 or 8 and any mode as one of the three.
// EXT is an extension over NW's matrix: no other mode, and the walk over its band is NW's.
bool resolve_banded_form(const BandedForm& f, BandedKernels& k) {   // false: no such kernel
    k = BandedKernels{};
    if ((f.rl != 4 && f.rl != 8) || (f.mode != PWA_MODE_NW && f.mode != PWA_MODE_SW && f.mode != PWA_MODE_SG) || (f.ext && f.mode != PWA_MODE_NW)) return false;
    k.fill = f.ext ? (f.subst ? banded_ext_subst_kernel_for(f.rl, f.walk) : banded_ext_kernel_for(f.rl, f.walk))
             : f.subst ? banded_subst_kernel_for(f.rl, f.mode, f.walk)
             : f.walk  ? banded_kernel_for(f.rl, f.mode, false)
                       : banded_scores_kernel_for(f.rl, f.mode);
    if (f.walk) k.walk = banded_kernel_for(f.rl, f.mode, true);
    return k.fill && (k.walk || !f.walk);
}

// The fill's grid is what is resident at once -- the runtime's occupancy figure for this kernel (its VGPRs: 79 .. 248, two to six
// waves per SIMD) with this launch's hand-off rows in LDS -- and no more: pairs are dealt statically, longest first, so a workgroup
// that had to wait for a slot would run its whole share behind the others.  Only the dynamic LDS -- the hand-off rows -- is named to
// the runtime; it counts a table kernel's static SubstLds itself, both for the attribute's limit and for the occupancy figure.
hipError_t banded_launch(const BandedForm& f, const PairParams& G, int row_cap, int xdrop, const SubstRef& tab, int num_cu, hipStream_t st,
                         hipEvent_t after_fill) {
    BandedKernels k;
    if (!resolve_banded_form(f, k) || row_cap < 1 || row_cap > kBandedMaxWidth || !G.n_pairs || num_cu < 1) return hipErrorInvalidValue;
    if (f.subst && (!tab.tab || tab.n_sym < 1 || tab.n_sym > kSubstMaxSym || tab.stride < tab.n_sym || tab.stride > kSubstMaxSym)) return hipErrorInvalidValue;
    const size_t lds = (size_t)kBandedWaves * (size_t)row_cap * sizeof(bint2);
    hipError_t e = hipFuncSetAttribute(k.fill, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fill, 64 * kBandedWaves, lds)) != hipSuccess) return e;
    const uint32_t n_wg = (G.n_pairs + kBandedWaves - 1) / kBandedWaves;
    const uint32_t grid = std::min<uint32_t>(n_wg, (uint32_t)num_cu * (uint32_t)std::max(per_cu, 1));
    // the kernel's own parameter order: G, row_cap, then xdrop (EXT), then blob, n_sym, stride (a table)
    PairParams g = G;
    SubstRef t = tab;
    void* args[6] = {&g, &row_cap};
    int n_args = 2;
    if (f.ext) args[n_args++] = &xdrop;
    if (f.subst) args[n_args++] = &t.tab, args[n_args++] = &t.n_sym, args[n_args++] = &t.stride;
    if ((e = hipLaunchKernel(k.fill, dim3(grid), dim3(64 * kBandedWaves), args, lds, st)) != hipSuccess) return e;
    if (after_fill && (e = hipEventRecord(after_fill, st)) != hipSuccess) return e;
    if (!k.walk) return hipSuccess;
    void* walk_args[1] = {&g};
    return hipLaunchKernel(k.walk, dim3(G.n_pairs), dim3(64), walk_args, 0, st);   // one wave per pair
}

// A caller's substitution table, checked and laid out for the device: codes < n_sym for all 256 bytes, n_sym in 1 .. 32.  The table is
// stored with the text code as the row (a lane adds its pattern rows' offsets to one row address per step); the row stride is odd below
// 32 symbols, so that the rows of a small alphabet start in different LDS banks, and never more than 32 (4 KiB in all).
int subst_prepare(pwa_ctx* ctx, const uint8_t* code, int n_sym, const int32_t* submat, SubstTable& t) {
    if (!code || !submat) return fail(ctx, PWA_E_INVALID, "null input");
    if (n_sym < 1 || n_sym > kSubstMaxSym) return fail(ctx, PWA_E_INVALID, "n_sym must be 1 .. 32");
    for (int v = 0; v < 256; ++v)
        if (code[v] >= n_sym) return fail(ctx, PWA_E_INVALID, "code map: every one of the 256 entries must be below n_sym");
    t.n_sym = n_sym;
    t.stride = std::min(n_sym | 1, kSubstMaxSym);
    t.blob.assign((size_t)kSubstMapWords + kSubstTabWords, 0u);
    std::memcpy(t.blob.data(), code, 256);
    t.max_abs = 0;
    for (int cp = 0; cp < n_sym; ++cp)
        for (int ct = 0; ct < n_sym; ++ct) {
            const int32_t s = submat[cp * n_sym + ct];
            t.blob[(size_t)kSubstMapWords + (size_t)ct * t.stride + cp] = (uint32_t)s;
            t.max_abs = std::max<int64_t>(t.max_abs, std::llabs((long long)s));
        }
    return PWA_OK;
}
int subst_upload(pwa_ctx* ctx, SubstTable& t) {
    t.dev.pool = ctx;
    HIPC(ctx, t.dev.alloc(ctx, t.blob.size() * sizeof(uint32_t)));
    HIPC(ctx, upload_via_bounce(ctx, t.dev.p, t.blob.data(), t.blob.size() * sizeof(uint32_t)));
    return PWA_OK;
}

// the pair-list checks of the alignment batches
int check_pair_list(pwa_ctx* ctx, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, uint32_t n_seq) {
    if (n_pairs >= 0xffffffffull) return fail(ctx, PWA_E_CAPACITY, "more than 2^32-2 pairs in one batch");
    for (uint64_t k = 0; k < n_pairs; ++k)
        if (pair_a[k] >= n_seq || pair_b[k] >= n_seq) return fail(ctx, PWA_E_INVALID, "pair index out of range");
    return PWA_OK;
}

// Arena layout of the used sequences: s at aoff[s], 16-byte aligned, at least one byte of padding behind each and tail_pad bytes behind
// the last; returns the arena's size
uint64_t layout_arena(const uint64_t* seq_off, uint32_t n_seq, const std::vector<uint8_t>& is_used, uint64_t tail_pad, std::vector<uint64_t>& aoff) {
    aoff.assign(n_seq, 0);
    uint64_t arena_bytes = 0;
    for (uint32_t s = 0; s < n_seq; ++s)
        if (is_used[s]) {
            aoff[s] = arena_bytes;
            arena_bytes += align_up(seq_off[s + 1] - seq_off[s] + 1, 16);
        }
    return arena_bytes + tail_pad;
}

}  // namespace pwa

// pwa_selftest_host: every form the seven call sites of PairLaunch can build (pair_form_listing) resolves to kernels; so do the forms
// with a band and no walk that no call site asks for (pwa_align_matrices builds a few of them: those are listed); and a list of forms
// that mean nothing is refused.  (Kernel host stubs have addresses without a device.)
static int selftest_pair_forms() {
    static const uint32_t tab_word = 0;
    const SubstRef tab{&tab_word, 1, 1};
    const std::vector<PairGeom> stripe = {{2, 1}, {2, 4}, {4, 1}, {4, 4}};
    std::vector<PairGeom> mini;
    for (const int rl : kMiniRL) mini.push_back({rl, 16});
    for (const int rl : {6, 8, 12, 16}) mini.push_back({rl, 64});   // (wide_rl_for)
    int bad = 0;
    PairKernels k;
    for (const PairForm& f : pair_form_listing()) bad += !resolve_pair_form(f, k);
    auto must = [&](PairFamily fam, int mode, PairBand band, int walk, PairCells cells, PairGeom g) {
        bad += !resolve_pair_form(PairForm{fam, mode, band, walk, cells, g.rl, g.w}, k);
    };
    for (const int mode : {PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG})   // a band, the end-cell pick only: every cell form, either band
        for (const PairBand band : {BAND_TB, BAND_TB_SCORES}) {
            for (const PairGeom g : stripe)
                for (const PairCells c : {CELLS_PLAIN, CELLS_KEYED, CELLS_CODED, CELLS_GAP0})
                    if ((c != CELLS_PLAIN || g.rl == 4) && (c != CELLS_GAP0 || (mode == PWA_MODE_NW && band == BAND_TB))) must(PF_STRIPE_FILL, mode, band, WALK_NONE, c, g);
            for (const PairGeom g : mini)
                for (const PairCells c : {CELLS_CODED, CELLS_GAP0})
                    if (c != CELLS_GAP0 || (mode == PWA_MODE_NW && band == BAND_TB)) must(PF_MINI_FILL, mode, band, WALK_NONE, c, g);
        }
    if (bad) return 1;
    const PairForm none[] = {
        {PF_MINI_GOTOH, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 4, 4},             // a gotoh family with stripe geometry
        {PF_MINI_GOTOH, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 2, 16},
        {PF_MINI_SUBST, PWA_MODE_SW, BAND_NONE, WALK_NONE, CELLS_KEYED, 6, 64, tab},    // (the gotoh classes of 64 lanes: RL = 8 | 16)
        {PF_STRIPE_FILL, PWA_MODE_SG, BAND_TB, WALK_OPS, CELLS_GAP0, 4, 4},             // the gap shift: global only ...
        {PF_MINI_FILL, PWA_MODE_SG, BAND_NONE, WALK_NONE, CELLS_GAP0, 8, 16},
        {PF_STRIPE_FILL, PWA_MODE_SW, BAND_NONE, WALK_NONE, CELLS_GAP0, 4, 4},
        {PF_MINI_FILL, PWA_MODE_SW, BAND_TB, WALK_OPS, CELLS_GAP0, 8, 16},
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_TB_SCORES, WALK_OPS, CELLS_GAP0, 2, 4},      // ... and never with a score band
        {PF_MINI_FILL, PWA_MODE_NW, BAND_TB_SCORES, WALK_NONE, CELLS_GAP0, 16, 64},
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_PLAIN, 2, 4},            // the plain int32 traceback form at RL != 4
        {PF_STRIPE_FILL, PWA_MODE_SG, BAND_TB_SCORES, WALK_NONE, CELLS_PLAIN, 2, 1},
        {PF_STRIPE_FILL, PWA_MODE_SG, BAND_TB, WALK_OVERLAP, CELLS_CODED, 4, 4},        // no semi-global overlap walk
        {PF_MINI_FILL, PWA_MODE_SG, BAND_TB, WALK_OVERLAP, CELLS_CODED, 8, 16},
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_NONE, WALK_OPS, CELLS_CODED, 4, 4},          // a walk over a band that is not there
        {PF_MINI_FILL, PWA_MODE_NW, BAND_NONE, WALK_OVERLAP, CELLS_CODED, 4, 16},
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_NONE, WALK_NONE, CELLS_KEYED, 4, 4},         // no keyed band-less fill on raw bytes
        {PF_STRIPE_FILL, 3, BAND_TB, WALK_OPS, CELLS_KEYED, 4, 4},                      // unknown mode
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 3, 4},            // geometries without an instantiation
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 4, 2},
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 8, 16},
        {PF_MINI_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_CODED, 5, 16},
        {PF_MINI_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_CODED, 4, 64},
        {PF_MINI_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_CODED, 4, 1},
        {PF_MINI_FILL, PWA_MODE_NW, BAND_NONE, WALK_NONE, CELLS_CODED, 8, 64},          // (one pair per wave: band only)
        {PF_MINI_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 8, 16},             // the mini-stripe fills score by table
        {PF_STRIPE_DIST, PWA_MODE_SW, BAND_NONE, WALK_NONE, CELLS_PLAIN, 4, 4},         // hw4 / hw3: global, one form each
        {PF_STRIPE_DIST, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_PLAIN, 4, 4},
        {PF_STRIPE_AFFINE, PWA_MODE_NW, BAND_NONE, WALK_NONE, CELLS_GAP0, 4, 4},
        {PF_STRIPE_AFFINE_TB, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_PLAIN, 2, 4},
        {PF_STRIPE_AFFINE_TB, PWA_MODE_NW, BAND_TB, WALK_OVERLAP, CELLS_PLAIN, 4, 4},
        {PF_STRIPE_AFFINE_TB, PWA_MODE_NW, BAND_NONE, WALK_NONE, CELLS_PLAIN, 4, 4},
        {PF_MINI_GOTOH, PWA_MODE_NW, BAND_TB_SCORES, WALK_OPS, CELLS_KEYED, 8, 16},     // the gotoh kernels write no score band ...
        {PF_MINI_GOTOH, PWA_MODE_NW, BAND_TB, WALK_OVERLAP, CELLS_KEYED, 8, 16},        // ... and walk for op lists only
        {PF_MINI_GOTOH, PWA_MODE_NW, BAND_TB, WALK_NONE, CELLS_KEYED, 8, 16},
        {PF_MINI_GOTOH, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_CODED, 8, 16},
        {PF_MINI_GOTOH, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 8, 16, tab},       // a table without the subst family, and the reverse
        {PF_STRIPE_FILL, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 4, 4, tab},
        {PF_MINI_SUBST, PWA_MODE_NW, BAND_TB, WALK_OPS, CELLS_KEYED, 8, 16},
    };
    for (const PairForm& f : none)
        if (resolve_pair_form(f, k)) return 2;
    return 0;
}

// ... and that the listing's forms resolve to the RIGHT number of kernels: no form twice (1); two forms that differ in a field the fill
// depends on -- anything but the walk -- have different fills (2); the walk is a function of (engine class, rl, lanes, mode, walk)
// alone (3) and differs whenever one of the five does (4).  Engine class: the stripe fills, hw3's alignment, the mini-stripe fills, the
// gotoh kernels (whose walk the subst family shares); a stripe walk is one wave per pair whatever W is: 64 lanes.
static int selftest_pair_listing() {
    struct Key {
        int a[6];
        bool operator<(const Key& o) const { return std::lexicographical_compare(a, a + 6, o.a, o.a + 6); }
        bool operator==(const Key& o) const { return std::equal(a, a + 6, o.a); }
    };
    std::vector<std::pair<Key, const void*>> fills, walks;
    std::vector<std::string> names;
    PairKernels k;
    for (const PairForm& f : pair_form_listing()) {
        if (!resolve_pair_form(f, k)) return 1;
        names.push_back(pair_form_name(f));
        fills.push_back({Key{{f.family, f.mode, f.band, f.cells, f.rl, f.w}}, k.sfill ? reinterpret_cast<const void*>(k.sfill) : reinterpret_cast<const void*>(k.fill)});
        if (!k.walks) continue;
        const int cls = f.family == PF_STRIPE_FILL ? 0 : f.family == PF_STRIPE_AFFINE_TB ? 1 : f.family == PF_MINI_FILL ? 2 : 3;
        walks.push_back({Key{{cls, f.rl, f.mini() ? f.w : 64, f.mode, f.walk, 0}}, reinterpret_cast<const void*>(k.walk)});
    }
    std::sort(names.begin(), names.end());
    if (names.empty() || std::adjacent_find(names.begin(), names.end()) != names.end()) return 1;
    // sorted by key, then by pointer: equal keys are neighbours; sorted by pointer: equal pointers are
    int at = 2;
    for (auto* v : {&fills, &walks}) {
        std::sort(v->begin(), v->end());
        for (size_t i = 1; i < v->size(); ++i)
            if ((*v)[i].first == (*v)[i - 1].first && (*v)[i].second != (*v)[i - 1].second) return v == &fills ? 1 : 3;   // (a fill key twice is a form twice)
        v->erase(std::unique(v->begin(), v->end()), v->end());
        std::sort(v->begin(), v->end(), [](const auto& x, const auto& y) { return x.second < y.second; });
        for (size_t i = 1; i < v->size(); ++i)
            if ((*v)[i].second == (*v)[i - 1].second) return at;
        at = 4;
    }
    return 0;
}

// ... and the banded class: the 32 forms run_banded_launch can build resolve (the 24 plain ones, the 8 of EXT over NW's matrix), each
// to a fill of its own; a score pass has no walk, a fill has the walk of the byte-compare fill of its rl and mode (EXT: NW's), six in
// all; geometries, modes and EXT combinations that mean nothing are refused.
static int selftest_banded_forms() {
    std::vector<const void*> fills, walks;
    BandedKernels k, plain;
    for (const int rl : {4, 8})
        for (const int mode : {PWA_MODE_NW, PWA_MODE_SW, PWA_MODE_SG})
            for (const bool ext : {false, true})
                for (const bool subst : {false, true})
                    for (const bool walk : {false, true}) {
                        if (ext && mode != PWA_MODE_NW) continue;
                        if (!resolve_banded_form(BandedForm{rl, mode, ext, subst, walk}, k) || !k.fill) return 1;
                        if (!resolve_banded_form(BandedForm{rl, mode, false, false, true}, plain)) return 1;
                        if (k.walk != (walk ? plain.walk : nullptr)) return 2;
                        fills.push_back(k.fill);
                        if (!ext && !subst && walk) walks.push_back(k.walk);
                    }
    for (std::vector<const void*>* v : {&fills, &walks}) {
        std::sort(v->begin(), v->end());
        if (std::adjacent_find(v->begin(), v->end()) != v->end()) return 2;
    }
    if (fills.size() != 32 || walks.size() != 6 || !walks[0]) return 2;
    const BandedForm none[] = {
        {2, PWA_MODE_NW, false, false, true},   // stripe heights without an instantiation
        {6, PWA_MODE_SW, false, true, false},
        {16, PWA_MODE_NW, true, false, true},
        {4, 3, false, false, true},             // unknown mode
        {8, 3, false, true, false},
        {4, PWA_MODE_SW, true, false, true},    // EXT is NW's matrix
        {8, PWA_MODE_SW, true, true, false},
        {4, PWA_MODE_SG, true, true, true},
        {8, PWA_MODE_SG, true, false, false},
    };
    for (const BandedForm& f : none)
        if (resolve_banded_form(f, k)) return 3;
    return 0;
}

// ... and DevMem's policy (dev_mem.h; DESIGN.md 3.20, "The allocation rule") over a fake device: a byte budget, addresses that are
// never dereferenced, every call counted, every free checked against what is live.  The return value names the rule that broke:
// 1 a slot big enough is reused without a call; 2 it is regrown with one free and one malloc; 3 a request beyond kBandCacheMax leaves
// the slot alone and its buffer goes with the lease; 4 best fit takes the smallest admissible buffer of the free list; 5 none larger
// than 2 n + 1 MiB; 6 the list's count and byte caps; 7 parking a larger hand-off buffer moves the displaced one to the list without a
// free; 8 a parked buffer that is too small stays parked; 9 out of memory frees the list and the parked buffer and the second try
// succeeds; 10 a leased slot survives that; 11 with nothing idle the failure comes back after exactly one retry; 12 the destructor
// frees every slot, the parked buffer and the list once each; 13 nothing is left live and nothing was freed twice.
namespace {
struct FakeDev {
    std::vector<std::pair<void*, size_t>> live;
    size_t budget = ~size_t(0), used = 0, mallocs = 0, frees = 0, bad_frees = 0;
    uintptr_t next = 0x1000;
    bool is_live(const void* p) const {
        return std::any_of(live.begin(), live.end(), [&](const auto& b) { return b.first == p; });
    }
};
thread_local FakeDev fake;   // (DevMem's allocator is a plain function pointer)
hipError_t fake_malloc(void** p, size_t n) {
    ++fake.mallocs;
    *p = nullptr;
    if (n > fake.budget - fake.used) return hipErrorOutOfMemory;
    *p = reinterpret_cast<void*>(fake.next);
    fake.next += 0x1000;
    fake.used += n;
    fake.live.emplace_back(*p, n);
    return hipSuccess;
}
hipError_t fake_free(void* p) {
    ++fake.frees;
    for (size_t i = 0; i < fake.live.size(); ++i)
        if (fake.live[i].first == p) {
            fake.used -= fake.live[i].second;
            fake.live.erase(fake.live.begin() + (long)i);
            return hipSuccess;
        }
    ++fake.bad_frees;
    return hipErrorInvalidValue;
}
}  // namespace
static int selftest_dev_mem() {
    constexpr size_t MiB = 1u << 20;
    FakeDev& f = fake;
    auto calls = [&](size_t mallocs, size_t frees) { return f.mallocs == mallocs && f.frees == frees; };
    auto fresh = [&](DevMem& m, size_t n, void** p) {   // a buffer of exactly n bytes, not from the list
        size_t got = 0;
        return m.buffer(n, false, p, &got) == hipSuccess && *p && got == n;
    };
    void *p = nullptr, *q[3] = {};
    size_t got = 0;
    f = FakeDev{};
    {   // slots
        DevMem m(fake_malloc, fake_free);
        Lease a, b;
        if (m.workspace(DevMem::RES, 1000, a) != hipSuccess || !a.get() || a.cap() != 1000 || !calls(1, 0)) return 1;
        void* const p0 = a.get();
        if (m.workspace(DevMem::RES, 600, a) != hipSuccess || a.get() != p0 || a.cap() != 1000 || !calls(1, 0)) return 1;
        if (m.workspace(DevMem::RES, 1001, a) != hipSuccess || a.cap() != 1001 || !calls(2, 1) || f.is_live(p0) || f.used != 1001) return 2;
        if (m.workspace(DevMem::RES, kBandCacheMax + 1, b) != hipSuccess || b.get() == a.get() || b.cap() != kBandCacheMax + 1 || !calls(3, 1)) return 3;
        void* const big = b.get();
        b.release();
        if (!calls(3, 2) || f.is_live(big) || m.workspace(DevMem::RES, 1001, b) != hipSuccess || b.get() != a.get() || !calls(3, 2)) return 3;
        // the free list: 3, 2 and 8 MiB kept
        const size_t sizes[3] = {3 * MiB, 2 * MiB, 8 * MiB};
        for (int i = 0; i < 3; ++i) {
            if (!fresh(m, sizes[i], &q[i])) return 4;
            m.keep(q[i], sizes[i]);
        }
        if (!calls(6, 2)) return 4;
        if (m.buffer(3 * MiB / 2, true, &p, &got) != hipSuccess || p != q[1] || got != 2 * MiB || !calls(6, 2)) return 4;   // 2 and 3 MiB are admissible
        m.keep(p, got);
        if (!fresh(m, 2 * MiB, &p) || p == q[1] || !calls(7, 2)) return 4;   // an un-pooled request never takes from the list
        m.drop(p);
        if (m.buffer(7 * MiB / 2 - 1, true, &p, &got) != hipSuccess || p == q[2] || got != 7 * MiB / 2 - 1 || !calls(8, 3)) return 5;   // 8 MiB > 2 n + 1 MiB
        m.drop(p);
        if (m.buffer(7 * MiB / 2, true, &p, &got) != hipSuccess || p != q[2] || got != 8 * MiB || !calls(8, 4)) return 5;   // ... = 2 n + 1 MiB
        m.drop(p);
    }
    if (!calls(8, 8) || !f.live.empty() || f.bad_frees) return 12;   // (the slot and the two kept buffers)
    f = FakeDev{};
    {   // the list's caps
        DevMem m(fake_malloc, fake_free);
        for (size_t i = 0; i <= DevMem::kListMaxCount; ++i) {
            if (!fresh(m, 16, &p)) return 6;
            m.keep(p, 16);
            if (f.frees != (i == DevMem::kListMaxCount ? 1u : 0u)) return 6;
        }
    }
    if (!f.live.empty() || f.bad_frees) return 12;
    f = FakeDev{};
    {
        DevMem m(fake_malloc, fake_free);
        for (int i = 0; i < 4; ++i) {   // three buffers fill the list's bytes exactly; 16 bytes more are refused
            const size_t n = i < 3 ? DevMem::kListMaxBytes / 3 : 16;
            if (!fresh(m, n, &p)) return 6;
            m.keep(p, n);
            if (f.frees != (i < 3 ? 0u : 1u)) return 6;
        }
    }
    if (!f.live.empty() || f.bad_frees) return 12;
    f = FakeDev{};
    {   // the hand-off buffer
        DevMem m(fake_malloc, fake_free);
        if (!fresh(m, 1000, &q[0]) || !fresh(m, 2000, &q[1])) return 7;
        m.park_hand(q[0], 1000);
        m.park_hand(q[1], 2000);   // displaces the first one ...
        if (!calls(2, 0) || m.buffer(1000, true, &p, &got) != hipSuccess || p != q[0] || got != 1000 || !calls(2, 0)) return 7;   // ... onto the list
        m.park_hand(q[0], 1000);   // the smaller one is refused: the list again
        if (!calls(2, 0) || m.buffer(1000, true, &p, &got) != hipSuccess || p != q[0] || !calls(2, 0)) return 7;
        m.drop(p);
        if (m.take_hand(2001, &p, &got) || !m.take_hand(2000, &p, &got) || p != q[1] || got != 2000 || m.take_hand(1, &p, &got) || !calls(2, 1)) return 8;
        m.drop(q[1]);
    }
    if (!calls(2, 2) || !f.live.empty() || f.bad_frees) return 12;
    f = FakeDev{};
    f.budget = 10000;
    {   // out of memory
        DevMem m(fake_malloc, fake_free);
        Lease res, band, ops;
        if (m.workspace(DevMem::RES, 3000, res) != hipSuccess || !fresh(m, 3000, &q[0]) || !fresh(m, 3000, &q[1])) return 9;
        m.keep(q[0], 3000);
        m.park_hand(q[1], 3000);
        if (m.workspace(DevMem::BAND, 4000, band) != hipSuccess || !band.get() || f.mallocs != 5 || f.is_live(q[0]) || f.is_live(q[1])) return 9;
        if (!f.is_live(res.get()) || !calls(5, 2) || m.workspace(DevMem::RES, 3000, ops) != hipSuccess || ops.get() != res.get() || !calls(5, 2)) return 10;
        if (m.workspace(DevMem::OPS, 5000, ops) != hipErrorOutOfMemory || ops.get() || !calls(7, 2) || !f.is_live(res.get()) || !f.is_live(band.get())) return 11;
        if (m.buffer(5000, true, &p, &got) != hipErrorOutOfMemory || p || got || !calls(9, 2)) return 11;
        if (!fresh(m, 1000, &q[0]) || !fresh(m, 1000, &q[1])) return 12;
        m.keep(q[0], 1000);
        m.park_hand(q[1], 1000);
        if (!calls(11, 2) || f.live.size() != 4) return 12;
    }
    if (!calls(11, 6) || f.bad_frees) return 12;   // two slots, the parked buffer, the list
    return f.live.empty() && f.used == 0 ? 0 : 13;
}

extern "C" {

const char* pwa_version(void) { return "pwalign 0.1 gfx950"; }

// Host-only checks of the scheduler's sorting helpers, of the alignment batches' range planner (include/pwalign.h) and of the wavefront
// unit's: tests call this on machines without a GPU.
int pwa_selftest_host(uint32_t seed) try {
    uint64_t x = 0x9e3779b97f4a7c15ull ^ seed;
    auto rnd = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    int check = 0;
    for (const size_t n : {size_t(0), size_t(1), size_t(2), size_t(1000), size_t(70000), size_t(300000), size_t(1) << 20}) {
        for (const size_t buckets : {size_t(1), size_t(3), size_t(4352), size_t(65536), size_t(200000)}) {
            ++check;
            std::vector<uint32_t> key(n), idx(n), tmp, want(n);
            for (size_t i = 0; i < n; ++i) {
                key[i] = (uint32_t)(rnd() % buckets);
                idx[i] = (uint32_t)i;
            }
            want = idx;
            std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
            counting_sort(idx, tmp, buckets, [&](uint32_t v) { return (size_t)key[v]; });   // (threaded from 2^18 elements, <= 2^16 buckets)
            if (idx != want) return check;
        }
        for (const uint64_t span : {uint64_t(1), uint64_t(7), uint64_t(3000), uint64_t(1) << 33}) {   // the last one takes the radix path
            ++check;
            std::vector<uint64_t> len(n);
            std::vector<uint32_t> idx(n), want(n);
            for (size_t i = 0; i < n; ++i) {
                len[i] = 5 + rnd() % span;
                idx[i] = (uint32_t)i;
            }
            want = idx;
            std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return len[a] > len[b]; });
            sort_by_length_desc(idx, [&](uint32_t v) { return len[v]; });
            if (idx != want) return check;
        }
        {
            ++check;
            std::vector<uint64_t> key(n);
            std::vector<uint32_t> idx(n), want(n);
            for (size_t i = 0; i < n; ++i) {
                key[i] = rnd() >> (rnd() % 50);
                idx[i] = (uint32_t)i;
            }
            want = idx;
            const std::vector<uint64_t> key0 = key;
            std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key0[a] < key0[b]; });
            radix_sort_by_key(key, idx);
            if (idx != want) return check;
        }
    }
    {   // PWA_POISON's value: decimal or 0x.., 0 .. 255, nothing else; unset is not an error
        ++check;
        static const struct { const char* s; int want; } cases[] = {
            {nullptr, -1}, {"0", 0}, {"1", 1}, {"255", 255}, {"0x00", 0}, {"0x80", 128}, {"0X7f", 127}, {"0xFF", 255}, {"0xff", 255}, {"007", 7},
            {"", -2}, {"256", -2}, {"0x100", -2}, {"0x", -2}, {"-1", -2}, {"+1", -2}, {" 1", -2}, {"1 ", -2}, {"12a", -2}, {"ff", -2}, {"0xg", -2},
            {"4294967297", -2}, {"0x100000001", -2}, {"1.0", -2}, {"true", -2},
        };
        for (const auto& c : cases)
            if (parse_poison(c.s) != c.want) return check;
    }
    {   // cut_runs (side_unit.h): the edge cases by hand, then random lists against what defines the cut -- the runs tile 0 .. n in order,
        // a run's weight is its items' sum, a run of several items fits the budget, and the item after a run would not have fitted
        ++check;
        static const struct {
            uint64_t n, budget, w[5], runs, want[3][3];
        } cases[] = {
            {0, 5, {}, 0, {}},                                               // nothing to cut
            {3, 5, {10, 1, 1}, 2, {{0, 1, 10}, {1, 3, 2}}},                  // a first item that alone exceeds the budget
            {1, 5, {9}, 1, {{0, 1, 9}}},
            {3, 0, {0, 0, 0}, 1, {{0, 3, 0}}},                               // zero weights
            {5, 4, {0, 0, 5, 0, 0}, 3, {{0, 2, 0}, {2, 3, 5}, {3, 5, 0}}},
            {5, 5, {1, 0, 4, 0, 1}, 2, {{0, 4, 5}, {4, 5, 1}}},
            {3, 4, {2, 2, 2}, 2, {{0, 2, 4}, {2, 3, 2}}},                    // an exact fit
        };
        for (const auto& c : cases) {
            const std::vector<Run> got = cut_runs(c.n, c.budget, [&](uint64_t k) { return c.w[k]; });
            if (got.size() != c.runs) return check;
            for (size_t r = 0; r < got.size(); ++r)
                if (got[r].k0 != c.want[r][0] || got[r].k1 != c.want[r][1] || got[r].weight != c.want[r][2]) return check;
        }
        for (int rep = 0; rep < 200; ++rep) {
            const uint64_t budget = rnd() % 40;
            std::vector<uint64_t> w(rnd() % 30);
            for (uint64_t& e : w) e = rnd() % 4 ? rnd() % 25 : 0;
            uint64_t at = 0;
            for (const Run& r : cut_runs(w.size(), budget, [&](uint64_t k) { return w[k]; })) {
                uint64_t sum = 0;
                for (uint64_t k = r.k0; k < r.k1; ++k) sum += w[k];
                if (r.k0 != at || r.k1 <= r.k0 || r.k1 > w.size() || r.weight != sum || (r.k1 - r.k0 > 1 && sum > budget) || (r.k1 < w.size() && sum + w[r.k1] <= budget))
                    return check;
                at = r.k1;
            }
            if (at != w.size()) return check;
        }
    }
    if (const int rc = selftest_pair_forms()) return check + rc;
    if (const int rc = selftest_banded_forms()) return check + 2 + rc;
    if (const int rc = selftest_align_plan(x, check + 5)) return rc;
    if (const int rc = selftest_wfa_plan(x, check + 11)) return rc;
    if (const int rc = selftest_pair_listing()) return check + 16 + rc;   // (the wavefront planner's checks end at check + 16)
    if (const int rc = selftest_dev_mem()) return check + 20 + rc;
    return 0;
} catch (...) {
    return -1;
}

int pwa_pair_form_table(uint32_t index, const char** name, uint32_t* count) try {
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v;
        for (const PairForm& f : pair_form_listing()) v.push_back(pair_form_name(f));
        return v;
    }();
    if (count) *count = (uint32_t)names.size();
    if (index >= names.size()) return PWA_E_INVALID;
    if (name) *name = names[index].c_str();
    return PWA_OK;
} catch (...) {
    return PWA_E_NOMEM;
}

int pwa_pair_forms(const pwa_ctx* ctx, char* buf, uint64_t cap, uint64_t* needed) try {
    if (!ctx) return PWA_E_INVALID;
    std::string s;
    for (const std::string& n : ctx->pair_forms) s += (s.empty() ? "" : "\n") + n;
    if (needed) *needed = s.size() + 1;
    if (!buf || cap < s.size() + 1) return PWA_E_CAPACITY;
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return PWA_OK;
} catch (...) {
    return PWA_E_NOMEM;
}

int pwa_pair_forms_reset(pwa_ctx* ctx) {
    if (!ctx) return PWA_E_INVALID;
    ctx->pair_forms.clear();
    return PWA_OK;
}

const char* pwa_strerror(int code) {
    switch (code) {
        case PWA_OK: return "ok";
        case PWA_E_INVALID: return "invalid argument";
        case PWA_E_NODEVICE: return "no usable gfx950 device";
        case PWA_E_HIP: return "HIP runtime error";
        case PWA_E_NOMEM: return "out of memory";
        case PWA_E_CAPACITY: return "capacity exceeded";
        case PWA_E_IO: return "cannot open or read file";
        default: return "unknown error";
    }
}

int pwa_ctx_create(int device, pwa_ctx** out) {
    if (!out) return PWA_E_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return PWA_E_NODEVICE;
    if (device < 0 || device >= count) return PWA_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return PWA_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PWA_E_NODEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PWA_E_NODEVICE;   // kernels exist for gfx950 only
    pwa_ctx* c = new (std::nothrow) pwa_ctx();
    if (!c) return PWA_E_NOMEM;
    c->knobs.read();   // the only place the library's switches are read from the environment
    if (c->knobs.poison == -2) {   // PWA_POISON set to something that is no byte: a run that poisons nothing must not look like one that does
        delete c;
        return PWA_E_INVALID;
    }
    c->poison.byte = c->knobs.poison;
    c->poison.device = device;
    for (PinnedBuf& pb : c->pin) pb.poison = &c->poison;
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return PWA_E_HIP;
    }
    for (auto& e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            pwa_ctx_destroy(c);
            return PWA_E_HIP;
        }
    if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->copy_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->copy_ev[1], hipEventDisableTiming) != hipSuccess || hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->aux_ev[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->aux_ev[1], hipEventDisableTiming) != hipSuccess) {
        pwa_ctx_destroy(c);
        return PWA_E_HIP;
    }
    *out = c;
    return PWA_OK;
}

void pwa_ctx_destroy(pwa_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    for (auto& e : c->copy_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (auto& e : c->aux_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    delete c;
}

const char* pwa_last_error(const pwa_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pwa_ctx_poison_stats(const pwa_ctx* c, uint64_t* buffers, uint64_t* bytes) {
    if (!c) return PWA_E_INVALID;
    if (buffers) *buffers = c->poison.buffers;
    if (bytes) *bytes = c->poison.bytes;
    return PWA_OK;
}

int pwa_ctx_set_score_band(pwa_ctx* c, int on) {
    if (!c) return PWA_E_INVALID;
    c->score_band = on != 0;
    return PWA_OK;
}

}  // extern "C"
