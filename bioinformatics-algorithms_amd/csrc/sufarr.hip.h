// sufarr.hip.h -- the suffix-array index of hw1_amd: prefix doubling over a stable device LSD radix sort,
// binary search of many patterns, occurrence lists.  Self-contained: none of the alignment templates.
//
// Every kernel is a plain data-parallel pass.  Nothing waits on another workgroup: the radix sort and the scans are
// reduce-then-scan (per-tile counts, a separate scan launch, a separate apply launch), so the non-coherent per-XCD L2s
// never see a hand-off inside a launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pwa {
namespace sufarr {

constexpr int kThreads = 256;                    // every kernel below: four waves
constexpr int kItems = 16;                       // elements per thread of a radix-sort tile / a scan chunk
constexpr int kTile = kThreads * kItems;         // 4096 elements per tile
constexpr int kRadixBits = 8;
constexpr int kBuckets = 1 << kRadixBits;

// ------------------------------------------------------------------------------------------------------------ scans
// Exclusive prefix of v over the workgroup (256 threads); *total gets the sum.  lds: 4 words.
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) {
        const uint32_t s = lds[i];
        before += i < w ? s : 0u;
        all += s;
    }
    __syncthreads();   // lds may be reused by the caller's next scan
    *total = all;
    return before + x - v;
}

// x[c0 .. c0 + kTile) (clipped to len) := carry + exclusive prefix; returns the chunk's sum.
__device__ inline uint32_t scan_chunk(uint32_t* x, size_t c0, size_t len, uint32_t carry, uint32_t* lds) {
    const size_t b = c0 + (size_t)threadIdx.x * kItems;
    uint32_t v[kItems], s = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        v[j] = b + j < len ? x[b + j] : 0u;
        s += v[j];
    }
    uint32_t total;
    uint32_t run = carry + block_excl_scan(s, lds, &total);
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        if (b + j < len) x[b + j] = run;
        run += v[j];
    }
    return total;
}

// part[chunk] := sum of x over the chunk
__global__ __launch_bounds__(kThreads) void scan_reduce_kernel(const uint32_t* x, size_t len, uint32_t* part) {
    __shared__ uint32_t lds[4];
    const size_t b = (size_t)blockIdx.x * kTile + (size_t)threadIdx.x * kItems;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) s += b + j < len ? x[b + j] : 0u;
    uint32_t total;
    (void)block_excl_scan(s, lds, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the chunk sums, in place
__global__ __launch_bounds__(kThreads) void scan_partials_kernel(uint32_t* part, uint32_t n_part) {
    __shared__ uint32_t lds[4];
    uint32_t carry = 0;
    for (size_t c0 = 0; c0 < n_part; c0 += kTile) carry += scan_chunk(part, c0, n_part, carry, lds);
}

__global__ __launch_bounds__(kThreads) void scan_apply_kernel(uint32_t* x, size_t len, const uint32_t* part) {
    __shared__ uint32_t lds[4];
    (void)scan_chunk(x, (size_t)blockIdx.x * kTile, len, part[blockIdx.x], lds);
}

// ------------------------------------------------------------------------------------------------------- radix sort
// Which key bits vary: OR and AND over all keys (first launch over the keys, second, one workgroup, over the partials).
template <class K>
__global__ __launch_bounds__(kThreads) void key_bits_kernel(const K* in_or, const K* in_and, size_t n, K* out_or, K* out_and) {
    __shared__ K s_or[4], s_and[4];
    K o = 0, a = ~K(0);
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        o |= in_or[i];
        a &= in_and[i];
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        o |= __shfl_xor(o, d, 64);
        a &= __shfl_xor(a, d, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        s_or[w] = o;
        s_and[w] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out_or[blockIdx.x] = s_or[0] | s_or[1] | s_or[2] | s_or[3];
        out_and[blockIdx.x] = s_and[0] & s_and[1] & s_and[2] & s_and[3];
    }
}

// Per-tile digit counts, digit-major: hist[d * n_tiles + tile].  One sub-histogram per wave keeps LDS atomics on a
// skewed digit from serialising the whole workgroup.
template <class K>
__global__ __launch_bounds__(kThreads) void radix_hist_kernel(const K* key, size_t n, int shift, uint32_t* hist, uint32_t n_tiles) {
    __shared__ uint32_t h[4][kBuckets];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q][threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kTile + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < kItems; ++j) {
        const size_t i = base + (size_t)j * kThreads;
        if (i < n) atomicAdd(&h[w][(uint32_t)(key[i] >> shift) & (kBuckets - 1)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
}

// Stable scatter of one tile: off[d * n_tiles + tile] (the scanned histogram) is where the tile's first element of digit d
// goes.  The tile is walked in element order, 256 elements per step (element = step * 256 + thread): within a wave the
// elements of a digit are ranked by a ballot match (8 ballots), across the four waves by their counts in LDS, across steps
// by a running count per digit.  Counts alternate between two LDS buffers so that a step's clearing never races the next
// step's writes.
template <class K, class V>
__global__ __launch_bounds__(kThreads) void radix_scatter_kernel(const K* kin, const V* vin, K* kout, V* vout, size_t n, int shift,
                                                                  const uint32_t* off, uint32_t n_tiles) {
    __shared__ uint32_t run[kBuckets];
    __shared__ uint32_t cnt[2][4][kBuckets];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    run[threadIdx.x] = off[(size_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
    for (int q = 0; q < 4; ++q) cnt[0][q][threadIdx.x] = cnt[1][q][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    const size_t base = (size_t)blockIdx.x * kTile + threadIdx.x;
    for (int j = 0; j < kItems; ++j) {
        const size_t i = base + (size_t)j * kThreads;
        const bool ok = i < n;
        const K k = ok ? kin[i] : K(0);
        const V v = ok ? vin[i] : V(0);
        const uint32_t d = (uint32_t)(k >> shift) & (kBuckets - 1);
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < kRadixBits; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const int buf = j & 1;
        const uint32_t r = (uint32_t)__popcll(peers & below);
        if (ok && r == 0) cnt[buf][w][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (ok) {
            uint32_t pos = run[d] + r;
            for (int q = 0; q < w; ++q) pos += cnt[buf][q][d];
            kout[pos] = k;
            vout[pos] = v;
        }
        __syncthreads();
        run[threadIdx.x] += cnt[buf][0][threadIdx.x] + cnt[buf][1][threadIdx.x] + cnt[buf][2][threadIdx.x] + cnt[buf][3][threadIdx.x];
#pragma unroll
        for (int q = 0; q < 4; ++q) cnt[buf][q][threadIdx.x] = 0;
    }
}

// ------------------------------------------------------------------------------------------------- prefix doubling
struct CodeTable {
    uint16_t c[256];   // byte -> code 1..sigma in signed-char order (0 = past the end of the text); sigma <= 256
};

// key[i] = the codes of t[i .. i + k), first byte most significant, bits per code; val[i] = i
__global__ __launch_bounds__(kThreads) void sa_first_key_kernel(const uint8_t* t, uint32_t n, const CodeTable tab, int bits, int k,
                                                                uint64_t* key, uint32_t* val) {
    __shared__ uint16_t lut[256];
    lut[threadIdx.x] = tab.c[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t x = 0;
    for (int j = 0; j < k; ++j) x = (x << bits) | (i + (uint32_t)j < n ? (uint64_t)lut[t[i + j]] : 0ull);
    key[i] = x;
    val[i] = i;
}

// head[j] = 1 where sorted key j starts a group; head[n] = 0 (so that the exclusive scan leaves the group count there)
__global__ __launch_bounds__(kThreads) void sa_heads_kernel(const uint64_t* key, uint32_t n, uint32_t* head) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n) head[j] = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
    else if (j == n) head[j] = 0;
}

// rank[sa[j]] = dense group number of j (scan = exclusive scan of the heads)
__global__ __launch_bounds__(kThreads) void sa_rank_kernel(const uint64_t* key, const uint32_t* sa, const uint32_t* scan, uint32_t n, uint32_t* rank) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const uint32_t head = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
    rank[sa[j]] = scan[j] + head - 1u;
}

// key[i] = (rank[i], rank[i + h] + 1 or 0 past the end); val[i] = i
__global__ __launch_bounds__(kThreads) void sa_pair_key_kernel(const uint32_t* rank, uint32_t n, uint32_t h, uint64_t* key, uint32_t* val) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t second = i + h < n ? rank[i + h] + 1u : 0u;
    key[i] = (uint64_t)rank[i] << 32 | second;
    val[i] = i;
}

// ------------------------------------------------------------------------------------------------------------ search
// Eight bytes from any offset of a buffer that is 8-byte aligned and readable 16 bytes past the last byte used.
__device__ inline uint64_t load8(const uint8_t* base, uint64_t off) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(base) + (off >> 3);
    const uint32_t s = (uint32_t)(off & 7u) * 8u;
    const uint64_t lo = w[0];
    return s ? (lo >> s) | (w[1] << (64u - s)) : lo;
}

// sign of (suffix t[pos ..) cut to m bytes) - p[0 .. m), bytes as signed char; a suffix shorter than m that agrees is smaller
__device__ inline int cmp_suffix(const uint8_t* t, uint32_t n, uint32_t pos, const uint8_t* pb, uint64_t po, uint32_t m) {
    const uint32_t left = n - pos, len = left < m ? left : m;
    for (uint32_t o = 0; o < len; o += 8) {
        const uint64_t a = load8(t, (uint64_t)pos + o), b = load8(pb, po + o);
        const uint32_t rem = len - o;
        const uint64_t mask = rem >= 8 ? ~0ull : ((1ull << (8 * rem)) - 1ull);
        const uint64_t x = (a ^ b) & mask;
        if (x) {
            const uint32_t sh = (uint32_t)__builtin_ctzll(x) & ~7u;
            return (int8_t)(uint8_t)(a >> sh) < (int8_t)(uint8_t)(b >> sh) ? -1 : 1;
        }
    }
    return left < m ? -1 : 0;
}

// Per pattern: the SA range [lo, lo + cnt) of the suffixes that start with it
__global__ __launch_bounds__(kThreads) void sa_search_kernel(const uint8_t* t, uint32_t n, const uint32_t* sa, const uint8_t* pb,
                                                             const uint64_t* poff, uint32_t n_pat, uint32_t* lo_out, uint32_t* cnt_out) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_pat) return;
    const uint64_t po = poff[p];
    const uint64_t ml = poff[p + 1] - po;
    const uint32_t m = ml > n ? n + 1 : (uint32_t)ml;   // longer than the text: found nowhere, and the compare stops at n anyway
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (cmp_suffix(t, n, sa[mid], pb, po, m) < 0) a = mid + 1;
        else b = mid;
    }
    const uint32_t lo = a;
    b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (cmp_suffix(t, n, sa[mid], pb, po, m) <= 0) a = mid + 1;
        else b = mid;
    }
    lo_out[p] = lo;
    cnt_out[p] = a - lo;
}

// One thread per hit of a chunk of patterns: pattern by binary search over the chunk's offsets, text position from the SA,
// reference by binary search over ref_start (n_ref + 1 entries, reference r = [ref_start[r], ref_start[r + 1]), its last byte
// the terminator).  key = header_rank << 32 | local position, or ~0 on a terminator (dropped later: it sorts last).
__global__ __launch_bounds__(kThreads) void occ_gather_kernel(const uint32_t* sa, const uint32_t* lo, const uint32_t* off, uint32_t np,
                                                              uint32_t total, const uint32_t* ref_start, uint32_t n_ref,
                                                              const uint32_t* header_rank, uint64_t* key, uint32_t* pid) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= total) return;
    uint32_t a = 0, b = np;   // largest p with off[p] <= k
    while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if (off[mid] <= k) a = mid;
        else b = mid;
    }
    const uint32_t pos = sa[lo[a] + (k - off[a])];
    uint32_t r0 = 0, r1 = n_ref;   // largest r with ref_start[r] <= pos
    while (r1 - r0 > 1) {
        const uint32_t mid = r0 + (r1 - r0) / 2;
        if (ref_start[mid] <= pos) r0 = mid;
        else r1 = mid;
    }
    key[k] = pos + 1u == ref_start[r0 + 1] ? ~0ull : ((uint64_t)header_rank[r0] << 32 | (pos - ref_start[r0]));
    pid[k] = a;
}

}  // namespace sufarr
}  // namespace pwa
