// seed.hip.h -- seeding a list of reads against the suffix-array index: the k-mers are cut out of the read blob by the
// search kernel, every k-mer is searched once, the hits are gathered in slot order and put into (read, t, q) order by one stable radix
// sort.  The compare and the 8-byte loads are sufarr.hip.h's; like every kernel there, these are plain data-parallel passes.
//
// A range of consecutive reads is on the device as: the read blob (8-byte aligned, zero-padded 16 bytes past its end, as load8 requires),
// read_off[n_reads + 1] (byte offsets into the blob), slot_off[n_reads + 1] (read r's slots are slot_off[r] .. slot_off[r + 1]), and slot s
// of read r is the k-mer at q = (s - slot_off[r]) * step.
#pragma once
#include "sufarr.hip.h"

namespace pwa {
namespace sufarr {

// The largest i in [0, n) with off[i] <= x, for a non-decreasing off with off[0] <= x.  Among equal entries that is the last one: the
// read (slot) that owns slot (hit) x when the reads (slots) before it are empty.
__device__ inline uint32_t owner_of(const uint32_t* off, uint32_t n, uint32_t x) {
    uint32_t a = 0, b = n;
    while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if (off[mid] <= x) a = mid;
        else b = mid;
    }
    return a;
}

// One lane per slot; consecutive lanes take consecutive slots of a read, so their 8-byte loads from the blob share cache lines.
// lo_out[s] = the first suffix that starts with the k-mer, cnt_out[s] = how many do, or 0 where more than max_occ do.  k <= n.
// The lower bound is sa_search_kernel's.  The upper bound: if sa[lo + max_occ] exists and still starts with the k-mer, the slot is
// dropped; otherwise every suffix from min(lo + max_occ, n) on is larger, and the bound lies in [lo, that] -- log2(max_occ) + 1 steps.
__global__ __launch_bounds__(kThreads) void seed_search_kernel(const uint8_t* t, uint32_t n, const uint32_t* sa, const uint8_t* blob,
                                                               const uint64_t* read_off, const uint32_t* slot_off, uint32_t n_reads,
                                                               uint32_t n_slots, uint32_t k, uint32_t step, uint32_t max_occ, uint32_t* lo_out,
                                                               uint32_t* cnt_out) {
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= n_slots) return;
    const uint32_t r = owner_of(slot_off, n_reads, s);
    const uint64_t po = read_off[r] + (uint64_t)(s - slot_off[r]) * step;
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (cmp_suffix(t, n, sa[mid], blob, po, k) < 0) a = mid + 1;
        else b = mid;
    }
    const uint32_t lo = a;
    const uint64_t probe = (uint64_t)lo + max_occ;
    uint32_t cnt = 0;
    if (probe >= n || cmp_suffix(t, n, sa[probe], blob, po, k) != 0) {
        b = probe < n ? (uint32_t)probe : n;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (cmp_suffix(t, n, sa[mid], blob, po, k) <= 0) a = mid + 1;
            else b = mid;
        }
        cnt = a - lo;
    }
    lo_out[s] = lo;
    cnt_out[s] = cnt;
}

// anc_off[r] = hit_off[slot_off[r]] for r = 0 .. n_reads: where read r's anchors start among the range's (hit_off: the scanned counts,
// n_slots + 1 entries, the total last)
__global__ __launch_bounds__(kThreads) void seed_read_offsets_kernel(const uint32_t* hit_off, const uint32_t* slot_off, uint32_t n_reads,
                                                                     uint32_t* anc_off) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r <= n_reads) anc_off[r] = hit_off[slot_off[r]];
}

// One lane per hit, in slot order (ascending q within a read): key = local read << 32 | t, val = q.  A stable sort by key then leaves
// the hits in (read, t, q) order.
__global__ __launch_bounds__(kThreads) void seed_gather_kernel(const uint32_t* sa, const uint32_t* lo, const uint32_t* hit_off, uint32_t n_slots,
                                                               uint32_t total, const uint32_t* slot_off, uint32_t n_reads, uint32_t step,
                                                               uint64_t* key, uint32_t* val) {
    const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
    if (h >= total) return;
    const uint32_t s = owner_of(hit_off, n_slots, h);
    const uint32_t r = owner_of(slot_off, n_reads, s);
    key[h] = (uint64_t)r << 32 | sa[lo[s] + (h - hit_off[s])];
    val[h] = (s - slot_off[r]) * step;
}

// t_out[h] = the text position of sorted key h
__global__ __launch_bounds__(kThreads) void seed_split_kernel(const uint64_t* key, uint32_t total, uint32_t* t_out) {
    const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
    if (h < total) t_out[h] = (uint32_t)key[h];
}

}  // namespace sufarr
}  // namespace pwa
