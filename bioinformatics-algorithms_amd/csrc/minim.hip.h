// minim.hip.h -- (w, k)-minimizer sketches of a sequence list, and the lookup of read minimizers in a sorted minimizer index
// (DESIGN.md §3.27, and §3.28 for the canonical form; the definitions are in include/pwalign.h, "Minimizer sketches, a minimizer index,
// seeding against it" and "Canonical minimizers: one sketch, both strands").  Like
// seed.hip.h these are plain data-parallel passes of the suffix-array unit: the flattened slot order, owner_of and load8 are its own,
// and so are the scan, the sort and the split that the host code runs around them.
//
// A range of consecutive sequences is on the device as seed.hip.h has it: the blob (8-byte aligned, zero-padded 16 bytes past its end),
// seq_off[n_seqs + 1] (byte offsets), slot_off[n_seqs + 1]; slot s of sequence r is the k-mer that starts at p = s - slot_off[r], and
// sequence r has K = slot_off[r + 1] - slot_off[r] = max(len - k + 1, 0) of them.
#pragma once
#include "seed.hip.h"

namespace pwa {
namespace minim {

using sufarr::kThreads;
using sufarr::load8;
using sufarr::owner_of;

constexpr uint32_t kMaxK = 31, kMaxW = 128;
constexpr int kStage = kThreads + 2 * ((int)kMaxW - 1);   // a tile's hashes and a halo of w - 1 on either side: 4080 bytes of LDS
constexpr uint64_t kInvalid = ~0ull;                      // a k-mer over a byte that is not ACGT: above every hash (those are below 2^62)

// The invertible integer mix under a mask of 2 k bits: a bijection of the k-mer values, so equal hashes are equal k-mers
__host__ __device__ inline uint64_t mix(uint64_t key, uint64_t mask) {
    key = (~key + (key << 21)) & mask;
    key ^= key >> 24;
    key = (key + (key << 3) + (key << 8)) & mask;
    key ^= key >> 14;
    key = (key + (key << 2) + (key << 4)) & mask;
    key ^= key >> 28;
    key = (key + (key << 31)) & mask;
    return key;
}

// The hash of blob[po .. po + k), first symbol most significant, or kInvalid.  k = 31 takes four load8, five words at a bad offset.
__device__ inline uint64_t kmer_hash(const uint8_t* blob, uint64_t po, uint32_t k, uint64_t mask) {
    uint64_t v = 0;
    uint32_t seen = 0;
    for (uint32_t o = 0; o < k; o += 8) {
        uint64_t word = load8(blob, po + o);
        const uint32_t m = k - o < 8 ? k - o : 8;
        for (uint32_t j = 0; j < m; ++j, word >>= 8) {
            const uint32_t b = (uint32_t)word & 0xffu;
            const uint32_t c = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
            seen |= c;
            v = v << 2 | (c & 3u);
        }
    }
    return (seen & 4u) ? kInvalid : mix(v, mask);
}

// The canonical form: f = the k-mer's value, r = its reverse complement's, both out of the same load8 loop -- every
// symbol enters f at the bottom and, complemented, r at the top.  The smaller of the two is hashed and strand = 1 where that is r;
// f == r (a reverse palindrome, even k only) is kInvalid like a k-mer over N.
__device__ inline uint64_t kmer_hash_canonical(const uint8_t* blob, uint64_t po, uint32_t k, uint64_t mask, uint32_t& strand) {
    uint64_t f = 0, r = 0;
    uint32_t seen = 0;
    const uint32_t top = 2 * (k - 1);
    for (uint32_t o = 0; o < k; o += 8) {
        uint64_t word = load8(blob, po + o);
        const uint32_t m = k - o < 8 ? k - o : 8;
        for (uint32_t j = 0; j < m; ++j, word >>= 8) {
            const uint32_t b = (uint32_t)word & 0xffu;
            const uint32_t c = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
            seen |= c;
            f = f << 2 | (c & 3u);
            r = r >> 2 | (uint64_t)(3u - (c & 3u)) << top;
        }
    }
    strand = r < f ? 1u : 0u;
    return ((seen & 4u) || f == r) ? kInvalid : mix(r < f ? r : f, mask);
}

constexpr uint32_t kStrandBit = 0x80000000u;   // of a canonical sketch's position word on the device (positions are below 2^31)

struct SketchArgs {
    const uint8_t* blob;
    const uint64_t* seq_off;
    const uint32_t* slot_off;
    uint32_t n_seqs, n_slots, k, w;
};

// One lane per slot, 256 slots per workgroup.  The workgroup stages the hashes of slots [t0 - (w - 1), t0 + 256 + (w - 1)) in LDS (each
// lane its own and at most one of the halo), then every lane counts, among the neighbours OF ITS OWN SEQUENCE, a = the run of larger
// hashes right before it and b = the run of hashes not smaller right after it, each cut at w - 1 and at the sequence's ends -- which
// is what keeps a neighbouring sequence's k-mers out, so LDS needs no owner beside a hash.  The start is selected iff it is valid and
// a + b >= min(w, K) - 1: some window holds it with only larger hashes before and no smaller one after (the leftmost minimum).
// COUNT form: tile_cnt[tile] = the tile's selected starts.  WRITE form: tile_cnt holds their exclusive scan; the in-tile rank is
// the wave's ballot below the lane plus the counts of the waves before, so the output is in slot order without an atomic.
// CANON: the hashes are canonical ones; LDS still holds hashes only, a lane keeps the strand bit of its own k-mer in a register and
// a selected one writes it as bit 31 of its position word.
template <bool WRITE, bool CANON = false>
__global__ __launch_bounds__(kThreads) void sketch_kernel(const SketchArgs a, uint32_t* tile_cnt, uint64_t* hash_out, uint32_t* pos_out,
                                                          uint32_t* flat_out, uint32_t cap, uint32_t* fault) {
    __shared__ uint64_t sh[kStage];
    __shared__ uint32_t wave_cnt[kThreads / 64];
    const uint32_t tid = threadIdx.x, halo = a.w - 1;
    const uint64_t mask = (1ull << (2 * a.k)) - 1ull;
    const uint64_t t0 = (uint64_t)blockIdx.x * kThreads;   // staged index i holds slot t0 - halo + i
    const uint64_t s = t0 + tid;
    const bool live = s < a.n_slots;
    uint32_t p = 0, K = 0, strand = 0;
    if (live) {
        const uint32_t r = owner_of(a.slot_off, a.n_seqs, (uint32_t)s);
        p = (uint32_t)s - a.slot_off[r];
        K = a.slot_off[r + 1] - a.slot_off[r];
        sh[halo + tid] = CANON ? kmer_hash_canonical(a.blob, a.seq_off[r] + p, a.k, mask, strand) : kmer_hash(a.blob, a.seq_off[r] + p, a.k, mask);
    }
    if (tid < 2 * halo) {
        const uint32_t i = tid < halo ? tid : kThreads + tid;
        const uint64_t at = t0 + i;   // the slot + halo
        if (at >= halo && at - halo < a.n_slots) {
            const uint32_t x = (uint32_t)(at - halo), r = owner_of(a.slot_off, a.n_seqs, x);
            uint32_t other;
            sh[i] = CANON ? kmer_hash_canonical(a.blob, a.seq_off[r] + (x - a.slot_off[r]), a.k, mask, other)
                          : kmer_hash(a.blob, a.seq_off[r] + (x - a.slot_off[r]), a.k, mask);
        }
    }
    __syncthreads();
    bool sel = false;
    uint64_t h = kInvalid;
    if (live) {
        const uint32_t c = halo + tid;
        h = sh[c];
        if (h != kInvalid) {
            const uint32_t need = (a.w < K ? a.w : K) - 1u;
            const uint32_t la = p < halo ? p : halo, rb = K - 1u - p < halo ? K - 1u - p : halo;
            uint32_t na = 0, nb = 0;
            while (na < la && sh[c - 1u - na] > h) ++na;
            if (na + rb >= need)
                while (nb < rb && na + nb < need && sh[c + 1u + nb] >= h) ++nb;
            sel = na + nb >= need;
        }
    }
    const uint64_t vote = __ballot(sel);
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(vote);
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) tile_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        return;
    }
    if (!sel) return;
    uint32_t rank = tile_cnt[blockIdx.x] + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
    for (uint32_t q = 0; q < wv; ++q) rank += wave_cnt[q];
    if (rank >= cap) {   // (the count pass and this one disagree: internal error)
        *fault = 1u;
        return;
    }
    hash_out[rank] = h;
    pos_out[rank] = CANON ? p | (strand ? kStrandBit : 0u) : p;
    if (flat_out) flat_out[rank] = (uint32_t)s;
}

// min_off[r] = how many of the `total` selected slots (flat: ascending) lie before sequence r's first slot, r = 0 .. n_seqs
__global__ __launch_bounds__(kThreads) void sketch_offsets_kernel(const uint32_t* flat, uint32_t total, const uint32_t* slot_off, uint32_t n_seqs,
                                                                  uint32_t* min_off) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r > n_seqs) return;
    const uint32_t x = slot_off[r];
    uint32_t lo = 0, hi = total;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (flat[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    min_off[r] = lo;
}

// One lane per read minimizer: lo_out = the first index entry with its hash, cnt_out = how many have it, or 0 where more than max_occ
// do -- seed_search_kernel's bounds and probe over plain uint64 compares of the sorted hashes; no text is loaded.
__global__ __launch_bounds__(kThreads) void lookup_kernel(const uint64_t* ix_hash, uint32_t n_min, const uint64_t* q_hash, uint32_t n_q,
                                                          uint32_t max_occ, uint32_t* lo_out, uint32_t* cnt_out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_q) return;
    const uint64_t h = q_hash[i];
    uint32_t a = 0, b = n_min;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (ix_hash[mid] < h) a = mid + 1;
        else b = mid;
    }
    const uint32_t lo = a;
    const uint64_t probe = (uint64_t)lo + max_occ;
    uint32_t cnt = 0;
    if (probe >= n_min || ix_hash[probe] != h) {
        b = probe < n_min ? (uint32_t)probe : n_min;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (ix_hash[mid] <= h) a = mid + 1;
            else b = mid;
        }
        cnt = a - lo;
    }
    lo_out[i] = lo;
    cnt_out[i] = cnt;
}

// One lane per hit, in minimizer order (ascending q within a read): seed_gather_kernel with t from the index's positions and q the
// minimizer's own.  key = local read << 32 | t, val = q.
__global__ __launch_bounds__(kThreads) void gather_kernel(const uint32_t* ix_pos, uint32_t n_min, const uint32_t* lo, const uint32_t* hit_off,
                                                          uint32_t n_q, uint32_t total, const uint32_t* min_off, uint32_t n_reads,
                                                          const uint32_t* q_pos, uint64_t* key, uint32_t* val, uint32_t* fault) {
    const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
    if (h >= total) return;
    const uint32_t m = owner_of(hit_off, n_q, h);
    const uint32_t r = owner_of(min_off, n_reads, m);
    const uint64_t at = (uint64_t)lo[m] + (h - hit_off[m]);
    uint32_t t = 0;
    if (at < n_min) t = ix_pos[at];
    else *fault = 1u;   // (a range past the index: internal error)
    key[h] = (uint64_t)r << 32 | t;
    val[h] = q_pos[m];
}

// The gather of a canonical seeding, one lane per hit: t and s_t from the index's position word, q and s_q from the
// read sketch's, L from seq_off.  key = (2 local read + (s_q ^ s_t)) << 32 | t; val = q in a forward list (s_q == s_t) and the mirrored
// start L - k - q in a reverse one, which descends where q ascends: split_strands_kernel turns those runs round after the sort.
__global__ __launch_bounds__(kThreads) void gather_strands_kernel(const uint32_t* ix_pos, uint32_t n_min, const uint32_t* lo, const uint32_t* hit_off,
                                                                  uint32_t n_q, uint32_t total, const uint32_t* min_off, uint32_t n_reads,
                                                                  const uint32_t* q_pos, const uint64_t* seq_off, uint32_t k, uint64_t* key,
                                                                  uint32_t* val, uint32_t* fault) {
    const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
    if (h >= total) return;
    const uint32_t m = owner_of(hit_off, n_q, h);
    const uint32_t r = owner_of(min_off, n_reads, m);
    const uint64_t at = (uint64_t)lo[m] + (h - hit_off[m]);
    uint32_t tw = 0;
    if (at < n_min) tw = ix_pos[at];
    else *fault = 1u;   // (a range past the index: internal error)
    const uint32_t qw = q_pos[m], q = qw & ~kStrandBit, flip = (qw ^ tw) >> 31;
    const uint64_t len = seq_off[r + 1] - seq_off[r];
    uint32_t v = q;
    if (flip) {
        if ((uint64_t)q + k <= len) v = (uint32_t)(len - k - q);
        else *fault = 1u;   // (a minimizer past its read's end: internal error)
    }
    key[h] = (uint64_t)(2u * r + flip) << 32 | (tw & ~kStrandBit);
    val[h] = v;
}

// list_off[i] = how many of the `total` sorted keys belong to a list below i, i = 0 .. n_lists: a hit's list is known only once it is
// gathered, so the cuts come from the sorted keys, one lower bound per boundary as in sketch_offsets_kernel.
__global__ __launch_bounds__(kThreads) void list_offsets_kernel(const uint64_t* key, uint32_t total, uint32_t n_lists, uint32_t* list_off) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i > n_lists) return;
    const uint64_t x = (uint64_t)i << 32;
    uint32_t lo = 0, hi = total;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    list_off[i] = lo;
}

// The first (DIR = -1) or last (+1) index of the run of keys equal to key[h] = kk in the sorted key[0 .. total): doubling steps away
// from h, then a binary search in the last step -- two loads where the run is h alone, log of the run otherwise.
template <int DIR>
__device__ inline uint32_t run_edge(const uint64_t* key, uint32_t total, uint32_t h, uint64_t kk) {
    uint32_t in = h, out, step = 1;   // key[in] == kk; out: one past the edge at the earliest
    for (;;) {
        const uint32_t room = DIR < 0 ? in : total - 1u - in;
        if (room < step) {
            out = DIR < 0 ? 0u : total - 1u;
            break;
        }
        const uint32_t at = DIR < 0 ? in - step : in + step;
        if (key[at] != kk) {
            out = DIR < 0 ? at + 1u : at - 1u;
            break;
        }
        in = at;
        step <<= 1;
    }
    uint32_t lo = DIR < 0 ? out : in, hi = DIR < 0 ? in : out;   // the edge lies in [lo, hi]
    while (lo < hi) {
        if (DIR < 0) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (key[mid] == kk) hi = mid;
            else lo = mid + 1u;
        } else {
            const uint32_t mid = lo + (hi - lo + 1u) / 2;
            if (key[mid] == kk) lo = mid;
            else hi = mid - 1u;
        }
    }
    return lo;
}

// seed_split_kernel for the two lists per read, one lane per sorted hit: t_out = the key's low word, and the values move to val_out --
// in place in a forward (even) list; in a reverse (odd) list the hits of one (list, t) arrived in ascending q, that is in descending
// mirrored start, so hit h of the run [a, b] goes to a + b - h and every list leaves in ascending (t, q').
__global__ __launch_bounds__(kThreads) void split_strands_kernel(const uint64_t* key, const uint32_t* val, uint32_t total, uint32_t* t_out,
                                                                 uint32_t* val_out) {
    const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
    if (h >= total) return;
    const uint64_t kk = key[h];
    t_out[h] = (uint32_t)kk;
    uint32_t dst = h;
    if ((kk >> 32) & 1u) dst = run_edge<-1>(key, total, h, kk) + (run_edge<1>(key, total, h, kk) - h);
    val_out[dst] = val[h];
}

}  // namespace minim
}  // namespace pwa
