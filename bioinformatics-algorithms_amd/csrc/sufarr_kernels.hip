// sufarr_kernels.hip -- the suffix-array entries of include/pwalign.h (pwa_sa_*, pwa_seed_plan): device buffers, the prefix-doubling
// rounds, the radix-sort passes, the chunked occurrence lists, and the seeding of read lists against a kept index; and the minimizer
// entries (pwa_mm_*), which share the seeding's planner, scan, sort and split.  Kernels: sufarr.hip.h, seed.hip.h, minim.hip.h.
// DESIGN.md §3.8, §3.25, §3.27, §3.28.
#include "../../include/pwalign.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "minim.hip.h"
#include "seed.hip.h"
#include "sufarr.hip.h"
#include "sufarr_ctx.h"

using namespace pwa::sufarr;
using pwa::blocks_for;
using pwa::Dev;
using pwa::Fail;

struct pwa_sa_index {
    pwa_ctx* ctx = nullptr;
    uint32_t n = 0;
    Dev d_text;   // round_up(n, 8) + 16 bytes, zero past n (sufarr::load8)
    Dev d_sa;     // n positions (one where n == 0)
    uint32_t rounds = 0;
    float build_ms = 0.f, search_ms = 0.f;
    // the last pwa_sa_seed: its anchors (all reads, in the call's order) until the next one, and its stats
    bool seeded = false;
    std::vector<uint32_t> anc_t, anc_q;
    float seed_search_ms = 0.f, seed_sort_ms = 0.f;
    uint64_t seed_slots = 0, seed_hits = 0, seed_ranges = 0;
};

struct pwa_mm_index {
    pwa_ctx* ctx = nullptr;
    uint32_t k = 0, w = 0, n_min = 0;
    bool canonical = false;   // canonical hashes, and the strand of every entry in bit 31 of its position word
    Dev d_hash, d_pos;   // 2 n_min entries each, as sort_pairs takes them; half `half` holds the pairs in (hash, t) order
    int half = 0;
    float build_ms = 0.f;
    // the last pwa_mm_seed: its anchors (all reads, in the call's order) until the next one, and its stats
    bool seeded = false;
    std::vector<uint32_t> anc_t, anc_q;
    float sketch_ms = 0.f, search_ms = 0.f, sort_ms = 0.f;
    uint64_t slots = 0, minimizers = 0, hits = 0, ranges = 0;

    const uint64_t* hashes() const { return d_hash.as<uint64_t>() + (size_t)half * n_min; }
    const uint32_t* positions() const { return d_pos.as<uint32_t>() + (size_t)half * n_min; }
};

constexpr uint64_t kDefaultChunkHits = 1ull << 27;   // 24 B of device buffers per raw hit: 3.2 GB per chunk at most

// x[0 .. len) := exclusive prefix sums, in place (reduce, scan of the chunk sums, apply); part: scan_part_words(len) words.
// Also the scan of pwa_align_batch_cigar's string lengths (pwalign_align.hip), hence outside this unit's anonymous namespace.
size_t pwa::scan_part_words(size_t len) { return len / kTile + 1; }
void pwa::scan_excl(hipStream_t s, uint32_t* x, size_t len, uint32_t* part) {
    if (!len) return;
    const uint32_t nb = blocks_for(len, kTile);
    scan_reduce_kernel<<<nb, kThreads, 0, s>>>(x, len, part);
    scan_partials_kernel<<<1, kThreads, 0, s>>>(part, nb);
    scan_apply_kernel<<<nb, kThreads, 0, s>>>(x, len, part);
}

void pwa::SortScratch::alloc(pwa::Poison* po, size_t n) {
    const size_t tiles = std::max<size_t>(1, (n + kTile - 1) / kTile);
    UNIT_CHECK(hist.alloc(po, tiles * kBuckets * 4));
    UNIT_CHECK(part.alloc(po, ((std::max(tiles * kBuckets, n + 1) + kTile - 1) / kTile + 1) * 4));
    UNIT_CHECK(bits.alloc(po, (2 * 1024 + 2) * 8));
}

namespace {

// Buffers of a stable LSD radix sort of n (key, value) pairs: k[cur] / v[cur] hold the input and, afterwards, the result.
template <class K, class V>
struct SortBufs {
    K* k[2];
    V* v[2];
    int cur = 0;
};

// Scratch of radix_sort for up to n elements (sufarr_ctx.h)
using pwa::SortScratch;

// Stable sort by key.  Digits (8 bits) that are the same in every key are skipped: one OR / AND reduction and a 16-byte
// read-back decide which passes run.  Returns the number of passes.
template <class K, class V>
int radix_sort(hipStream_t s, SortBufs<K, V>& b, size_t n, SortScratch& sc) {
    if (n <= 1) return 0;
    const uint32_t tiles = blocks_for(n, kTile), g = std::min<uint32_t>(tiles, 1024);
    K* bits = sc.bits.as<K>();
    key_bits_kernel<K><<<g, kThreads, 0, s>>>(b.k[b.cur], b.k[b.cur], n, bits, bits + g);
    key_bits_kernel<K><<<1, kThreads, 0, s>>>(bits, bits + g, g, bits + 2 * g, bits + 2 * g + 1);
    K h[2];
    UNIT_CHECK(hipMemcpyAsync(h, bits + 2 * g, sizeof h, hipMemcpyDeviceToHost, s));
    UNIT_CHECK(hipStreamSynchronize(s));
    const K vary = h[0] ^ h[1];
    int passes = 0;
    for (int sh = 0; sh < (int)(8 * sizeof(K)); sh += kRadixBits) {
        if (((vary >> sh) & (K)(kBuckets - 1)) == 0) continue;
        uint32_t* hist = sc.hist.as<uint32_t>();
        radix_hist_kernel<K><<<tiles, kThreads, 0, s>>>(b.k[b.cur], n, sh, hist, tiles);
        pwa::scan_excl(s, hist, (size_t)tiles * kBuckets, sc.part.as<uint32_t>());
        radix_scatter_kernel<K, V><<<tiles, kThreads, 0, s>>>(b.k[b.cur], b.v[b.cur], b.k[b.cur ^ 1], b.v[b.cur ^ 1], n, sh, hist, tiles);
        b.cur ^= 1;
        ++passes;
    }
    UNIT_CHECK(hipGetLastError());
    return passes;
}

// Patterns on the device (blob padded for sufarr::load8, offsets rebased to 0) and their SA ranges.
struct Ranges {
    Dev blob, off, lo, cnt;
    std::vector<uint32_t> h_cnt;
};

void search(pwa::SaCtxView& v, const pwa_sa_index* ix, const uint8_t* pb, const uint64_t* poff, uint32_t n_pat, Ranges& r) {
    const uint64_t base = poff[0], bytes = poff[n_pat] - base;
    std::vector<uint64_t> off(poff, poff + n_pat + 1);
    for (auto& o : off) o -= base;
    UNIT_CHECK(r.blob.alloc(v.poison, (bytes + 7) / 8 * 8 + 16));
    UNIT_CHECK(r.off.alloc(v.poison, off.size() * 8));
    UNIT_CHECK(r.lo.alloc(v.poison, (size_t)n_pat * 4));
    UNIT_CHECK(r.cnt.alloc(v.poison, (size_t)n_pat * 4 + 4));
    UNIT_CHECK(hipMemsetAsync(r.blob.p, 0, (bytes + 7) / 8 * 8 + 16, v.stream));
    UNIT_CHECK(hipMemcpyAsync(r.blob.p, pb + base, bytes, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(r.off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, v.stream));
    if (n_pat) sa_search_kernel<<<blocks_for(n_pat, kThreads), kThreads, 0, v.stream>>>(ix->d_text.as<uint8_t>(), ix->n, ix->d_sa.as<uint32_t>(), r.blob.as<uint8_t>(),
                                                                                        r.off.as<uint64_t>(), n_pat, r.lo.as<uint32_t>(), r.cnt.as<uint32_t>());
    UNIT_CHECK(hipGetLastError());
    r.h_cnt.resize(n_pat);
    UNIT_CHECK(hipMemcpyAsync(r.h_cnt.data(), r.cnt.p, (size_t)n_pat * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
}

bool patterns_ok(const uint8_t* pb, const uint64_t* poff, uint32_t n_pat) {
    if (!poff || (!pb && poff[n_pat] != poff[0])) return false;
    for (uint32_t k = 0; k < n_pat; ++k)
        if (poff[k + 1] < poff[k]) return false;
    return true;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- seeding: validation and the host-only planner, then the stages of one range

constexpr uint32_t kNoRead = 0xFFFFFFFFu;

struct SeedCall {
    uint64_t n = 0;                  // text bytes
    const uint64_t* off = nullptr;   // n_reads + 1 byte offsets of the reads
    uint32_t n_reads = 0, k = 0, step = 0, max_occ = 0;

    uint64_t slots(uint64_t r) const {
        const uint64_t len = off[r + 1] - off[r];
        return len < k ? 0 : (len - k) / step + 1;
    }
    uint64_t hits_per_slot() const { return n < k ? 0 : std::min<uint64_t>(max_occ, n - k + 1); }
    uint64_t worst_hits(uint64_t r) const { return slots(r) * hits_per_slot(); }   // both factors below 2^32
};

// Pointers and parameters, then the reads in order, then the list's slots: the code, the first offending read in `bad`, the slots
int seed_validate(const SeedCall& c, uint32_t& bad, uint64_t& n_slots, std::string& what) {
    bad = kNoRead;
    n_slots = 0;
    if (c.n_reads && !c.off) {
        what = "a required pointer is null";
        return PWA_E_INVALID;
    }
    if (!c.k || !c.step || !c.max_occ) {
        what = "k, step and max_occ are at least 1";
        return PWA_E_INVALID;
    }
    uint64_t total = 0;
    for (uint32_t r = 0; r < c.n_reads; ++r) {
        const auto fail = [&](int code, const char* why) {
            bad = r;
            what = "read " + std::to_string(r) + ": " + why;
            return code;
        };
        if (c.off[r + 1] < c.off[r]) return fail(PWA_E_INVALID, "read_off decreases");
        if (c.off[r + 1] - c.off[r] >= (1ull << 31)) return fail(PWA_E_CAPACITY, "2^31 bytes or more");
        if (c.worst_hits(r) >= (1ull << 32)) return fail(PWA_E_CAPACITY, "its slots times min(max_occ, n - k + 1) reach 2^32");
        total += c.slots(r);   // below 2^31 each, 2^32 of them at most: no overflow
    }
    if (total >= (1ull << 32)) {
        what = std::to_string(total) + " slots; at most 2^32 - 1";
        return PWA_E_CAPACITY;
    }
    n_slots = total;
    return PWA_OK;
}

// Consecutive reads whose worst-case hits fit the budget (or one read that alone exceeds it); a range without a slot is left out.
// Every range's slots and hits fit uint32: a read's worst case is below 2^32, and so is the budget.
std::vector<pwa::Run> seed_ranges(const SeedCall& c, uint64_t budget) {
    budget = std::min<uint64_t>(budget ? budget : kDefaultChunkHits, 0xFFFFFFFFull);
    std::vector<pwa::Run> out;
    if (!c.hits_per_slot()) return out;   // n < k: no k-mer of any read occurs
    for (const pwa::Run& g : pwa::cut_runs(c.n_reads, budget, [&](uint64_t r) { return c.worst_hits(r); }))
        if (g.weight) out.push_back(g);
    return out;
}

// Grow-only: the buffer handed out again (and poisoned again) where it is large enough
void fit(pwa::Poison* po, Dev& d, size_t bytes) {
    if (d.p && d.cap >= bytes) UNIT_CHECK(d.again(po));
    else UNIT_CHECK(d.alloc(po, bytes));
}

struct SeedBuffers {
    Dev blob, read_off, slot_off, lo, cnt, slot_part, anc_off;   // by the range's bytes, reads and slots
    Dev key, val;                                                // by the range's hits, as the scan reports them
    SortScratch sc;
    size_t sc_n = 0;
    std::vector<uint64_t> h_read_off;
    std::vector<uint32_t> h_slot_off, h_anc_off;

    void fit_sort(pwa::Poison* po, size_t n) {
        if (n > sc_n) {
            sc.alloc(po, n);
            sc_n = n;
        } else {
            for (Dev* d : {&sc.hist, &sc.part, &sc.bits}) UNIT_CHECK(d->again(po));
        }
    }
};

// One range: reads g.k0 .. g.k1 searched, their hits sorted and appended to the index's kept anchors, their offsets into anc_off_out
void seed_range(pwa::SaCtxView& v, pwa_sa_index* ix, const SeedCall& c, const uint8_t* bytes, const pwa::Run& g, SeedBuffers& b, pwa::Events<4>& ev,
                uint64_t* anc_off_out) {
    const uint32_t nr = (uint32_t)(g.k1 - g.k0);
    const uint64_t base = c.off[g.k0], n_bytes = c.off[g.k1] - base;
    b.h_read_off.resize((size_t)nr + 1);
    b.h_slot_off.resize((size_t)nr + 1);
    uint64_t ns64 = 0;
    for (uint64_t i = 0; i <= nr; ++i) {
        b.h_read_off[i] = c.off[g.k0 + i] - base;
        b.h_slot_off[i] = (uint32_t)ns64;
        if (i < nr) ns64 += c.slots(g.k0 + i);
    }
    const uint32_t ns = (uint32_t)ns64;   // <= the range's worst-case hits
    const size_t blob_bytes = (n_bytes + 7) / 8 * 8 + 16;
    fit(v.poison, b.blob, blob_bytes);
    fit(v.poison, b.read_off, ((size_t)nr + 1) * 8);
    fit(v.poison, b.slot_off, ((size_t)nr + 1) * 4);
    fit(v.poison, b.anc_off, ((size_t)nr + 1) * 4);
    fit(v.poison, b.lo, (size_t)ns * 4);
    fit(v.poison, b.cnt, ((size_t)ns + 1) * 4);
    fit(v.poison, b.slot_part, pwa::scan_part_words((size_t)ns + 1) * 4);
    UNIT_CHECK(hipMemcpyAsync(b.blob.p, bytes + base, n_bytes, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemsetAsync(b.blob.as<uint8_t>() + n_bytes, 0, blob_bytes - n_bytes, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.read_off.p, b.h_read_off.data(), ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.slot_off.p, b.h_slot_off.data(), ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, v.stream));
    uint32_t* hit_off = b.cnt.as<uint32_t>();   // the counts, then, scanned, where each slot's hits start; the total last
    UNIT_CHECK(hipMemsetAsync(hit_off + ns, 0, 4, v.stream));
    UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
    seed_search_kernel<<<blocks_for(ns, kThreads), kThreads, 0, v.stream>>>(ix->d_text.as<uint8_t>(), ix->n, ix->d_sa.as<uint32_t>(), b.blob.as<uint8_t>(),
                                                                            b.read_off.as<uint64_t>(), b.slot_off.as<uint32_t>(), nr, ns, c.k, c.step,
                                                                            c.max_occ, b.lo.as<uint32_t>(), hit_off);
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
    pwa::scan_excl(v.stream, hit_off, (size_t)ns + 1, b.slot_part.as<uint32_t>());
    seed_read_offsets_kernel<<<blocks_for((size_t)nr + 1, kThreads), kThreads, 0, v.stream>>>(hit_off, b.slot_off.as<uint32_t>(), nr, b.anc_off.as<uint32_t>());
    UNIT_CHECK(hipGetLastError());
    b.h_anc_off.resize((size_t)nr + 1);
    UNIT_CHECK(hipMemcpyAsync(b.h_anc_off.data(), b.anc_off.p, ((size_t)nr + 1) * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    const uint32_t total = b.h_anc_off[nr];
    const size_t kept = ix->anc_t.size();
    for (uint32_t i = 0; i < nr; ++i) anc_off_out[g.k0 + i] = kept + b.h_anc_off[i];
    float ms = 0.f;
    UNIT_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ix->seed_search_ms += ms;
    ix->seed_hits += total;
    ix->seed_ranges += 1;
    if (!total) return;
    fit(v.poison, b.key, (size_t)total * 16);
    fit(v.poison, b.val, (size_t)total * 8);
    b.fit_sort(v.poison, total);
    SortBufs<uint64_t, uint32_t> s{{b.key.as<uint64_t>(), b.key.as<uint64_t>() + total}, {b.val.as<uint32_t>(), b.val.as<uint32_t>() + total}, 0};
    UNIT_CHECK(hipEventRecord(ev.e[2], v.stream));
    seed_gather_kernel<<<blocks_for(total, kThreads), kThreads, 0, v.stream>>>(ix->d_sa.as<uint32_t>(), b.lo.as<uint32_t>(), hit_off, ns, total,
                                                                               b.slot_off.as<uint32_t>(), nr, c.step, s.k[0], s.v[0]);
    UNIT_CHECK(hipGetLastError());
    radix_sort(v.stream, s, total, b.sc);
    uint32_t* d_t = reinterpret_cast<uint32_t*>(s.k[s.cur ^ 1]);   // the sort's other key buffer is free now
    seed_split_kernel<<<blocks_for(total, kThreads), kThreads, 0, v.stream>>>(s.k[s.cur], total, d_t);
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[3], v.stream));
    ix->anc_t.resize(kept + total);
    ix->anc_q.resize(kept + total);
    UNIT_CHECK(hipMemcpyAsync(ix->anc_t.data() + kept, d_t, (size_t)total * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipMemcpyAsync(ix->anc_q.data() + kept, s.v[s.cur], (size_t)total * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    UNIT_CHECK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
    ix->seed_sort_ms += ms;
}

// ---- minimizers: the sketch of a range of sequences in two passes, then the index build and the stages of one seeded range

namespace mm = pwa::minim;

bool mm_params_ok(uint32_t k, uint32_t w) { return k >= 1 && k <= mm::kMaxK && w >= 1 && w <= mm::kMaxW; }

uint64_t kmers_of(uint64_t len, uint32_t k) { return len < k ? 0 : len - k + 1; }

// The reads of a minimizer seeding as a SeedCall: step 1, and a text that has n_min k-mers (only min(max_occ, that) enters the plan)
SeedCall mm_call(uint64_t n_min, const uint64_t* off, uint32_t n_reads, uint32_t k, uint32_t max_occ) {
    return SeedCall{std::min<uint64_t>(n_min, 1ull << 32) + k - 1, off, n_reads, k, 1, max_occ};
}

// Pointers aside: k and w, then the sequences in order -- offsets decreasing, 2^31 bytes or more
int sketch_validate(const uint64_t* off, uint32_t n_seqs, uint32_t k, uint32_t w, std::string& what) {
    if (!mm_params_ok(k, w)) {
        what = "k is 1 .. 31 and w is 1 .. 128";
        return PWA_E_INVALID;
    }
    for (uint32_t r = 0; r < n_seqs; ++r) {
        if (off[r + 1] < off[r]) {
            what = "sequence " + std::to_string(r) + ": seq_off decreases";
            return PWA_E_INVALID;
        }
        if (off[r + 1] - off[r] >= (1ull << 31)) {
            what = "sequence " + std::to_string(r) + ": 2^31 bytes or more";
            return PWA_E_CAPACITY;
        }
    }
    return PWA_OK;
}

// A range of sequences on the device and its sketch: the per-tile counts (scanned in place, the total last), then the sketch itself
// in slot order -- hash, position in the sequence, flattened slot -- and where each sequence's minimizers start among them
struct SketchBuffers {
    Dev blob, seq_off, slot_off, tile, part, hash, pos, flat, min_off, fault;
    std::vector<uint64_t> h_seq_off;
    std::vector<uint32_t> h_slot_off, h_min_off;
    mm::SketchArgs args{};
    uint32_t n_tiles = 0, total = 0;
    bool canonical = false;   // the canonical kernels: pos then carries the strand in bit 31

    void start(pwa::SaCtxView& v, bool canon = false) {   // once per call: the fault word of all its launches
        canonical = canon;
        UNIT_CHECK(fault.alloc(v.poison, 4));
        UNIT_CHECK(hipMemsetAsync(fault.p, 0, 4, v.stream));
    }
    void check_fault(const char* who) {   // after a wait on the stream
        uint32_t f = 0;
        UNIT_CHECK(hipMemcpy(&f, fault.p, 4, hipMemcpyDeviceToHost));
        if (f) throw Fail{PWA_E_HIP, std::string(who) + ": a kernel left its bounds (internal error)"};
    }
};

// Sequences k0 .. k1 of the list uploaded, their slots laid out, and the count pass: b.total minimizers (waits for it).
// ev: two events around the device work, or null.
void sketch_count(pwa::SaCtxView& v, const uint8_t* bytes, const uint64_t* off, uint64_t k0, uint64_t k1, uint32_t k, uint32_t w, SketchBuffers& b,
                  hipEvent_t* ev) {
    const uint32_t nr = (uint32_t)(k1 - k0);
    const uint64_t base = off[k0], n_bytes = off[k1] - base;
    b.h_seq_off.resize((size_t)nr + 1);
    b.h_slot_off.resize((size_t)nr + 1);
    uint64_t ns64 = 0;
    for (uint64_t i = 0; i <= nr; ++i) {
        b.h_seq_off[i] = off[k0 + i] - base;
        b.h_slot_off[i] = (uint32_t)ns64;
        if (i < nr) ns64 += kmers_of(off[k0 + i + 1] - off[k0 + i], k);
    }
    const uint32_t ns = (uint32_t)ns64;   // the caller's ranges hold fewer than 2^32 slots
    b.n_tiles = blocks_for(ns, kThreads);
    const size_t blob_bytes = (n_bytes + 7) / 8 * 8 + 16;
    fit(v.poison, b.blob, blob_bytes);
    fit(v.poison, b.seq_off, ((size_t)nr + 1) * 8);
    fit(v.poison, b.slot_off, ((size_t)nr + 1) * 4);
    fit(v.poison, b.tile, ((size_t)b.n_tiles + 1) * 4);
    fit(v.poison, b.part, pwa::scan_part_words((size_t)b.n_tiles + 1) * 4);
    if (n_bytes) UNIT_CHECK(hipMemcpyAsync(b.blob.p, bytes + base, n_bytes, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemsetAsync(b.blob.as<uint8_t>() + n_bytes, 0, blob_bytes - n_bytes, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.seq_off.p, b.h_seq_off.data(), ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemcpyAsync(b.slot_off.p, b.h_slot_off.data(), ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, v.stream));
    UNIT_CHECK(hipMemsetAsync(b.tile.as<uint32_t>() + b.n_tiles, 0, 4, v.stream));
    b.args = mm::SketchArgs{b.blob.as<uint8_t>(), b.seq_off.as<uint64_t>(), b.slot_off.as<uint32_t>(), nr, ns, k, w};
    b.total = 0;
    if (ev) UNIT_CHECK(hipEventRecord(ev[0], v.stream));
    if (ns) {
        const auto count = b.canonical ? mm::sketch_kernel<false, true> : mm::sketch_kernel<false, false>;
        count<<<b.n_tiles, kThreads, 0, v.stream>>>(b.args, b.tile.as<uint32_t>(), nullptr, nullptr, nullptr, 0, b.fault.as<uint32_t>());
        UNIT_CHECK(hipGetLastError());
        pwa::scan_excl(v.stream, b.tile.as<uint32_t>(), (size_t)b.n_tiles + 1, b.part.as<uint32_t>());
    }
    if (ev) UNIT_CHECK(hipEventRecord(ev[1], v.stream));
    UNIT_CHECK(hipMemcpyAsync(&b.total, b.tile.as<uint32_t>() + b.n_tiles, 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
}

// The write pass of the range counted last, into hash_out / pos_out (b.total entries each); with offsets also b.flat and b.min_off.
// Enqueued only.
void sketch_write(pwa::SaCtxView& v, SketchBuffers& b, uint64_t* hash_out, uint32_t* pos_out, bool offsets) {
    if (offsets) {
        fit(v.poison, b.flat, (size_t)b.total * 4);
        fit(v.poison, b.min_off, ((size_t)b.args.n_seqs + 1) * 4);
    }
    if (b.total) {
        const auto write = b.canonical ? mm::sketch_kernel<true, true> : mm::sketch_kernel<true, false>;
        write<<<b.n_tiles, kThreads, 0, v.stream>>>(b.args, b.tile.as<uint32_t>(), hash_out, pos_out, offsets ? b.flat.as<uint32_t>() : nullptr, b.total,
                                                    b.fault.as<uint32_t>());
        UNIT_CHECK(hipGetLastError());
    }
    if (offsets) {
        mm::sketch_offsets_kernel<<<blocks_for((size_t)b.args.n_seqs + 1, kThreads), kThreads, 0, v.stream>>>(b.flat.as<uint32_t>(), b.total, b.slot_off.as<uint32_t>(),
                                                                                                              b.args.n_seqs, b.min_off.as<uint32_t>());
        UNIT_CHECK(hipGetLastError());
    }
}

float span_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    UNIT_CHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
}

// One range: reads g.k0 .. g.k1 sketched, their minimizers looked up, the hits sorted and appended to the index's kept anchors.
// On a canonical index (pwa_mm_seed_strands) a read has two lists, whose cuts are known only once the hits are gathered and sorted:
// the total comes from the scan, the 2 nr + 1 offsets from the sorted keys, and the split turns the reverse lists' tied runs round.
void mm_seed_range(pwa::SaCtxView& v, pwa_mm_index* ix, const SeedCall& c, const uint8_t* bytes, const pwa::Run& g, SketchBuffers& sb, SeedBuffers& b,
                   pwa::Events<8>& ev, uint64_t* anc_off_out, const char* who) {
    const uint32_t nr = (uint32_t)(g.k1 - g.k0);
    const bool two = ix->canonical;
    const size_t lists = (size_t)nr * (two ? 2 : 1), first = (size_t)g.k0 * (two ? 2 : 1);
    const size_t kept = ix->anc_t.size();
    sketch_count(v, bytes, c.off, g.k0, g.k1, ix->k, ix->w, sb, &ev.e[0]);
    ix->sketch_ms += span_ms(ev.e[0], ev.e[1]);
    ix->ranges += 1;
    const uint32_t nm = sb.total;
    ix->minimizers += nm;
    for (size_t i = 0; i < lists; ++i) anc_off_out[first + i] = kept;
    if (!nm) return;   // (every k-mer of the range holds a byte that is not ACGT, or is a reverse palindrome)
    fit(v.poison, sb.hash, (size_t)nm * 8);
    fit(v.poison, sb.pos, (size_t)nm * 4);
    fit(v.poison, b.lo, (size_t)nm * 4);
    fit(v.poison, b.cnt, ((size_t)nm + 1) * 4);
    fit(v.poison, b.slot_part, pwa::scan_part_words((size_t)nm + 1) * 4);
    fit(v.poison, b.anc_off, (lists + 1) * 4);
    uint32_t* hit_off = b.cnt.as<uint32_t>();   // the counts, then, scanned, where each minimizer's hits start; the total last
    UNIT_CHECK(hipMemsetAsync(hit_off + nm, 0, 4, v.stream));
    UNIT_CHECK(hipEventRecord(ev.e[2], v.stream));
    sketch_write(v, sb, sb.hash.as<uint64_t>(), sb.pos.as<uint32_t>(), true);
    UNIT_CHECK(hipEventRecord(ev.e[3], v.stream));
    mm::lookup_kernel<<<blocks_for(nm, kThreads), kThreads, 0, v.stream>>>(ix->hashes(), ix->n_min, sb.hash.as<uint64_t>(), nm, c.max_occ, b.lo.as<uint32_t>(),
                                                                          hit_off);
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[4], v.stream));
    pwa::scan_excl(v.stream, hit_off, (size_t)nm + 1, b.slot_part.as<uint32_t>());
    b.h_anc_off.resize(lists + 1);
    if (two) {
        UNIT_CHECK(hipMemcpyAsync(&b.h_anc_off[lists], hit_off + nm, 4, hipMemcpyDeviceToHost, v.stream));
    } else {
        seed_read_offsets_kernel<<<blocks_for((size_t)nr + 1, kThreads), kThreads, 0, v.stream>>>(hit_off, sb.min_off.as<uint32_t>(), nr, b.anc_off.as<uint32_t>());
        UNIT_CHECK(hipGetLastError());
        UNIT_CHECK(hipMemcpyAsync(b.h_anc_off.data(), b.anc_off.p, ((size_t)nr + 1) * 4, hipMemcpyDeviceToHost, v.stream));
    }
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    sb.check_fault(who);
    const uint32_t total = b.h_anc_off[lists];
    if (!two)
        for (uint32_t i = 0; i < nr; ++i) anc_off_out[g.k0 + i] = kept + b.h_anc_off[i];
    ix->sketch_ms += span_ms(ev.e[2], ev.e[3]);
    ix->search_ms += span_ms(ev.e[3], ev.e[4]);
    ix->hits += total;
    if (!total) return;
    fit(v.poison, b.key, (size_t)total * 16);
    fit(v.poison, b.val, (size_t)total * 8);
    b.fit_sort(v.poison, total);
    SortBufs<uint64_t, uint32_t> s{{b.key.as<uint64_t>(), b.key.as<uint64_t>() + total}, {b.val.as<uint32_t>(), b.val.as<uint32_t>() + total}, 0};
    UNIT_CHECK(hipEventRecord(ev.e[5], v.stream));
    if (two)
        mm::gather_strands_kernel<<<blocks_for(total, kThreads), kThreads, 0, v.stream>>>(ix->positions(), ix->n_min, b.lo.as<uint32_t>(), hit_off, nm, total,
                                                                                         sb.min_off.as<uint32_t>(), nr, sb.pos.as<uint32_t>(),
                                                                                         sb.seq_off.as<uint64_t>(), ix->k, s.k[0], s.v[0],
                                                                                         sb.fault.as<uint32_t>());
    else
        mm::gather_kernel<<<blocks_for(total, kThreads), kThreads, 0, v.stream>>>(ix->positions(), ix->n_min, b.lo.as<uint32_t>(), hit_off, nm, total,
                                                                                 sb.min_off.as<uint32_t>(), nr, sb.pos.as<uint32_t>(), s.k[0], s.v[0],
                                                                                 sb.fault.as<uint32_t>());
    UNIT_CHECK(hipGetLastError());
    radix_sort(v.stream, s, total, b.sc);
    uint32_t* d_t = reinterpret_cast<uint32_t*>(s.k[s.cur ^ 1]);   // the sort's other key buffer is free now
    const uint32_t* d_q = s.v[s.cur];
    if (two) {   // ... and so is its other value buffer
        mm::list_offsets_kernel<<<blocks_for(lists + 1, kThreads), kThreads, 0, v.stream>>>(s.k[s.cur], total, (uint32_t)lists, b.anc_off.as<uint32_t>());
        mm::split_strands_kernel<<<blocks_for(total, kThreads), kThreads, 0, v.stream>>>(s.k[s.cur], s.v[s.cur], total, d_t, s.v[s.cur ^ 1]);
        d_q = s.v[s.cur ^ 1];
    } else {
        seed_split_kernel<<<blocks_for(total, kThreads), kThreads, 0, v.stream>>>(s.k[s.cur], total, d_t);
    }
    UNIT_CHECK(hipGetLastError());
    UNIT_CHECK(hipEventRecord(ev.e[6], v.stream));
    ix->anc_t.resize(kept + total);
    ix->anc_q.resize(kept + total);
    UNIT_CHECK(hipMemcpyAsync(ix->anc_t.data() + kept, d_t, (size_t)total * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipMemcpyAsync(ix->anc_q.data() + kept, d_q, (size_t)total * 4, hipMemcpyDeviceToHost, v.stream));
    if (two) UNIT_CHECK(hipMemcpyAsync(b.h_anc_off.data(), b.anc_off.p, (lists + 1) * 4, hipMemcpyDeviceToHost, v.stream));
    UNIT_CHECK(hipStreamSynchronize(v.stream));
    sb.check_fault(who);
    if (two)
        for (size_t i = 0; i < lists; ++i) anc_off_out[first + i] = kept + b.h_anc_off[i];
    ix->sort_ms += span_ms(ev.e[5], ev.e[6]);
}

}  // namespace

// The sort above for another unit (sufarr_ctx.h): the chaining unit's candidate order
int pwa::sort_pairs(hipStream_t s, uint64_t* key2, uint32_t* val2, size_t n, SortScratch& sc) {
    SortBufs<uint64_t, uint32_t> b{{key2, key2 + n}, {val2, val2 + n}, 0};
    radix_sort(s, b, n, sc);
    return b.cur;
}

extern "C" {

int pwa_seed_plan(uint64_t text_n, const uint64_t* read_off, uint32_t n_reads, uint32_t k, uint32_t step, uint32_t max_occ, uint64_t budget_hits,
                  uint32_t* bad_read, uint64_t* n_slots, uint64_t* n_ranges) {
    const SeedCall c{text_n, read_off, n_reads, k, step, max_occ};
    uint32_t bad = kNoRead;
    uint64_t slots = 0, count = 0;
    std::string what;
    int rc = PWA_E_NOMEM;
    try {
        rc = seed_validate(c, bad, slots, what);
        if (rc == PWA_OK) count = seed_ranges(c, budget_hits).size();
    } catch (const std::bad_alloc&) {
        rc = PWA_E_NOMEM;
    }
    if (bad_read) *bad_read = bad;
    if (n_slots) *n_slots = slots;
    if (n_ranges) *n_ranges = count;
    return rc;
}

int pwa_sa_seed(pwa_sa_index* ix, const uint8_t* read_bytes, const uint64_t* read_off, uint32_t n_reads, uint32_t k, uint32_t step,
                uint32_t max_occ, uint64_t* anc_off_out) {
    if (!ix) return PWA_E_INVALID;
    pwa::SaCtxView v = pwa::sa_ctx_view(ix->ctx);
    const SeedCall c{ix->n, read_off, n_reads, k, step, max_occ};
    if (!anc_off_out || (!read_bytes && n_reads && read_off && read_off[n_reads] != read_off[0])) {
        *v.err = "pwa_sa_seed: a required pointer is null";
        return PWA_E_INVALID;
    }
    uint32_t bad = kNoRead;
    uint64_t slots = 0;
    std::string what;
    if (const int rc = seed_validate(c, bad, slots, what)) {
        *v.err = "pwa_sa_seed: " + what;
        return rc;
    }
    ix->seeded = false;
    ix->anc_t.clear();
    ix->anc_q.clear();
    ix->seed_search_ms = ix->seed_sort_ms = 0.f;
    ix->seed_slots = slots;
    ix->seed_hits = ix->seed_ranges = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = pwa::guarded(v, [&] {
        std::fill_n(anc_off_out, (size_t)n_reads + 1, 0ull);
        const std::vector<pwa::Run> ranges = seed_ranges(c, v.occ_chunk_hits);
        if (ranges.empty()) return;   // no read, no slot, or a text shorter than k: nothing for the device to do
        UNIT_CHECK(hipSetDevice(v.device));
        SeedBuffers b;
        pwa::Events<4> ev;
        UNIT_CHECK(ev.create());
        uint64_t done = 0;   // reads whose offsets are written
        for (const pwa::Run& g : ranges) {
            for (; done < g.k0; ++done) anc_off_out[done] = ix->anc_t.size();   // the reads of a range without a slot
            seed_range(v, ix, c, read_bytes, g, b, ev, anc_off_out);
            done = g.k1;
        }
        for (; done <= n_reads; ++done) anc_off_out[done] = ix->anc_t.size();
        if (v.debug)
            std::fprintf(stderr, "[pwa] sa seed: %u reads, k=%u step=%u max_occ=%u: %llu slots, %llu hits, %llu ranges, search %.3f ms, sort %.3f ms, call %.3f ms\n",
                         n_reads, k, step, max_occ, (unsigned long long)ix->seed_slots, (unsigned long long)ix->seed_hits,
                         (unsigned long long)ix->seed_ranges, ix->seed_search_ms, ix->seed_sort_ms, ms_since(t0));
    });
    ix->seeded = rc == PWA_OK;
    return rc;
}

int pwa_sa_seed_fetch(const pwa_sa_index* ix, uint32_t* anc_t, uint32_t* anc_q, uint64_t cap) {
    if (!ix || !ix->seeded) return PWA_E_INVALID;
    const uint64_t total = ix->anc_t.size();
    if (cap < total) {
        *pwa::sa_ctx_view(ix->ctx).err = "pwa_sa_seed_fetch: " + std::to_string(total) + " anchors, capacity " + std::to_string(cap);
        return PWA_E_CAPACITY;
    }
    if (total && (!anc_t || !anc_q)) return PWA_E_INVALID;
    std::copy(ix->anc_t.begin(), ix->anc_t.end(), anc_t);
    std::copy(ix->anc_q.begin(), ix->anc_q.end(), anc_q);
    return PWA_OK;
}

int pwa_sa_seed_last_stats(const pwa_sa_index* ix, float* search_ms, float* sort_ms, uint64_t* slots, uint64_t* hits, uint64_t* ranges) {
    if (!ix) return PWA_E_INVALID;
    if (search_ms) *search_ms = ix->seed_search_ms;
    if (sort_ms) *sort_ms = ix->seed_sort_ms;
    if (slots) *slots = ix->seed_slots;
    if (hits) *hits = ix->seed_hits;
    if (ranges) *ranges = ix->seed_ranges;
    return PWA_OK;
}

int pwa_sa_create(pwa_ctx* ctx, const uint8_t* text, uint64_t n, pwa_sa_index** out) {
    if (!ctx || !out || (!text && n)) return PWA_E_INVALID;
    *out = nullptr;
    pwa::SaCtxView v = pwa::sa_ctx_view(ctx);
    if (n >= (1ull << 31)) {
        *v.err = "pwa_sa_create: a text of " + std::to_string(n) + " bytes; positions are int32, so at most 2^31 - 1";
        return PWA_E_CAPACITY;
    }
    pwa_sa_index* ix = new (std::nothrow) pwa_sa_index();
    if (!ix) return PWA_E_NOMEM;
    ix->ctx = ctx;
    ix->n = (uint32_t)n;
    const int rc = pwa::guarded(v, [&] {
        (void)hipSetDevice(v.device);
        const auto t0 = std::chrono::steady_clock::now();
        const size_t tbytes = (n + 7) / 8 * 8 + 16;
        UNIT_CHECK(ix->d_text.alloc(v.poison, tbytes));
        UNIT_CHECK(ix->d_sa.alloc(v.poison, std::max<size_t>(n, 1) * 4));
        uint8_t* d_text = ix->d_text.as<uint8_t>();
        uint32_t* d_sa = ix->d_sa.as<uint32_t>();
        UNIT_CHECK(hipMemsetAsync(d_text, 0, tbytes, v.stream));
        if (n) UNIT_CHECK(hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, v.stream));
        // alphabet: codes 1 .. sigma in signed-char order, as few bits per code as sigma allows, as many codes per 64-bit key as fit
        std::vector<uint64_t> seen(256, 0);
        for (uint64_t i = 0; i < n; ++i) seen[text[i]] = 1;
        CodeTable tab{};
        int sigma = 0;
        for (int c = -128; c < 128; ++c)
            if (seen[(uint8_t)c]) tab.c[(uint8_t)c] = (uint16_t)++sigma;
        int bits = 1;
        while ((1 << bits) <= sigma) ++bits;
        const int k = 64 / bits;
        pwa::Events<2> ev;
        UNIT_CHECK(ev.create());
        UNIT_CHECK(hipEventRecord(ev.e[0], v.stream));
        int passes = 0;
        if (n) {
            Dev key2, val2, rank, head;
            SortScratch sc;
            UNIT_CHECK(key2.alloc(v.poison, n * 8 * 2));
            UNIT_CHECK(val2.alloc(v.poison, n * 4));
            UNIT_CHECK(rank.alloc(v.poison, n * 4));
            UNIT_CHECK(head.alloc(v.poison, (n + 1) * 4));
            sc.alloc(v.poison, n);
            SortBufs<uint64_t, uint32_t> b{{key2.as<uint64_t>(), key2.as<uint64_t>() + n}, {d_sa, val2.as<uint32_t>()}, 0};
            const uint32_t nb = blocks_for(n, kThreads), nn = (uint32_t)n;
            sa_first_key_kernel<<<nb, kThreads, 0, v.stream>>>(d_text, nn, tab, bits, k, b.k[0], b.v[0]);
            UNIT_CHECK(hipGetLastError());
            passes += radix_sort(v.stream, b, n, sc);
            ix->rounds = 1;
            uint32_t h = (uint32_t)k;
            for (;;) {
                sa_heads_kernel<<<blocks_for(n + 1, kThreads), kThreads, 0, v.stream>>>(b.k[b.cur], nn, head.as<uint32_t>());
                pwa::scan_excl(v.stream, head.as<uint32_t>(), n + 1, sc.part.as<uint32_t>());
                uint32_t groups = 0;
                UNIT_CHECK(hipMemcpyAsync(&groups, head.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, v.stream));
                UNIT_CHECK(hipStreamSynchronize(v.stream));
                if (groups == nn) break;
                if (h >= nn || ix->rounds >= 40) throw Fail{PWA_E_HIP, "pwa_sa_create: prefix doubling did not separate the suffixes"};
                sa_rank_kernel<<<nb, kThreads, 0, v.stream>>>(b.k[b.cur], b.v[b.cur], head.as<uint32_t>(), nn, rank.as<uint32_t>());
                sa_pair_key_kernel<<<nb, kThreads, 0, v.stream>>>(rank.as<uint32_t>(), nn, h, b.k[b.cur], b.v[b.cur]);
                UNIT_CHECK(hipGetLastError());
                passes += radix_sort(v.stream, b, n, sc);
                ++ix->rounds;
                h = h > (1u << 30) ? nn : 2 * h;
            }
            if (b.v[b.cur] != d_sa) UNIT_CHECK(hipMemcpyAsync(d_sa, b.v[b.cur], n * 4, hipMemcpyDeviceToDevice, v.stream));
        }
        UNIT_CHECK(hipEventRecord(ev.e[1], v.stream));
        UNIT_CHECK(hipStreamSynchronize(v.stream));
        UNIT_CHECK(hipEventElapsedTime(&ix->build_ms, ev.e[0], ev.e[1]));
        if (v.debug)
            std::fprintf(stderr, "[pwa] sa build: n=%llu sigma=%d codes/key=%d rounds=%u passes=%d device %.3f ms, call %.3f ms\n",
                         (unsigned long long)n, sigma, k, ix->rounds, passes, ix->build_ms, ms_since(t0));
    });
    if (rc == PWA_OK)
        *out = ix;
    else
        delete ix;   // (half built)
    return rc;
}

int pwa_sa_fetch(pwa_sa_index* ix, uint32_t* sa_out) {
    if (!ix || (!sa_out && ix->n)) return PWA_E_INVALID;
    pwa::SaCtxView v = pwa::sa_ctx_view(ix->ctx);
    return pwa::guarded(v, [&] {
        if (ix->n) UNIT_CHECK(hipMemcpyAsync(sa_out, ix->d_sa.p, (size_t)ix->n * 4, hipMemcpyDeviceToHost, v.stream));
        UNIT_CHECK(hipStreamSynchronize(v.stream));
    });
}

int pwa_sa_find(pwa_sa_index* ix, const uint8_t* pat_bytes, const uint64_t* pat_off, uint32_t n_pat, uint32_t* counts_out) {
    if (!ix || (!counts_out && n_pat) || !patterns_ok(pat_bytes, pat_off, n_pat)) return PWA_E_INVALID;
    pwa::SaCtxView v = pwa::sa_ctx_view(ix->ctx);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = pwa::guarded(v, [&] {
        Ranges r;
        search(v, ix, pat_bytes, pat_off, n_pat, r);
        std::copy(r.h_cnt.begin(), r.h_cnt.end(), counts_out);
    });
    if (rc == PWA_OK) ix->search_ms = (float)ms_since(t0);
    return rc;
}

int pwa_sa_occurrences(pwa_sa_index* ix, const uint8_t* pat_bytes, const uint64_t* pat_off, uint32_t n_pat, const uint32_t* ref_start,
                       uint32_t n_ref, const uint32_t* header_rank, uint64_t* occ_off, uint64_t* occ, uint64_t cap, uint64_t* needed) {
    if (!ix || !occ_off || !ref_start || (!header_rank && n_ref) || (!occ && cap) || !patterns_ok(pat_bytes, pat_off, n_pat)) return PWA_E_INVALID;
    if (ref_start[0] != 0 || ref_start[n_ref] != ix->n) return PWA_E_INVALID;
    for (uint32_t r = 0; r < n_ref; ++r)
        if (ref_start[r + 1] <= ref_start[r]) return PWA_E_INVALID;   // every reference holds at least its terminator
    pwa::SaCtxView v = pwa::sa_ctx_view(ix->ctx);
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t kept = 0;
    const int rc = pwa::guarded(v, [&] {
        Ranges r;
        search(v, ix, pat_bytes, pat_off, n_pat, r);
        const uint64_t budget = v.occ_chunk_hits ? v.occ_chunk_hits : kDefaultChunkHits;
        // chunks of consecutive patterns: raw hits within the budget, or one pattern that alone exceeds it (at most n hits)
        const std::vector<pwa::Run> chunks = pwa::cut_runs(n_pat, budget, [&](uint64_t p) { return (uint64_t)r.h_cnt[p]; });
        uint64_t max_hits = 0;
        uint32_t max_np = 0;
        for (const pwa::Run& c : chunks) {
            max_hits = std::max(max_hits, c.weight);
            max_np = std::max(max_np, (uint32_t)(c.k1 - c.k0));
        }
        Dev d_ref, d_rank, key, pid, off;
        SortScratch sc;
        if (max_hits) {
            UNIT_CHECK(d_ref.alloc(v.poison, ((size_t)n_ref + 1) * 4));
            UNIT_CHECK(d_rank.alloc(v.poison, (size_t)n_ref * 4));
            UNIT_CHECK(hipMemcpyAsync(d_ref.p, ref_start, ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice, v.stream));
            if (n_ref) UNIT_CHECK(hipMemcpyAsync(d_rank.p, header_rank, (size_t)n_ref * 4, hipMemcpyHostToDevice, v.stream));
            UNIT_CHECK(key.alloc(v.poison, max_hits * 16));
            UNIT_CHECK(pid.alloc(v.poison, max_hits * 8));
            UNIT_CHECK(off.alloc(v.poison, ((size_t)max_np + 1) * 4));
            sc.alloc(v.poison, std::max<uint64_t>(max_hits, (uint64_t)max_np + 1));   // (the offsets scan of a chunk of many hit-less patterns)
        }
        std::vector<uint64_t> h_key;
        int n_chunks = 0;
        for (const pwa::Run& c : chunks) {
            const uint32_t p0 = (uint32_t)c.k0, p1 = (uint32_t)c.k1, np = p1 - p0;
            const uint64_t total = c.weight;
            if (total) {
                ++n_chunks;
                uint32_t* d_off = off.as<uint32_t>();
                UNIT_CHECK(hipMemcpyAsync(d_off, r.cnt.as<uint32_t>() + p0, (size_t)np * 4, hipMemcpyDeviceToDevice, v.stream));
                UNIT_CHECK(hipMemsetAsync(d_off + np, 0, 4, v.stream));
                pwa::scan_excl(v.stream, d_off, (size_t)np + 1, sc.part.as<uint32_t>());
                SortBufs<uint64_t, uint32_t> s1{{key.as<uint64_t>(), key.as<uint64_t>() + max_hits}, {pid.as<uint32_t>(), pid.as<uint32_t>() + max_hits}, 0};
                occ_gather_kernel<<<blocks_for(total, kThreads), kThreads, 0, v.stream>>>(ix->d_sa.as<uint32_t>(), r.lo.as<uint32_t>() + p0, d_off, np, (uint32_t)total,
                                                                                          d_ref.as<uint32_t>(), n_ref, d_rank.as<uint32_t>(), s1.k[0], s1.v[0]);
                UNIT_CHECK(hipGetLastError());
                radix_sort(v.stream, s1, total, sc);   // by key ...
                SortBufs<uint32_t, uint64_t> s2{{s1.v[0], s1.v[1]}, {s1.k[0], s1.k[1]}, s1.cur};
                radix_sort(v.stream, s2, total, sc);   // ... then, stably, by pattern
                h_key.resize(total);
                UNIT_CHECK(hipMemcpyAsync(h_key.data(), s2.v[s2.cur], total * 8, hipMemcpyDeviceToHost, v.stream));
                UNIT_CHECK(hipStreamSynchronize(v.stream));
            }
            uint64_t at = 0;
            for (uint32_t p = p0; p < p1; ++p) {
                occ_off[p] = kept;
                for (const uint64_t e = at + r.h_cnt[p]; at < e; ++at)
                    if (h_key[at] != ~0ull) {   // (hits on a terminator)
                        if (kept < cap) occ[kept] = h_key[at];
                        ++kept;
                    }
            }
        }
        occ_off[n_pat] = kept;
        if (v.debug)
            std::fprintf(stderr, "[pwa] sa occurrences: %u patterns, %zu chunks (%d with hits), %llu hits kept, %.3f ms\n", n_pat, chunks.size(),
                         n_chunks, (unsigned long long)kept, ms_since(t0));
    });
    if (rc != PWA_OK) return rc;
    ix->search_ms = (float)ms_since(t0);
    if (needed) *needed = kept;
    if (kept > cap) {
        *v.err = "pwa_sa_occurrences: " + std::to_string(kept) + " occurrences, capacity " + std::to_string(cap);
        return PWA_E_CAPACITY;
    }
    return PWA_OK;
}

int pwa_sa_last_stats(const pwa_sa_index* ix, uint32_t* rounds, float* build_ms, float* search_ms) {
    if (!ix) return PWA_E_INVALID;
    if (rounds) *rounds = ix->rounds;
    if (build_ms) *build_ms = ix->build_ms;
    if (search_ms) *search_ms = ix->search_ms;
    return PWA_OK;
}

void pwa_sa_destroy(pwa_sa_index* ix) { delete ix; }

// ---- minimizer sketches, the minimizer index, seeding against it

// pwa_mm_create and pwa_mm_create_canonical
static int mm_create(const char* who, pwa_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t k, uint32_t w, bool canonical, pwa_mm_index** out) {
    if (!ctx || !out || (!text && n)) return PWA_E_INVALID;
    *out = nullptr;
    pwa::SaCtxView v = pwa::sa_ctx_view(ctx);
    if (!mm_params_ok(k, w)) {
        *v.err = std::string(who) + ": k is 1 .. 31 and w is 1 .. 128";
        return PWA_E_INVALID;
    }
    if (n >= (1ull << 31)) {
        *v.err = std::string(who) + ": a text of " + std::to_string(n) + " bytes; at most 2^31 - 1";
        return PWA_E_CAPACITY;
    }
    pwa_mm_index* ix = new (std::nothrow) pwa_mm_index();
    if (!ix) return PWA_E_NOMEM;
    ix->ctx = ctx;
    ix->k = k;
    ix->w = w;
    ix->canonical = canonical;
    const int rc = pwa::guarded(v, [&] {
        if (!kmers_of(n, k)) return;   // n < k: a valid, empty index
        UNIT_CHECK(hipSetDevice(v.device));
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t off[2] = {0, n};
        SketchBuffers b;
        pwa::Events<4> ev;
        UNIT_CHECK(ev.create());
        b.start(v, canonical);
        sketch_count(v, text, off, 0, 1, k, w, b, &ev.e[0]);
        ix->n_min = b.total;
        ix->build_ms = span_ms(ev.e[0], ev.e[1]);
        if (!b.total) return;   // no k-mer of the text is over ACGT alone
        SortScratch sc;
        UNIT_CHECK(ix->d_hash.alloc(v.poison, (size_t)b.total * 16));
        UNIT_CHECK(ix->d_pos.alloc(v.poison, (size_t)b.total * 8));
        sc.alloc(v.poison, b.total);
        UNIT_CHECK(hipEventRecord(ev.e[2], v.stream));
        sketch_write(v, b, ix->d_hash.as<uint64_t>(), ix->d_pos.as<uint32_t>(), false);
        ix->half = pwa::sort_pairs(v.stream, ix->d_hash.as<uint64_t>(), ix->d_pos.as<uint32_t>(), b.total, sc);   // stable: (hash, t) order
        UNIT_CHECK(hipEventRecord(ev.e[3], v.stream));
        UNIT_CHECK(hipStreamSynchronize(v.stream));
        b.check_fault(who);
        ix->build_ms += span_ms(ev.e[2], ev.e[3]);
        if (v.debug)
            std::fprintf(stderr, "[pwa] mm build%s: n=%llu k=%u w=%u: %u minimizers, device %.3f ms, call %.3f ms\n", canonical ? " (canonical)" : "",
                         (unsigned long long)n, k, w, ix->n_min, ix->build_ms, ms_since(t0));
    });
    if (rc == PWA_OK)
        *out = ix;
    else
        delete ix;   // (half built)
    return rc;
}

int pwa_mm_create(pwa_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t k, uint32_t w, pwa_mm_index** out) {
    return mm_create("pwa_mm_create", ctx, text, n, k, w, false, out);
}

int pwa_mm_create_canonical(pwa_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t k, uint32_t w, pwa_mm_index** out) {
    return mm_create("pwa_mm_create_canonical", ctx, text, n, k, w, true, out);
}

void pwa_mm_destroy(pwa_mm_index* ix) { delete ix; }

// Position words as the canonical kernels leave them, taken apart on the host: bit 31 into strand_out (where wanted), the rest stays
static void split_strand_words(uint32_t* pos, uint8_t* strand_out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        if (strand_out) strand_out[i] = (uint8_t)(pos[i] >> 31);
        pos[i] &= ~mm::kStrandBit;
    }
}

// pwa_mm_fetch and, with want_strand, pwa_mm_fetch_canonical
static int mm_fetch(const char* who, pwa_mm_index* ix, uint64_t* hash_out, uint32_t* pos_out, uint8_t* strand_out, bool want_strand, uint64_t cap) {
    if (!ix) return PWA_E_INVALID;
    pwa::SaCtxView v = pwa::sa_ctx_view(ix->ctx);
    if (want_strand && !ix->canonical) {
        *v.err = std::string(who) + ": the index is not canonical (pwa_mm_create_canonical builds one)";
        return PWA_E_INVALID;
    }
    if (cap < ix->n_min) {
        *v.err = std::string(who) + ": " + std::to_string(ix->n_min) + " minimizers, capacity " + std::to_string(cap);
        return PWA_E_CAPACITY;
    }
    if (ix->n_min && (!hash_out || !pos_out || (want_strand && !strand_out))) return PWA_E_INVALID;
    return pwa::guarded(v, [&] {
        if (!ix->n_min) return;
        UNIT_CHECK(hipMemcpyAsync(hash_out, ix->hashes(), (size_t)ix->n_min * 8, hipMemcpyDeviceToHost, v.stream));
        UNIT_CHECK(hipMemcpyAsync(pos_out, ix->positions(), (size_t)ix->n_min * 4, hipMemcpyDeviceToHost, v.stream));
        UNIT_CHECK(hipStreamSynchronize(v.stream));
        if (ix->canonical) split_strand_words(pos_out, strand_out, ix->n_min);
    });
}

int pwa_mm_fetch(pwa_mm_index* ix, uint64_t* hash_out, uint32_t* pos_out, uint64_t cap) {
    return mm_fetch("pwa_mm_fetch", ix, hash_out, pos_out, nullptr, false, cap);
}

int pwa_mm_fetch_canonical(pwa_mm_index* ix, uint64_t* hash_out, uint32_t* pos_out, uint8_t* strand_out, uint64_t cap) {
    return mm_fetch("pwa_mm_fetch_canonical", ix, hash_out, pos_out, strand_out, true, cap);
}

int pwa_mm_last_stats(const pwa_mm_index* ix, uint64_t* n_min, float* build_ms) {
    if (!ix) return PWA_E_INVALID;
    if (n_min) *n_min = ix->n_min;
    if (build_ms) *build_ms = ix->build_ms;
    return PWA_OK;
}

// pwa_mm_sketch and, with canonical, pwa_mm_sketch_canonical (strand_out beside pos_out)
static int mm_sketch(const std::string& who, pwa_ctx* ctx, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seqs, uint32_t k, uint32_t w,
                     bool canonical, uint64_t* min_off_out, uint32_t* pos_out, uint64_t* hash_out, uint8_t* strand_out, uint64_t cap, uint64_t* needed) {
    if (!ctx || !min_off_out || (n_seqs && !seq_off) || (cap && (!pos_out || !hash_out || (canonical && !strand_out)))) return PWA_E_INVALID;
    pwa::SaCtxView v = pwa::sa_ctx_view(ctx);
    if (!seq_bytes && n_seqs && seq_off[n_seqs] != seq_off[0]) {
        *v.err = who + ": a required pointer is null";
        return PWA_E_INVALID;
    }
    std::string what;
    if (const int rc = sketch_validate(seq_off, n_seqs, k, w, what)) {
        *v.err = who + ": " + what;
        return rc;
    }
    uint64_t kept = 0;
    const int rc = pwa::guarded(v, [&] {
        std::fill_n(min_off_out, (size_t)n_seqs + 1, 0ull);
        const uint64_t budget = std::min<uint64_t>(v.occ_chunk_hits ? v.occ_chunk_hits : kDefaultChunkHits, 0xFFFFFFFFull);
        // consecutive sequences whose k-mers fit the budget, or one that alone exceeds it (below 2^31 k-mers)
        const std::vector<pwa::Run> runs = pwa::cut_runs(n_seqs, budget, [&](uint64_t r) { return kmers_of(seq_off[r + 1] - seq_off[r], k); });
        SketchBuffers b;
        bool started = false;
        uint64_t done = 0;   // sequences whose offsets are written
        for (const pwa::Run& g : runs) {
            if (!g.weight) continue;
            if (!started) {
                UNIT_CHECK(hipSetDevice(v.device));
                b.start(v, canonical);
                started = true;
            }
            for (; done < g.k0; ++done) min_off_out[done] = kept;
            sketch_count(v, seq_bytes, seq_off, g.k0, g.k1, k, w, b, nullptr);
            const uint32_t nr = (uint32_t)(g.k1 - g.k0);
            fit(v.poison, b.hash, (size_t)b.total * 8);
            fit(v.poison, b.pos, (size_t)b.total * 4);
            sketch_write(v, b, b.hash.as<uint64_t>(), b.pos.as<uint32_t>(), true);
            b.h_min_off.resize((size_t)nr + 1);
            UNIT_CHECK(hipMemcpyAsync(b.h_min_off.data(), b.min_off.p, ((size_t)nr + 1) * 4, hipMemcpyDeviceToHost, v.stream));
            if (b.total && kept + b.total <= cap) {
                UNIT_CHECK(hipMemcpyAsync(hash_out + kept, b.hash.p, (size_t)b.total * 8, hipMemcpyDeviceToHost, v.stream));
                UNIT_CHECK(hipMemcpyAsync(pos_out + kept, b.pos.p, (size_t)b.total * 4, hipMemcpyDeviceToHost, v.stream));
            }
            UNIT_CHECK(hipStreamSynchronize(v.stream));
            b.check_fault(who.c_str());
            if (canonical && b.total && kept + b.total <= cap) split_strand_words(pos_out + kept, strand_out + kept, b.total);
            for (uint32_t i = 0; i < nr; ++i) min_off_out[g.k0 + i] = kept + b.h_min_off[i];
            kept += b.total;
            done = g.k1;
        }
        for (; done <= n_seqs; ++done) min_off_out[done] = kept;
    });
    if (rc != PWA_OK) return rc;
    if (needed) *needed = kept;
    if (kept > cap) {
        *v.err = who + ": " + std::to_string(kept) + " minimizers, capacity " + std::to_string(cap);
        return PWA_E_CAPACITY;
    }
    return PWA_OK;
}

int pwa_mm_sketch(pwa_ctx* ctx, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seqs, uint32_t k, uint32_t w, uint64_t* min_off_out,
                  uint32_t* pos_out, uint64_t* hash_out, uint64_t cap, uint64_t* needed) {
    return mm_sketch("pwa_mm_sketch", ctx, seq_bytes, seq_off, n_seqs, k, w, false, min_off_out, pos_out, hash_out, nullptr, cap, needed);
}

int pwa_mm_sketch_canonical(pwa_ctx* ctx, const uint8_t* seq_bytes, const uint64_t* seq_off, uint32_t n_seqs, uint32_t k, uint32_t w,
                            uint64_t* min_off_out, uint32_t* pos_out, uint64_t* hash_out, uint8_t* strand_out, uint64_t cap, uint64_t* needed) {
    return mm_sketch("pwa_mm_sketch_canonical", ctx, seq_bytes, seq_off, n_seqs, k, w, true, min_off_out, pos_out, hash_out, strand_out, cap, needed);
}

int pwa_mm_plan(uint64_t n_min, const uint64_t* read_off, uint32_t n_reads, uint32_t k, uint32_t max_occ, uint64_t budget_hits, uint32_t* bad_read,
                uint64_t* n_slots, uint64_t* n_ranges) {
    const SeedCall c = mm_call(n_min, read_off, n_reads, k, max_occ);
    uint32_t bad = kNoRead;
    uint64_t slots = 0, count = 0;
    std::string what;
    int rc = PWA_E_NOMEM;
    try {
        rc = k > mm::kMaxK ? PWA_E_INVALID : seed_validate(c, bad, slots, what);
        if (rc == PWA_OK) count = seed_ranges(c, budget_hits).size();
    } catch (const std::bad_alloc&) {
        rc = PWA_E_NOMEM;
    }
    if (bad_read) *bad_read = bad;
    if (n_slots) *n_slots = slots;
    if (n_ranges) *n_ranges = count;
    return rc;
}

// pwa_mm_seed (a plain index, one list per read) and pwa_mm_seed_strands (a canonical one, two)
static int mm_seed(const std::string& who, bool strands, pwa_mm_index* ix, const uint8_t* read_bytes, const uint64_t* read_off, uint32_t n_reads,
                   uint32_t max_occ, uint64_t* anc_off_out) {
    if (!ix) return PWA_E_INVALID;
    pwa::SaCtxView v = pwa::sa_ctx_view(ix->ctx);
    const SeedCall c = mm_call(ix->n_min, read_off, n_reads, ix->k, max_occ);
    if (!anc_off_out || (!read_bytes && n_reads && read_off && read_off[n_reads] != read_off[0])) {
        *v.err = who + ": a required pointer is null";
        return PWA_E_INVALID;
    }
    if (strands != ix->canonical) {
        *v.err = who + (strands ? ": the index is not canonical; pwa_mm_seed seeds a plain index" : ": the index is canonical; pwa_mm_seed_strands seeds it");
        return PWA_E_INVALID;
    }
    if (strands && n_reads > 0x7FFFFFFFu) {
        *v.err = who + ": " + std::to_string(n_reads) + " reads; at most 2^31 - 1, two lists each";
        return PWA_E_CAPACITY;
    }
    uint32_t bad = kNoRead;
    uint64_t slots = 0;
    std::string what;
    if (const int rc = seed_validate(c, bad, slots, what)) {
        *v.err = who + " (the text's k-mers being the index's minimizers): " + what;
        return rc;
    }
    ix->seeded = false;
    ix->anc_t.clear();
    ix->anc_q.clear();
    ix->sketch_ms = ix->search_ms = ix->sort_ms = 0.f;
    ix->slots = slots;
    ix->minimizers = ix->hits = ix->ranges = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t per = strands ? 2 : 1;   // lists per read
    const int rc = pwa::guarded(v, [&] {
        std::fill_n(anc_off_out, per * n_reads + 1, 0ull);
        const std::vector<pwa::Run> ranges = seed_ranges(c, v.occ_chunk_hits);
        if (ranges.empty()) return;   // no read, no k-mer, or an empty index: nothing for the device to do
        UNIT_CHECK(hipSetDevice(v.device));
        SketchBuffers sb;
        SeedBuffers b;
        pwa::Events<8> ev;
        UNIT_CHECK(ev.create());
        sb.start(v, strands);
        size_t done = 0;   // lists whose offsets are written
        for (const pwa::Run& g : ranges) {
            for (; done < per * g.k0; ++done) anc_off_out[done] = ix->anc_t.size();   // the reads of a range without a k-mer
            mm_seed_range(v, ix, c, read_bytes, g, sb, b, ev, anc_off_out, who.c_str());
            done = per * g.k1;
        }
        for (; done <= per * n_reads; ++done) anc_off_out[done] = ix->anc_t.size();
        if (v.debug)
            std::fprintf(stderr, "[pwa] mm seed%s: %u reads, k=%u w=%u max_occ=%u: %llu slots, %llu minimizers, %llu hits, %llu ranges, sketch %.3f ms, search %.3f ms, sort %.3f ms, call %.3f ms\n",
                         strands ? " (strands)" : "", n_reads, ix->k, ix->w, max_occ, (unsigned long long)ix->slots, (unsigned long long)ix->minimizers, (unsigned long long)ix->hits,
                         (unsigned long long)ix->ranges, ix->sketch_ms, ix->search_ms, ix->sort_ms, ms_since(t0));
    });
    ix->seeded = rc == PWA_OK;
    return rc;
}

int pwa_mm_seed(pwa_mm_index* ix, const uint8_t* read_bytes, const uint64_t* read_off, uint32_t n_reads, uint32_t max_occ, uint64_t* anc_off_out) {
    return mm_seed("pwa_mm_seed", false, ix, read_bytes, read_off, n_reads, max_occ, anc_off_out);
}

int pwa_mm_seed_strands(pwa_mm_index* ix, const uint8_t* read_bytes, const uint64_t* read_off, uint32_t n_reads, uint32_t max_occ,
                        uint64_t* anc_off_out) {
    return mm_seed("pwa_mm_seed_strands", true, ix, read_bytes, read_off, n_reads, max_occ, anc_off_out);
}

int pwa_mm_seed_fetch(const pwa_mm_index* ix, uint32_t* anc_t, uint32_t* anc_q, uint64_t cap) {
    if (!ix || !ix->seeded) return PWA_E_INVALID;
    const uint64_t total = ix->anc_t.size();
    if (cap < total) {
        *pwa::sa_ctx_view(ix->ctx).err = "pwa_mm_seed_fetch: " + std::to_string(total) + " anchors, capacity " + std::to_string(cap);
        return PWA_E_CAPACITY;
    }
    if (total && (!anc_t || !anc_q)) return PWA_E_INVALID;
    std::copy(ix->anc_t.begin(), ix->anc_t.end(), anc_t);
    std::copy(ix->anc_q.begin(), ix->anc_q.end(), anc_q);
    return PWA_OK;
}

int pwa_mm_seed_last_stats(const pwa_mm_index* ix, float* sketch_ms, float* search_ms, float* sort_ms, uint64_t* slots, uint64_t* minimizers,
                           uint64_t* hits, uint64_t* ranges) {
    if (!ix) return PWA_E_INVALID;
    if (sketch_ms) *sketch_ms = ix->sketch_ms;
    if (search_ms) *search_ms = ix->search_ms;
    if (sort_ms) *sort_ms = ix->sort_ms;
    if (slots) *slots = ix->slots;
    if (minimizers) *minimizers = ix->minimizers;
    if (hits) *hits = ix->hits;
    if (ranges) *ranges = ix->ranges;
    return PWA_OK;
}

}  // extern "C"
