// wfa.hip.h -- wavefront (WFA, Marco-Sola et al. 2021) affine-gap global alignment of long pairs (gfx950 / MI355X): the sweep by
// penalty and the backtrace over the stored wavefronts.  Semantics: include/pwalign.h ("Wavefront alignments"); DESIGN.md §3.21.
//
// One wave per pair, four waves per workgroup, nothing between waves: no flags, no spin-waits, every loop bounded by the host's plan
// (the sweep by P_max, an extend by the two lengths, the walk by the op region).  Lanes are diagonals, in chunks of 64.  A pair's
// wavefronts live in its own workspace in global memory; what a lane reads was stored by lanes of the SAME wave at an earlier score,
// so a workgroup-scope release / acquire (wait counts only, the CU's own L1) orders it -- no agent-scope fence anywhere.
//
// Layout of wavefront s with the planned span [lo, hi] (w = hi - lo + 1 cells): M[w], I[w], D[w] as int32 offsets, kNull for none,
// at cell offset cum(s) of the workspace (alignment form: every wavefront up to P_max, 12 bytes per planned cell) or in slot
// s mod R of a ring of R = max(x, o + e) + 1 wavefronts of the widest span (score form; the codes form too, which adds one code byte
// per planned cell behind the ring and backtraces over those: wfa_codes_sweep_kernel, wfa_codes_walk_kernel).  A score whose three
// source wavefronts are all empty is skipped in O(1): its first M cell takes kEmpty, which no computed cell ever holds, and that is
// the whole per-score bookkeeping -- a non-empty wavefront is computed over its planned span.  While R <= 64 the sweep keeps the
// emptiness of the last 64 scores in a register and reads no marker.
//
// The semi-global form (SG; include/pwalign.h, "Semi-global wavefront alignments") is the same sweep and the same
// codes walk with another geometry: penalties per pattern symbol with two extends (e for 'I', ed for 'D'), so five source wavefronts;
// every diagonal 0 .. m seeded at score 0; the span [max(-n, -khi(s)), m]; the end on the lowest diagonal that reaches row n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pwa {
namespace wfa {

constexpr int kWaves = 4;                       // pairs per 256-thread workgroup
constexpr int32_t kNull = -(1 << 30);           // no offset: stays negative under + 1, and every negative offset is trimmed
constexpr int32_t kEmpty = INT32_MIN;           // first M cell of a skipped wavefront
constexpr uint32_t kNotFound = 0xffffffffu;     // penalty of a pair whose sweep reached P_max without ending
constexpr uint32_t kPad = 16;                   // zero bytes behind the sequence blob: an 8-byte extend load never leaves it

struct Pen {
    uint32_t x, o, e;   // reduced penalties of a mismatch, a gap open, a gap extend (SG: of an 'I' run)
    uint32_t ed;        // SG: the extend of a 'D' run; the global form never reads it
};

struct Pair {            // one pair of a range (host-built), in launch order: longest plan first
    uint64_t pat, txt;   // blob offsets of the pattern (i) and the text (j)
    uint64_t ws;         // first int32 of its wavefront workspace
    uint64_t ops;        // first byte of its op region in the range's op buffer (alignment form)
    uint32_t n, m;
    uint32_t p_max;      // the sweep's last score
    uint32_t out;        // its place in the range's result arrays
};

struct Span {
    int32_t lo, hi;
};

// The extend that widens the span: the only one (global), the 'D' run's (SG: 'I' runs start on diagonals that are live from score 0)
template <bool SG>
__host__ __device__ inline uint32_t span_e(const Pen& p) {
    return SG ? p.ed : p.e;
}

template <bool SG = false>
__host__ __device__ inline uint32_t khi(uint32_t s, const Pen& p) {
    const uint32_t e = span_e<SG>(p);
    return s < p.o + e ? 0u : (s - p.o) / e;
}

template <bool SG = false>
__host__ __device__ inline Span span_of(uint32_t s, uint32_t n, uint32_t m, const Pen& p) {
    const uint32_t h = khi<SG>(s, p);
    return Span{-(int32_t)(n < h ? n : h), (int32_t)(SG || m < h ? m : h)};
}

__host__ __device__ inline uint64_t tri(uint64_t c, uint64_t K) {   // sum of min(c, q) over q = 1 .. K
    return K <= c ? K * (K + 1) / 2 : c * (c + 1) / 2 + (K - c) * c;
}

// Cells of the wavefronts 0 .. s - 1: sum of 1 + min(n, khi) + min(m, khi).  khi is q on the e scores from o + q e on.
// SG: sum of m + 1 + min(n, khi) -- the m-side triangle gives way to (m + 1) s
template <bool SG = false>
__host__ __device__ inline uint64_t cum(uint32_t s, uint32_t n, uint32_t m, const Pen& p) {
    const uint32_t e = span_e<SG>(p);
    uint64_t r = SG ? (uint64_t)s * ((uint64_t)m + 1) : s;
    if (s > p.o + e) {
        const uint32_t t = s - p.o, Q = (t - 1) / e;   // Q = khi(s - 1) >= 1
        const uint64_t last = t - (uint64_t)Q * e;     // scores with khi = Q among them
        if (SG)
            r += (uint64_t)e * tri(n, Q - 1) + (uint64_t)(n < Q ? n : Q) * last;
        else
            r += (uint64_t)e * (tri(m, Q - 1) + tri(n, Q - 1)) + ((m < Q ? m : Q) + (uint64_t)(n < Q ? n : Q)) * last;
    }
    return r;
}

__device__ __forceinline__ int32_t trim(int32_t j, int32_t k, int32_t n, int32_t m) {
    const int32_t i = j - k;
    return (j >= 0 && j <= m && i >= 0 && i <= n) ? j : kNull;
}

__device__ __forceinline__ uint64_t load8(const uint8_t* p) {   // any byte address
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

struct SweepParams {
    const uint8_t* blob;    // the sequences, kPad zero bytes behind them
    const Pair* pairs;
    uint32_t n_pairs;
    Pen pen;
    int32_t* ws;
    uint32_t* penalty;      // [out]: P, or kNotFound.  SG: [2 out] with the end diagonal (int32, 0 when not found) at [2 out + 1]
};

// The int32 of a pair's ring in the score and the codes form: min(R, P_max + 1) slots of the widest span's three planes.  In the codes
// form the code plane (one byte per planned cell, wavefront s at byte cum(s)) lies right behind it in the pair's workspace.
template <bool SG>
__host__ __device__ inline uint32_t ring_depth(const Pen& p) {   // the furthest source wavefront, plus the one being written
    const uint32_t og = p.o + (SG && p.ed > p.e ? p.ed : p.e);
    return (p.x > og ? p.x : og) + 1;
}

template <bool SG = false>
__host__ __device__ inline uint64_t ring_words(uint32_t p_max, uint32_t n, uint32_t m, const Pen& p) {
    const uint64_t R = ring_depth<SG>(p);
    const Span sp = span_of<SG>(p_max, n, m, p);
    return 3 * (R < (uint64_t)p_max + 1 ? R : (uint64_t)p_max + 1) * (uint64_t)(sp.hi - sp.lo + 1);
}

// Code byte of a cell (codes form): all the backtrace ever asks of it
constexpr uint32_t kSrcX = 0, kSrcI = 1, kSrcD = 2, kSrcNone = 3;   // bits 0-1: where M came from (none: the cell is NULL, or s == 0)
constexpr uint32_t kOpenI = 4, kOpenD = 8;                           // bit 2: I opened (ml >= il); bit 3: D opened (mr >= dr)

// RING: the wavefronts live in the ring; CODES (with RING only): one code byte per valid cell goes to the pair's code plane as well;
// SG (with RING only): the semi-global form -- the D terms come from wavefronts of their own (s - o - ed, s - ed), score 0 seeds every
// diagonal 0 .. m, and the sweep ends on the lowest diagonal whose offset stands on row n
template <bool RING, bool CODES, bool SG = false>
__device__ __forceinline__ void sweep(const SweepParams& a) {
    static_assert(RING || !CODES, "the code plane goes with the ring");
    static_assert(RING || !SG, "the semi-global form keeps a ring");
    const uint32_t q = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    if (q >= a.n_pairs) return;   // whole waves
    const int lane = threadIdx.x & 63;
    const Pair P = a.pairs[q];
    const Pen pen = a.pen;
    const uint32_t n = P.n, m = P.m, oe = pen.o + pen.e;
    const uint32_t ed = SG ? pen.ed : pen.e, od = pen.o + ed;   // the D terms' sources: the I terms' own unless SG
    const uint8_t* const pat = a.blob + P.pat;
    const uint8_t* const txt = a.blob + P.txt;
    int32_t* const w = a.ws + P.ws;
    const uint32_t R = ring_depth<SG>(pen);
    const bool use_hist = R <= 64;
    const Span widest = span_of<SG>(P.p_max, n, m, pen);
    const uint64_t stride = 3ull * (uint32_t)(widest.hi - widest.lo + 1);   // of a ring slot
    const int32_t kend = (int32_t)m - (int32_t)n;
    uint8_t* codes = nullptr;
    if constexpr (CODES) codes = reinterpret_cast<uint8_t*>(w + ring_words<SG>(P.p_max, n, m, pen));

    uint64_t hist = 0;     // bit b: wavefront s - 1 - b is not empty
    uint32_t slot = 0;     // s mod R
    uint32_t found = kNotFound;
    int32_t found_k = 0;   // SG: the end diagonal
    // wavefront s - d
    auto wf = [&](uint32_t s, uint32_t d) -> int32_t* {
        if (RING) return w + (uint64_t)(slot >= d ? slot - d : slot + R - d) * stride;
        return w + 3 * cum(s - d, n, m, pen);
    };
    auto filled = [&](uint32_t s, uint32_t d) -> bool {
        if (d > s) return false;
        if (use_hist) return (hist >> (d - 1)) & 1;
        return *wf(s, d) != kEmpty;
    };
    for (uint32_t s = 0; s <= P.p_max; ++s) {
        if (!use_hist) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the markers below
        const bool ex = filled(s, pen.x), eo = filled(s, oe), ee = filled(s, pen.e);
        const bool eod = SG ? filled(s, od) : eo, eed = SG ? filled(s, ed) : ee;
        int32_t* const cur = wf(s, 0);
        if (s && !(ex || eo || ee || (SG && (eod || eed)))) {
            if (!(RING && use_hist) && lane == 0) cur[0] = kEmpty;
            hist <<= 1;
            slot = slot + 1 == R ? 0 : slot + 1;
            continue;
        }
        if (use_hist) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // earlier scores' stores before this score's loads
        const Span sp = span_of<SG>(s, n, m, pen);
        const uint32_t wd = (uint32_t)(sp.hi - sp.lo + 1);
        Span sx = {0, -1}, so = {0, -1}, se = {0, -1};
        const int32_t *bx = w, *bo = w, *be = w;
        uint32_t wde = 0;
        if (ex) {
            sx = span_of<SG>(s - pen.x, n, m, pen);
            bx = wf(s, pen.x);
        }
        if (eo) {
            so = span_of<SG>(s - oe, n, m, pen);
            bo = wf(s, oe);
        }
        if (ee) {
            se = span_of<SG>(s - pen.e, n, m, pen);
            be = wf(s, pen.e);
            wde = (uint32_t)(se.hi - se.lo + 1);
        }
        Span sod = so, sed = se;   // of the D terms
        const int32_t *bod = bo, *bed = be;
        uint32_t wdd = wde;
        if constexpr (SG) {
            sod = sed = Span{0, -1};
            bod = bed = w;
            wdd = 0;
            if (eod) {
                sod = span_of<SG>(s - od, n, m, pen);
                bod = wf(s, od);
            }
            if (eed) {
                sed = span_of<SG>(s - ed, n, m, pen);
                bed = wf(s, ed);
                wdd = (uint32_t)(sed.hi - sed.lo + 1);
            }
        }
        uint8_t* cd = nullptr;   // a skipped wavefront (above) writes no codes: no walk is ever led to one
        if constexpr (CODES) cd = codes + cum<SG>(s, n, m, pen);
        bool done = false;
        for (uint32_t c0 = 0; c0 < wd; c0 += 64) {
            const uint32_t c = c0 + lane;
            const bool valid = c < wd;
            const int32_t k = sp.lo + (int32_t)c;
            int32_t mx = kNull, ml = kNull, mr = kNull, il = kNull, dr = kNull;
            if (valid) {
                if (k >= sx.lo && k <= sx.hi) mx = bx[k - sx.lo];
                if (k - 1 >= so.lo && k - 1 <= so.hi) ml = bo[k - 1 - so.lo];
                if (k + 1 >= sod.lo && k + 1 <= sod.hi) mr = bod[k + 1 - sod.lo];
                if (k - 1 >= se.lo && k - 1 <= se.hi) il = be[wde + (uint32_t)(k - 1 - se.lo)];
                if (k + 1 >= sed.lo && k + 1 <= sed.hi) dr = bed[2 * wdd + (uint32_t)(k + 1 - sed.lo)];
            }
            const int32_t vi = trim((ml > il ? ml : il) + 1, k, (int32_t)n, (int32_t)m);
            const int32_t vd = trim(mr > dr ? mr : dr, k, (int32_t)n, (int32_t)m);
            const int32_t vx = trim(mx + 1, k, (int32_t)n, (int32_t)m);
            int32_t j = vx > vi ? vx : vi;
            j = j > vd ? j : vd;
            if constexpr (CODES) {   // the comparisons of wfa_walk_kernel, on the values it would read back
                const uint32_t src = (s == 0 || j < 0) ? kSrcNone : vx == j ? kSrcX : vi == j ? kSrcI : kSrcD;
                if (valid) cd[c] = (uint8_t)(src | (ml >= il ? kOpenI : 0u) | (mr >= dr ? kOpenD : 0u));
            }
            if (s == 0) j = SG ? k : 0;   // SG: a start at cell (0, k) on every diagonal 0 .. m, which is the whole span of score 0
            if (valid && j >= 0) {   // extend: 8 bytes per step, ended by the clamp to the two lengths
                const uint32_t i = (uint32_t)(j - k);
                const uint32_t rem = n - i < m - (uint32_t)j ? n - i : m - (uint32_t)j;
                const uint8_t* const pa = pat + i;
                const uint8_t* const pb = txt + j;
                uint32_t run = 0;
                while (run < rem) {
                    const uint64_t d = load8(pa + run) ^ load8(pb + run);
                    if (d) {
                        run += (uint32_t)__builtin_ctzll(d) >> 3;
                        break;
                    }
                    run += 8;
                }
                j += (int32_t)(run < rem ? run : rem);
            }
            if (valid) {
                cur[c] = j;
                cur[wd + c] = vi;
                cur[2 * wd + c] = vd;
            }
            if constexpr (SG) {   // the first chunk that stands on row n ends the sweep; its lowest such diagonal is the end
                const uint64_t hit = __ballot(valid && j >= 0 && j - k == (int32_t)n);
                if (hit) {
                    found_k = sp.lo + (int32_t)(c0 + (uint32_t)__builtin_ctzll(hit));
                    done = true;
                    break;
                }
            } else {
                done |= __ballot(valid && k == kend && j == (int32_t)m) != 0;
            }
        }
        hist = hist << 1 | 1;
        slot = slot + 1 == R ? 0 : slot + 1;
        if (done) {
            found = s;
            break;
        }
    }
    if constexpr (SG) {
        if (lane == 0) {
            a.penalty[2 * P.out] = found;
            a.penalty[2 * P.out + 1] = (uint32_t)found_k;
        }
    } else {
        if (lane == 0) a.penalty[P.out] = found;
    }
}

template <bool RING>
__global__ __launch_bounds__(256) void wfa_sweep_kernel(const SweepParams a) {
    sweep<RING, false>(a);
}

// The ring sweep of the codes form: wfa_sweep_kernel<true> plus one byte store per valid cell
__global__ __launch_bounds__(256) void wfa_codes_sweep_kernel(const SweepParams a) {
    sweep<true, true>(a);
}

// The semi-global form of the two: the score call's ring sweep, and the codes form's
__global__ __launch_bounds__(256) void wfa_sg_sweep_kernel(const SweepParams a) {
    sweep<true, false, true>(a);
}

__global__ __launch_bounds__(256) void wfa_sg_codes_sweep_kernel(const SweepParams a) {
    sweep<true, true, true>(a);
}

struct WalkParams {
    const Pair* pairs;
    uint32_t n_pairs;
    Pen pen;
    const int32_t* ws;
    const uint32_t* penalty;   // [out] of the sweep
    uint8_t* ops;
    uint32_t* n_ops;           // [out]
    uint32_t* fault;           // one word: set when a walk met a wavefront it cannot follow
};

// The backtrace over the stored wavefronts of the alignment form.  Every value it reads sits at a wave-uniform address, so the wave
// walks as one; its lanes share the writing of an 'M' run.
__global__ __launch_bounds__(256) void wfa_walk_kernel(const WalkParams a) {
    const uint32_t q = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    if (q >= a.n_pairs) return;   // whole waves
    const uint32_t lane = threadIdx.x & 63;
    const Pair P = a.pairs[q];
    const Pen pen = a.pen;
    const uint32_t n = P.n, m = P.m, oe = pen.o + pen.e;
    const int32_t* const w = a.ws + P.ws;
    uint8_t* const ops = a.ops + P.ops;
    const uint32_t cap = n + m;
    const uint32_t pnl = a.penalty[P.out];
    if (pnl == kNotFound) {
        if (lane == 0) a.n_ops[P.out] = 0;
        return;
    }
    // which: 0 M, 1 I, 2 D of wavefront s at diagonal k; kNull outside the sweep, outside the span, on a skipped wavefront
    auto get = [&](int64_t s, uint32_t which, int32_t k) -> int32_t {
        if (s < 0) return kNull;
        const Span sp = span_of((uint32_t)s, n, m, pen);
        if (k < sp.lo || k > sp.hi) return kNull;
        const int32_t* const b = w + 3 * cum((uint32_t)s, n, m, pen);
        if (b[0] == kEmpty) return kNull;
        return b[which * (uint32_t)(sp.hi - sp.lo + 1) + (uint32_t)(k - sp.lo)];
    };
    uint32_t cnt = 0;
    bool fault = false, finished = false;
    auto put_m = [&](uint32_t len) {
        if (len > cap - cnt) {
            fault = true;
            return;
        }
        for (uint32_t c = lane; c < len; c += 64) ops[cnt + c] = 'M';
        cnt += len;
    };
    int64_t s = pnl;
    int32_t k = (int32_t)m - (int32_t)n, j = (int32_t)m;
    int st = 0;   // 0: M, 1: I, 2: D
    for (uint64_t it = 0; it <= 2ull * cap + 2 && !fault; ++it) {
        if (st == 0) {
            if (s == 0) {
                if (k != 0 || j < 0) break;
                put_m((uint32_t)j);
                finished = !fault;
                break;
            }
            const int32_t vx = trim(get(s - pen.x, 0, k) + 1, k, (int32_t)n, (int32_t)m);
            const int32_t vi = get(s, 1, k), vd = get(s, 2, k);
            int32_t v = vx > vi ? vx : vi;
            v = v > vd ? v : vd;
            if (v < 0 || v > j) {
                fault = true;
                break;
            }
            put_m((uint32_t)(j - v) + (vx == v ? 1u : 0u));   // ties: mismatch >= I >= D
            if (vx == v) {
                s -= pen.x;
                j = v - 1;
            } else {
                st = vi == v ? 1 : 2;
                j = v;
            }
        } else {
            if (cnt >= cap) {   // cannot happen (every op moves i or j): never spin on the GPU
                fault = true;
                break;
            }
            const bool ins = st == 1;
            const int32_t ks = ins ? k - 1 : k + 1;
            if (lane == 0) ops[cnt] = ins ? 'I' : 'D';
            ++cnt;
            const int32_t vm = get(s - oe, 0, ks), vg = get(s - pen.e, (uint32_t)st, ks);
            if (vm < 0 && vg < 0) {
                fault = true;
                break;
            }
            if (vm >= vg) {   // a tie opens
                s -= oe;
                st = 0;
            } else {
                s -= pen.e;
            }
            k = ks;
            if (ins) --j;
        }
    }
    if (lane == 0) {
        a.n_ops[P.out] = finished ? cnt : 0u;
        if (!finished) *a.fault = 1u;
    }
}

struct CodesWalkParams {
    const uint8_t* blob;       // the sequences: pass B extends over them again
    const Pair* pairs;
    uint32_t n_pairs;
    Pen pen;
    const int32_t* ws;         // per pair: the ring (not read here), then the code plane
    const uint32_t* penalty;   // [out] of the sweep
    uint8_t* ops;
    uint32_t* n_ops;           // [out]
    uint32_t* fault;           // one word: set when a walk met a code it cannot follow
    uint32_t* cells;           // SG, [4 out]: the end cell (i, j), then the start cell; zeros for a pair without an op list
};

constexpr uint32_t kToM = 0x80;   // in an edit record: the walk is in state M after it, so a match run may stand there

// The backtrace of the codes form, in two passes, every address wave-uniform (the values are held in scalar registers).
// Pass A walks the codes from (P, m - n, state M) down to score 0 and leaves one record per edit ('M' for a mismatch, 'I', 'D', with
// kToM) at the front of the pair's op region, in traceback order.  Pass B replays them from (0, 0), last record first: a greedy
// extend over the lanes wherever the walk was in state M, then the edit, and writes the op list from its end downwards.  With t + 1
// records unread and `wr` slots unwritten, wr - (t + 1) is the number of matches still to come, so a write never lands on an
// unread record; record t is read before the op that may take its place.
// SG: pass A starts on the end diagonal the sweep left next to the penalty, reads the codes of an I and of a D at their own two
// source scores, and accepts any diagonal 0 .. m at score 0 -- the start cell (0, k), from which pass B replays to (n, n + k_end).
template <bool SG>
__device__ __forceinline__ void codes_walk(const CodesWalkParams& a) {
    const uint32_t q = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    if (q >= a.n_pairs) return;   // whole waves
    const uint32_t lane = threadIdx.x & 63;
    const Pair P = a.pairs[q];
    const Pen pen = a.pen;
    const uint32_t n = P.n, m = P.m, oe = pen.o + pen.e;
    const uint32_t ed = SG ? pen.ed : pen.e, od = pen.o + ed;
    const uint8_t* const pat = a.blob + P.pat;
    const uint8_t* const txt = a.blob + P.txt;
    const uint8_t* const codes = reinterpret_cast<const uint8_t*>(a.ws + P.ws + ring_words<SG>(P.p_max, n, m, pen));
    uint8_t* const ops = a.ops + P.ops;
    const uint32_t cap = n + m;
    const uint32_t pnl = __builtin_amdgcn_readfirstlane(a.penalty[SG ? 2 * P.out : P.out]);
    // where the alignment ends and starts on the text: (n, m) and (0, 0) unless SG
    int32_t k_end = (int32_t)m - (int32_t)n, k_start = 0;
    if constexpr (SG) k_end = __builtin_amdgcn_readfirstlane((int32_t)a.penalty[2 * P.out + 1]);
    auto cells_out = [&](bool ok) {
        if constexpr (SG) {
            if (lane < 4) a.cells[4 * (uint64_t)P.out + lane] = !ok ? 0u : lane == 0 ? n : lane == 1 ? n + (uint32_t)k_end : lane == 2 ? 0u : (uint32_t)k_start;
        }
    };
    if (pnl == kNotFound) {
        if (lane == 0) a.n_ops[P.out] = 0;
        cells_out(false);
        return;
    }
    // ---- pass A
    uint32_t E = 0, ui = 0, uj = 0;   // records; pattern and text symbols their edits consume
    bool fault = false, ended = false;
    int64_t s = pnl;
    int32_t k = k_end;
    uint32_t st = 0;   // 0: M, 1: I, 2: D
    for (uint64_t it = 0; it <= 2ull * cap + 2; ++it) {
        if (st == 0 && s == 0) {
            ended = SG ? k >= 0 && k <= (int32_t)m : k == 0;
            k_start = k;
            break;
        }
        if (s < 0 || E >= cap) break;   // (every record moves i or j: more than n + m of them cannot be)
        const Span sp = span_of<SG>((uint32_t)s, n, m, pen);
        if (k < sp.lo || k > sp.hi) break;
        const uint32_t code = __builtin_amdgcn_readfirstlane(codes[cum<SG>((uint32_t)s, n, m, pen) + (uint32_t)(k - sp.lo)]);
        if (st == 0) {
            const uint32_t src = code & 3u;
            if (src == kSrcNone) break;
            if (src == kSrcX) {
                if (lane == 0) ops[E] = (uint8_t)('M' | kToM);
                ++E;
                ++ui;
                ++uj;
                s -= pen.x;
            } else {
                st = src;   // kSrcI, kSrcD: the same cell in state I, D
            }
        } else {
            const bool ins = st == 1;
            const bool opened = (code & (ins ? kOpenI : kOpenD)) != 0;
            if (lane == 0) ops[E] = (uint8_t)((ins ? 'I' : 'D') | (opened ? kToM : 0u));
            ++E;
            if (ins) {
                ++uj;
                --k;
            } else {
                ++ui;
                ++k;
            }
            s -= ins ? (opened ? oe : pen.e) : (opened ? od : ed);
            if (opened) st = 0;
        }
    }
    // the text between the two cells: uj symbols under the edits and one per match, of which there are n - ui
    if constexpr (SG)
        fault = !ended || ui > n || (int64_t)n + k_end < 0 || (int64_t)n + k_end > (int64_t)m || (int64_t)k_start + uj + (n - ui) != (int64_t)n + k_end;
    else
        fault = !ended || ui > n || uj > m || n - ui != m - uj;
    const uint32_t cnt = fault ? 0u : E + (n - ui);   // <= n + m: E - ui is the number of 'I', at most uj <= m
    fault = fault || cnt > cap;
    // ---- pass B
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // lane 0's records before every lane's loads of them
    uint32_t i = 0, j = SG && !fault ? (uint32_t)k_start : 0u, wr = cnt;   // ops[0 .. wr) not written yet
    // the match run from (i, j), at most `room` long, into the slots below wr
    auto extend = [&](uint32_t room) {
        const uint32_t rem = n - i < m - j ? n - i : m - j;
        uint32_t run = rem;
        for (uint32_t base = 0; base < rem; base += 512) {
            const uint32_t off = base + 8 * lane;
            uint32_t pos = off;   // a lane beyond the clamp ends the run where it stands
            bool stop = true;
            if (off < rem) {
                const uint64_t d = load8(pat + i + off) ^ load8(txt + j + off);
                stop = d != 0;
                if (stop) pos += (uint32_t)__builtin_ctzll(d) >> 3;
            }
            const uint64_t b = __ballot(stop);
            if (b) {
                run = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)__builtin_ctzll(b));
                break;
            }
        }
        run = run < rem ? run : rem;
        if (run > room) {
            fault = true;
            return;
        }
        for (uint32_t c = lane; c < run; c += 64) ops[wr - run + c] = 'M';
        wr -= run;
        i += run;
        j += run;
    };
    for (uint32_t t = E; !fault && t-- > 0;) {
        const uint32_t rec = __builtin_amdgcn_readfirstlane(ops[t]);
        if (rec & kToM) extend(wr - (t + 1));
        if (fault) break;
        const uint32_t op = rec & 0x7fu;
        i += op != 'I';
        j += op != 'D';
        if (lane == 0) ops[wr - 1] = (uint8_t)op;   // wr - 1 >= t
        --wr;
    }
    if (!fault) extend(wr);
    const bool finished = !fault && wr == 0 && i == n && j == (SG ? n + (uint32_t)k_end : m);
    if (lane == 0) {
        a.n_ops[P.out] = finished ? cnt : 0u;
        if (!finished) *a.fault = 1u;
    }
    cells_out(finished);
}

__global__ __launch_bounds__(256) void wfa_codes_walk_kernel(const CodesWalkParams a) {
    codes_walk<false>(a);
}

__global__ __launch_bounds__(256) void wfa_sg_codes_walk_kernel(const CodesWalkParams a) {
    codes_walk<true>(a);
}

}  // namespace wfa
}  // namespace pwa
