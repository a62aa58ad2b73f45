// cigar.hip.h -- CIGAR and MD:Z strings of a range of walked pairs, built where the op lists sit (gfx950 / MI355X).
//
// Replaces, per pair of pwa_align_batch_cigar, the host formatter host/postprocess.cpp (pwa_format_alignment) over
// prepareCigarString (hw2.cpp:59-78) and prepareMDZString (80-116).  DESIGN.md §3.9.
//
// One wave per pair steps over the op list in FORWARD order (memory order reversed: the walk writes end -> start), 64
// columns per sub-chunk, lane l = column c0 + l, kSub sub-chunks' loads issued together.  Ballots give, per column:
//   * the pattern / text indices (start cell + the number of M|D, resp. M|I, columns before it);
//   * CIGAR: a token per run, emitted by the column that OPENS the next run (so nothing looks ahead), the last run's
//     token after the loop;
//   * MD:Z: a token at each mismatching M (count + text symbol), at the first D of a D run (count + '^' + pattern
//     symbol), one byte at every further D of the run; the count is the number of equal M columns since the last
//     mismatch or D ('I' columns neither count nor reset); the final count after the loop.
// A wave inclusive scan of the per-lane byte counts (both strings packed into one word) places every token.  What a
// sub-chunk carries into the next (open run and its start, op of the previous column, match count, i, j, the two
// output cursors) is wave-uniform.  The count pass (WRITE = false) and the write pass (WRITE = true) are the same code:
// the write pass stores exactly the bytes the count pass counted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pair_fill.hip.h"

namespace pwa {

struct CigarPair {     // one pair of a range (host-built)
    uint64_t pat, txt;  // arena offsets of the pattern (rows) and the text (columns)
    uint64_t ops;       // offset of its op list in the range's op buffer (traceback order)
    uint32_t n, m;
};

struct CigarParams {
    const uint8_t* arena;     // coded (<= 7 symbols: codes 0..6) or raw bytes
    const uint8_t* ops;
    const PairResult* res;    // n_ops, start cell, overflow of every pair of the range (index = pair in the range)
    const CigarPair* pairs;
    uint32_t* len;            // count pass: cigar lengths at [0, nc), 0 at nc, MD:Z lengths at [nc + 1, 2 nc + 1), 0 at 2 nc + 1;
                              // write pass: the same array after an exclusive scan (= where each string starts in `out`)
    uint8_t* out;             // the range's strings: every CIGAR, then every MD:Z
    uint64_t decode;          // coded arena: byte c = the symbol of code c
    uint32_t nc;
    int coded, local;
    int semi;                 // semi-global (PWA_MODE_SG): a pair with an empty side is all D (m = 0) or nothing (n = 0)
};

namespace cigar {

constexpr int kWaves = 4;   // pairs per 256-thread workgroup
constexpr int kSub = 8;     // 64-column sub-chunks per load batch

__device__ __forceinline__ uint32_t n_digits(uint32_t v) {
    uint32_t d = 1;
    for (uint64_t p = 10; v >= p; p *= 10) ++d;   // v < 2^32: at most 10 digits
    return d;
}

__device__ __forceinline__ uint8_t* put_count(uint8_t* o, uint32_t v, uint32_t nd) {
    for (uint32_t k = nd; k > 0; --k) {
        o[k - 1] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return o + nd;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {   // set bits of mask in lanes < this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ uint64_t above(int lane) {   // lanes > lane
    return lane >= 63 ? 0ull : ~0ull << (lane + 1);
}

}  // namespace cigar

template <bool WRITE>
__global__ __launch_bounds__(256) void cigar_kernel(const CigarParams a) {
    using namespace cigar;
    const uint32_t q = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (q >= a.nc) return;   // whole waves
    const int lane = threadIdx.x & 63;
    const uint64_t lt = (1ull << lane) - 1;
    const CigarPair P = a.pairs[q];
    const PairResult R = a.res[q];
    const bool one_side = !(P.n && P.m);   // NW: the boundary walk (all D or all I), SW: nothing, SG: column 0 (all D); the walk never saw the pair
    uint32_t n_ops, i, j;
    if (one_side) {
        n_ops = a.local ? 0u : a.semi ? P.n : P.n + P.m;
        i = j = 0;
    } else {
        n_ops = (R.overflow || R.n_ops > P.n + P.m) ? 0u : R.n_ops;   // an overflowed walk: nothing read, the host fails the call
        i = R.start_i;
        j = R.start_j;
    }
    const uint8_t side_op = P.n ? 'D' : 'I';
    const uint8_t* const ops_end = a.ops + P.ops + n_ops - 1;   // column c is ops_end[-c]
    const uint8_t* const pat = a.arena + P.pat;
    const uint8_t* const txt = a.arena + P.txt;
    auto decode = [&](uint32_t s) -> uint8_t { return a.coded ? (uint8_t)(a.decode >> (8 * (s & 7))) : (uint8_t)s; };

    uint32_t cur_c = 0, cur_m = 0;   // bytes written so far
    uint8_t* out_c = nullptr;
    uint8_t* out_m = nullptr;
    if (WRITE) {
        out_c = a.out + a.len[q];
        out_m = a.out + a.len[a.nc + 1 + q];
    }
    uint32_t prev_op = 0, run_start = 0, matches = 0;
    for (uint32_t c0 = 0; c0 < n_ops; c0 += 64 * kSub) {
        // ---- loads: the ops of kSub sub-chunks, then the symbols under them
        uint32_t op[kSub], sa[kSub], sb[kSub];
#pragma unroll
        for (int s = 0; s < kSub; ++s) {
            const uint32_t c = c0 + 64 * s + lane;
            op[s] = c < n_ops ? (one_side ? side_op : ops_end[-(int64_t)c]) : 0u;
        }
#pragma unroll
        for (int s = 0; s < kSub; ++s) {
            const uint64_t mM = __ballot(op[s] == 'M'), mD = __ballot(op[s] == 'D'), mI = __ballot(op[s] == 'I');
            const uint32_t il = i + lanes_below(mM | mD), jl = j + lanes_below(mM | mI);
            sa[s] = (op[s] == 'M' || op[s] == 'D') && il < P.n ? pat[il] : 0u;
            sb[s] = op[s] == 'M' && jl < P.m ? txt[jl] : 0u;
            i += (uint32_t)__popcll(mM | mD);
            j += (uint32_t)__popcll(mM | mI);
        }
        // ---- tokens, sub-chunk by sub-chunk
#pragma unroll
        for (int s = 0; s < kSub; ++s) {
            const uint32_t cs = c0 + 64 * s;
            if (cs >= n_ops) break;
            const uint32_t c = cs + lane;
            const bool valid = c < n_ops;
            const uint32_t o = op[s];
            const uint32_t up = __shfl_up(o, 1, 64);
            const uint32_t p = lane == 0 ? prev_op : up;   // op of column c - 1 (0 before column 0)
            // CIGAR: column c opens a run -> the token of the run that ended at c - 1
            const bool opens = valid && o != p;
            const uint64_t mS = __ballot(opens);
            const uint64_t sb_ = mS & lt;
            const uint32_t prev_start = sb_ ? cs + 63 - (uint32_t)__clzll(sb_) : run_start;
            const bool tok_c = opens && c > 0;
            const uint32_t run = c - prev_start;
            const uint32_t nd_c = tok_c ? n_digits(run) : 0u;
            const uint32_t bc = tok_c ? nd_c + 1 : 0u;
            // MD:Z
            const bool is_m = valid && o == 'M', is_d = valid && o == 'D';
            const bool eq = is_m && sa[s] == sb[s];
            const uint64_t mEq = __ballot(eq), mR = __ballot((is_m && !eq) || is_d);
            const uint64_t rb = mR & lt;
            uint32_t mb;   // matches before column c
            if (rb) {
                const int last = 63 - __clzll(rb);
                mb = (uint32_t)__popcll(mEq & lt & above(last));
            } else {
                mb = matches + (uint32_t)__popcll(mEq & lt);
            }
            const bool mis = is_m && !eq, d_open = is_d && p != 'D';
            const uint32_t nd_m = (mis || d_open) ? n_digits(mb) : 0u;
            const uint32_t bm = mis ? nd_m + 1 : d_open ? nd_m + 2 : is_d ? 1u : 0u;
            // places: one inclusive scan of both byte counts (each <= 12 per lane, <= 768 per sub-chunk)
            const uint32_t v = bc | bm << 16;
            uint32_t x = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d, 64);
                if (lane >= d) x += y;
            }
            const uint32_t excl = x - v, tot = __shfl(x, 63, 64);
            if (WRITE) {
                if (bc) {
                    uint8_t* w = put_count(out_c + cur_c + (excl & 0xffffu), run, nd_c);
                    *w = (uint8_t)p;
                }
                if (bm) {
                    uint8_t* w = out_m + cur_m + (excl >> 16);
                    if (mis) {
                        w = put_count(w, mb, nd_m);
                        *w = decode(sb[s]);
                    } else if (d_open) {
                        w = put_count(w, mb, nd_m);
                        w[0] = '^';
                        w[1] = decode(sa[s]);
                    } else {
                        *w = decode(sa[s]);
                    }
                }
            }
            cur_c += tot & 0xffffu;
            cur_m += tot >> 16;
            // carry
            if (mS) run_start = cs + 63 - (uint32_t)__clzll(mS);
            if (mR) {
                const int last = 63 - __clzll(mR);
                matches = (uint32_t)__popcll(mEq & above(last));
            } else {
                matches += (uint32_t)__popcll(mEq);
            }
            const uint32_t last_lane = n_ops - cs >= 64 ? 63u : n_ops - cs - 1;
            prev_op = __shfl(o, (int)last_lane, 64);
        }
    }
    // the last run's CIGAR token and the final MD:Z count
    const uint32_t last_run = n_ops - run_start;
    const uint32_t nd_c = n_ops ? n_digits(last_run) : 0u, nd_m = n_digits(matches);
    if (lane == 0) {
        if (WRITE) {
            if (n_ops) {
                uint8_t* w = put_count(out_c + cur_c, last_run, nd_c);
                *w = (uint8_t)prev_op;
            }
            put_count(out_m + cur_m, matches, nd_m);
        } else {
            a.len[q] = cur_c + (n_ops ? nd_c + 1 : 0u);
            a.len[a.nc + 1 + q] = cur_m + nd_m;
            if (q == 0) {
                a.len[a.nc] = 0;
                a.len[2 * a.nc + 1] = 0;
            }
        }
    }
}

}  // namespace pwa
