// side_unit.h -- the host kit of the units that stay away from pwalign_internal.h (sufarr_kernels.hip, approx_kernels.hip,
// wfa_kernels.hip, chain_kernels.hip): what each needs of a pwa_ctx, an owned device allocation, timing events, the error path from a HIP call to the
// entry point's return code, and the cutting of a list into runs under a budget.  Nothing here is exported.  DESIGN.md §3.21 ("The side units' host kit").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/pwalign.h"
#include "poison.h"

#pragma GCC visibility push(hidden)
namespace pwa {
// What every side unit reads of a context; a unit's own view (sufarr_ctx.h, approx_ctx.h, wfa_ctx.h, chain_ctx.h) adds its knobs and stats
struct UnitCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool debug = false;              // PWA_DEBUG
    std::string* err = nullptr;      // the context's last-error text
    Poison* poison = nullptr;        // the context's PWA_POISON state: every device allocation of a unit goes through poison_device
};
UnitCtx unit_ctx(pwa_ctx* c);   // pwalign_ctx.hip

struct Dev {   // one device allocation, freed with its owner
    void* p = nullptr;
    size_t cap = 0;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) (void)hipFree(p); }
    hipError_t alloc(Poison* po, size_t bytes) {   // po: the context's PWA_POISON state (UnitCtx::poison)
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = std::max<size_t>(bytes, 16);
        const hipError_t e = hipMalloc(&p, cap);
        return e == hipSuccess ? poison_device(po, p, cap) : e;
    }
    hipError_t again(Poison* po) { return poison_device(po, p, cap); }   // the same buffer handed out once more
    template <class T> T* as() const { return static_cast<T*>(p); }
};

template <int N>
struct Events {   // N timing events, destroyed with their owner
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    ~Events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    hipError_t create() {
        for (hipEvent_t& x : e)
            if (const hipError_t rc = hipEventCreate(&x)) return rc;
        return hipSuccess;
    }
};

struct Fail {   // an error on the way: the code and what to say about it
    int code;
    std::string what;
};
inline void check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Fail{e == hipErrorOutOfMemory ? PWA_E_NOMEM : PWA_E_HIP, std::string(what) + ": " + hipGetErrorString(e)};
}
#define UNIT_CHECK(call) pwa::check((call), #call)

// The tail of every entry point: body() runs to its end, or a Fail becomes the context's error text and its code
template <class F>
int guarded(UnitCtx& v, F&& body) {
    try {
        body();
    } catch (const Fail& f) {
        *v.err = f.what;
        return f.code;
    } catch (const std::bad_alloc&) {
        return PWA_E_NOMEM;
    }
    return PWA_OK;
}

inline uint32_t blocks_for(size_t n, size_t per) { return (uint32_t)((n + per - 1) / per); }

// Items 0 .. n cut into runs of consecutive items: each run as long as its weights fit the budget, or one item that alone exceeds it
struct Run {
    uint64_t k0, k1, weight;
};
template <class W>
std::vector<Run> cut_runs(uint64_t n, uint64_t budget, W&& weight_of) {
    std::vector<Run> runs;
    for (uint64_t k0 = 0; k0 < n;) {
        Run r{k0, k0 + 1, weight_of(k0)};
        for (; r.k1 < n; ++r.k1) {
            const uint64_t w = weight_of(r.k1);
            if (r.weight + w > budget) break;
            r.weight += w;
        }
        runs.push_back(r);
        k0 = r.k1;
    }
    return runs;
}
}  // namespace pwa
#pragma GCC visibility pop
