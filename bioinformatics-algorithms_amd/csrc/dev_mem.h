// dev_mem.h -- pwa::DevMem, the one owner of the device memory a context keeps between calls, and the alignment side's one path to
// hipMalloc ("The allocation rule").  A context holds one (pwa_ctx::mem).  Three kinds of memory, one allocation function:
//   slots      work buffers of the pwa_align* calls, one launch at a time per context: grow-only, at most kBandCacheMax each, handed out
//              as a Lease (workspace).  hipMalloc of several GiB is sometimes fast (0.3 ms) and sometimes not (0.2 - 1.5 s) depending on
//              the state of the device's memory, and each hipMalloc / hipFree also synchronises the device: a caller that aligns batch
//              after batch pays them once.
//   HAND       the strip hand-off workspace of the last destroyed batch object (5.2 GB for C3), parked for the next one (park_hand / take_hand).
//   free list  the other device buffers of destroyed batch objects (keep / buffer): a steady stream of batches -- the runs of a one-shot
//              call over a large list, a caller that builds batch after batch -- costs no hipMalloc and, more to the point, no hipFree:
//              hipFree waits for ALL work on the device, i.e. for the kernels of the batch that is still running, and with it the
//              overlap of preparing run k + 1 with computing run k would be gone (scores_in_arena_chunks).
// Policy only, inline host code over an injectable allocator: pwa_selftest_host drives it with a counting fake on machines without a GPU.
// PWA_POISON is not its business: the wrappers in pwalign_ctx.hip (workspace, DevBuf, PairLaunch::take) fill what it hands out.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)
namespace pwa {

constexpr size_t kBandCacheMax = 64ull << 30;   // most bytes a slot keeps (288 GB of HBM per GPU: a 4096-pair batch with both bands is 33 GB)

class DevMem;

// What a call holds of DevMem's memory: a slot's buffer (the slot stays the context's), or a buffer of its own that goes back with the
// lease -- to hipFree (a request beyond kBandCacheMax, a one-call buffer) or to the free list (a batch object's).  Move-only.
class Lease {
  public:
    Lease() = default;
    Lease(Lease&& o) noexcept { *this = std::move(o); }
    Lease& operator=(Lease&& o) noexcept {
        if (this != &o) {
            release();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
            own_ = std::exchange(o.own_, nullptr);
            keep_ = o.keep_;
        }
        return *this;
    }
    ~Lease() { release(); }
    inline void release();
    void* get() const { return p_; }
    size_t cap() const { return cap_; }   // the whole capacity behind get(): what PWA_POISON fills
    template <class T> T* as() const { return static_cast<T*>(p_); }

  private:
    friend class DevMem;
    Lease(void* p, size_t cap, DevMem* own, bool keep) : p_(p), cap_(cap), own_(own), keep_(keep) {}
    void* p_ = nullptr;
    size_t cap_ = 0;
    DevMem* own_ = nullptr;   // set: p_ is the lease's own
    bool keep_ = false;       // ... and goes to the free list
};

class DevMem {
  public:
    typedef hipError_t (*AllocFn)(void**, size_t);
    typedef hipError_t (*FreeFn)(void*);
    // sequence arena, op lists, results, pair descriptors, task list, hand-off rows, progress words, per-stripe bests, queue;
    // pwa_align_batch_cigar's strings and their pair list / lengths / scan partials; traceback band and int32 score band; the parked hand-off buffer
    enum Slot { ARENA, OPS, RES, DESC, TASKS, ROWS, PROGRESS, BEST, QUEUE, STR, STR_AUX, BAND, SBAND, HAND, SLOT_N };
    static constexpr size_t kListMaxBytes = 24ull << 30, kListMaxCount = 64;

    explicit DevMem(AllocFn a = hipMalloc, FreeFn f = hipFree) : alloc_(a), free_(f) {}
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() {
        drop_idle();
        for (Buf& s : slot_) drop(s.p);
    }

    // The only caller of hipMalloc.  Out of memory: everything idle -- the free list and the parked hand-off buffer -- goes back to the
    // device, the runtime's last error is cleared, and the request is tried once more.  The other slots are never given up: the call
    // in flight may hold a lease on any of them.
    hipError_t raw_alloc(void** p, size_t n) {
        hipError_t e = alloc_(p, n);
        if (e != hipSuccess) {
            drop_idle();
            (void)hipGetLastError();
            e = alloc_(p, n);
        }
        if (e != hipSuccess) *p = nullptr;
        return e;
    }

    // `bytes` of slot s: reused as it is when big enough, regrown to exactly `bytes` otherwise; out.cap() is the whole slot.  A request
    // beyond kBandCacheMax leaves the slot alone and is served by a buffer that is freed with the lease.
    hipError_t workspace(Slot s, size_t bytes, Lease& out) {
        if (bytes > kBandCacheMax) return lease(bytes, false, out);
        out.release();
        Buf& b = slot_[s];
        if (b.bytes < bytes) {
            drop(b.p);
            b = Buf{};
            const hipError_t e = raw_alloc(&b.p, bytes);
            if (e != hipSuccess) return e;
            b.bytes = bytes;
        }
        out = Lease(b.p, b.bytes, nullptr, false);
        return hipSuccess;
    }

    // A buffer of at least n bytes that the caller owns.  pooled: the best fit of the free list -- at least n, at most 2 n + 1 MiB (a
    // 5 GB block is not spent on a 1 KB request), the smallest such -- before a fresh one of exactly n.
    hipError_t buffer(size_t n, bool pooled, void** p, size_t* bytes) {
        size_t best = list_.size();
        for (size_t i = 0; pooled && i < list_.size(); ++i) {
            const size_t have = list_[i].second;
            if (have >= n && have <= 2 * n + (1u << 20) && (best == list_.size() || have < list_[best].second)) best = i;
        }
        if (best < list_.size()) {
            *p = list_[best].first;
            *bytes = list_[best].second;
            list_bytes_ -= *bytes;
            list_.erase(list_.begin() + (long)best);
            return hipSuccess;
        }
        const hipError_t e = raw_alloc(p, n);
        *bytes = e == hipSuccess ? n : 0;
        return e;
    }
    // ... as a lease: back to the free list (pooled) or to hipFree with it
    hipError_t lease(size_t n, bool pooled, Lease& out) {
        out.release();
        void* p = nullptr;
        size_t bytes = 0;
        const hipError_t e = buffer(n, pooled, &p, &bytes);
        if (e == hipSuccess) out = Lease(p, bytes, this, pooled);
        return e;
    }
    // A buffer nothing on the device uses any more: onto the free list, or to hipFree where the list's caps refuse it
    void keep(void* p, size_t bytes) {
        if (p && list_.size() < kListMaxCount && list_bytes_ + bytes <= kListMaxBytes) {
            list_.emplace_back(p, bytes);
            list_bytes_ += bytes;
        } else {
            drop(p);
        }
    }
    void drop(void* p) {
        if (p) (void)free_(p);
    }

    // The parked hand-off buffer if it holds at least n bytes (it then is the caller's); a smaller one stays parked
    bool take_hand(size_t n, void** p, size_t* bytes) {
        Buf& h = slot_[HAND];
        if (!h.p || h.bytes < n) return false;
        *p = h.p;
        *bytes = h.bytes;
        h = Buf{};
        return true;
    }
    // Parks (p, bytes) if it is the larger one and within the slot cap: the next batch of the same shape then skips a multi-GB
    // hipMalloc.  The buffer this displaces, or the refused one, goes the way of every other buffer of a destroyed batch (keep).
    void park_hand(void* p, size_t bytes) {
        Buf& h = slot_[HAND];
        if (p && bytes > h.bytes && bytes <= kBandCacheMax) {
            std::swap(h.p, p);
            std::swap(h.bytes, bytes);
        }
        keep(p, bytes);
    }

  private:
    struct Buf {
        void* p = nullptr;
        size_t bytes = 0;
    };
    void drop_idle() {
        for (auto& f : list_) drop(f.first);
        list_.clear();
        list_bytes_ = 0;
        drop(slot_[HAND].p);
        slot_[HAND] = Buf{};
    }
    AllocFn alloc_;
    FreeFn free_;
    Buf slot_[SLOT_N];
    std::vector<std::pair<void*, size_t>> list_;
    size_t list_bytes_ = 0;
};

inline void Lease::release() {
    if (own_ && keep_) own_->keep(p_, cap_);
    else if (own_) own_->drop(p_);
    p_ = nullptr;
    cap_ = 0;
    own_ = nullptr;
}

}  // namespace pwa
#pragma GCC visibility pop
