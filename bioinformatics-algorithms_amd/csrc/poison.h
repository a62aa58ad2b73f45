// poison.h -- PWA_POISON=<byte> (include/pwalign.h, "Environment switches"): a test mode in which every buffer the context
// hands to a call reads as that byte until the call first writes to it.  Every acquisition site of the host units -- a fresh or regrown
// allocation, a buffer from the free list, the parked hand-off buffer, a retained slot reused as it is, a page-locked staging buffer -- calls
// poison_device / poison_host on the buffer's whole capacity; with the switch unset that is one branch.  No kernel knows about it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#pragma GCC visibility push(hidden)
namespace pwa {
struct Poison {
    int byte = -1;                      // 0 .. 255, -1: unset
    int device = 0;                     // the owning context's HIP device: the fill makes it current itself
    uint64_t buffers = 0, bytes = 0;    // running totals of what was filled (pwa_ctx_poison_stats)
};
// The switch's value: nullptr -> -1 (unset); decimal or 0x.. of 0 .. 255 -> the byte; anything else -> -2 (pwa_ctx_create fails)
int parse_poison(const char* s);
// `cap` bytes at device pointer p := the byte, blocking: a device synchronise, a hipMemset, a device synchronise -- the fill is ordered
// after everything enqueued before the acquisition and before everything enqueued after it, on whatever stream of po->device, which
// the fill makes the calling thread's current device first (both calls act on the current device; every entry point has set it to
// the context's before its first acquisition, and the fill does not rely on that).  Unset: no HIP call
hipError_t poison_device(Poison* po, void* p, size_t cap);
// ... and of host (page-locked) memory
void poison_host(Poison* po, void* p, size_t cap);
}  // namespace pwa
#pragma GCC visibility pop
