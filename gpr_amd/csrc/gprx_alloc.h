// gprx_alloc.h — the one place libgprx allocates device memory (host code; included through
// gprx_internal.h).  Every hipMalloc, hipExtMallocWithFlags and hipMallocAsync of the library goes
// through dev_malloc / dev_malloc_async below (tests/test_poison_cpu.py keeps it that way), so
// GPRX_POISON reaches every buffer: the models' DevBufs, the sharded engine's DMem, the chained
// launches' counter and flag words, the tile engine's state, the stream-ordered partials and the
// caller's DeviceArray memory.
//
// GPRX_POISON (debugging; read once per process): a fresh allocation holds finite garbage (bytes
// 0x41: 12.1f, 2.3e6, the int 0x41414141), as reused memory does and a fresh hipMalloc usually
// does not, so a read of memory nothing has written shows in the results.  The byte stays 0x41: a
// NaN or all-ones fill would put -1 into a ticket or index word.  Unset, nothing below differs from
// the plain allocation call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>

namespace gprx {

constexpr int kPoisonByte = 0x41;

inline bool poison_on() {
    static const bool on = std::getenv("GPRX_POISON") != nullptr;
    return on;
}

// b bytes of device memory (fine: fine-grained, a mailbox other GPUs store into).  Poisoned: filled
// on the null stream and DRAINED -- the contexts' and the ranks' non-blocking streams do not wait
// for the null stream, so an undrained fill can land after the first kernel's stores into the new
// buffer.  The drain waits for every kernel on the device: never call this between the launches of
// kernels that wait for each other (the sharded engine's per-rank launches).
template <typename P>
inline hipError_t dev_malloc(P** p, size_t b, bool fine = false) {
    void* q = nullptr;
    hipError_t e = fine ? hipExtMallocWithFlags(&q, b, hipDeviceMallocFinegrained) : hipMalloc(&q, b);
    if (e == hipSuccess && poison_on()) {
        e = hipMemset(q, kPoisonByte, b);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void)hipFree(q);
            q = nullptr;
        }
    }
    *p = static_cast<P*>(q);
    return e;
}

// stream-ordered form (freed with hipFreeAsync on the same stream).  Poisoned: filled on that
// stream, ahead of whatever the caller enqueues next; nothing is synchronised.
template <typename P>
inline hipError_t dev_malloc_async(P** p, size_t b, hipStream_t s) {
    void* q = nullptr;
    hipError_t e = hipMallocAsync(&q, b, s);
    if (e == hipSuccess && poison_on()) e = hipMemsetAsync(q, kPoisonByte, b, s);
    *p = static_cast<P*>(q);
    return e;
}

}  // namespace gprx
