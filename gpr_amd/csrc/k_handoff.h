// k_handoff.h — the inter-workgroup hand-off shared by every chained kernel (gfx950).
//
// k_bsolve.hip, k_append.hip, k_dsolve.hip and the tile-dataflow factorisation (k_ptiles.hip)
// pass data from one running workgroup to another inside one launch.  The protocol, once
// (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility",
// "Valid forms" and the table under it):
//
// Producer.  Every handed-off byte is stored written through -- st_sc1 inside one device (the
//   {sc1 stores, sc1 loads} form, first row of the table), st_nc / `sc0 sc1` stores towards
//   another rank (the {sc0 sc1 stores and loads both sides} form) -- so no L2 write-back is owed.
//   What orders the flag after the data: every storing wave drains its stores
//   (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, and only then wave 0 stores the flag
//   with all its lanes (publish_flag, publish2, publish_by).  Data stored with plain stores
//   instead needs the agent release between the barrier and the flag: publish(flag, v, true).
// Consumer.  A wave polls the flag with an sc1 load (ld_uni, ld_agent; ld_sys for a flag another
//   rank stores) and, after its poll has matched, reads the handed-off bytes with ld_sc1 / ld_nc
//   only: loads that bypass this CU's L1, which no other CU's store refreshes.  Waves that did
//   not poll read after a workgroup barrier the polling wave joins (agree, or the kernel's next
//   barrier).  A consumer that reads with plain loads acquires first (the callers' fence).
//   A chain may poll the data values themselves against a sentinel no result can equal
//   (k_bsolve.hip): the same loads, one round trip fewer.
// Order.  Work is claimed through a ticket counter (claim_ticket) in dependency order, so a
//   workgroup waits only on work claimed by workgroups already running: no dispatch order can
//   deadlock.
// Every spin is bounded.  wait_until is the only wait loop: it ends when the predicate holds,
//   when another workgroup has set the launch's error word, or when `tlimit` wall-clock ticks
//   (100 MHz) have passed since t0 -- it then sets the error word itself, so every other wait of
//   the launch ends at its next look and the kernel reports *info = -1.  A producer that never
//   comes costs the time limit, not the machine.
#pragma once
#include <hip/hip_runtime.h>

namespace gprx {
namespace ho {

// ---- memory primitives -------------------------------------------------------------------------
// global_load_dword sc1: a flag or counter poll, per lane (first row: "an sc1 load poll")
__device__ __forceinline__ int ld_agent(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// global_store_dword sc1: the flag store or error word (first row: "an sc1 flag store")
__device__ __forceinline__ void st_agent(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ld_agent made wave-uniform (v_readfirstlane): a poll loop on it is a scalar loop, no divergence
__device__ __forceinline__ int ld_uni(const int* p) { return __builtin_amdgcn_readfirstlane(ld_agent(p)); }
// global_load sc1 of handed-off data (first row, "loads, all sc1": L2-served, never this CU's L1)
template <typename T>
__device__ __forceinline__ T ld_sc1(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// global_store sc1 of handed-off data (first row, "stores, all sc1": written through)
template <typename T>
__device__ __forceinline__ void st_sc1(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// global_load_dword sc0 sc1: a flag word another rank stores into this rank's mailbox
__device__ __forceinline__ unsigned ld_sys(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// global_store_dword sc0 sc1: a flag word in a mailbox (this rank's or another's)
__device__ __forceinline__ void st_sys(unsigned* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// global_load sc0 sc1 of data another rank pushed ({sc0 sc1 both sides}: bypasses stale lines)
template <typename T>
__device__ __forceinline__ T ld_nc(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// global_store sc0 sc1 of data for another workgroup or rank ({sc0 sc1 both sides}: written
// through to the destination, the line dropped from this XCD's L2)
template <typename T>
__device__ __forceinline__ void st_nc(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// ---- control words and the claim ---------------------------------------------------------------
// head of the counter block of the three chain kernels (k_bsolve, k_append, k_dsolve); the
// per-block flags follow.  (k_ptiles.hip keeps its own, longer layout: mm::C_NCTL.)
enum { C_TICKET = 0, C_ERR = 1, C_NCTL = 4 };

// The workgroup's next ticket, wave-uniform in every wave.  Wave 0 adds with ALL its lanes (lane
// 0 adds 1, the others 0: one atomic instruction, no divergent block) and passes the value
// through the LDS word s_slot; the barrier publishes it.
__device__ __forceinline__ int claim_ticket(int* ctl, int* s_slot) {
    if (wave_id() == 0) {
        const int v = __hip_atomic_fetch_add(ctl + C_TICKET, (threadIdx.x == 0) ? 1 : 0, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        *s_slot = __builtin_amdgcn_readfirstlane(v);
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*s_slot);
}

// ---- the one bounded wait ----------------------------------------------------------------------
struct Nop {
    __device__ __forceinline__ void operator()() const {}
};

// Poll ready() until it holds: s_sleep(SLEEP) between polls; the error word and the clock are
// looked at on every CHECK_EVERY-th poll (a power of two: each look is a round trip of its own
// between two polls).  False when another workgroup set *err_word, or when more than tlimit
// ticks have passed since t0: then on_timeout() runs (a diagnostic record) and *err_word is set.
// ready() may poll per lane (the lanes then leave one by one) or wave-uniformly; it may keep
// what it loaded through a reference capture.
template <int SLEEP = 1, int CHECK_EVERY = 1, class Ready, class OnTimeout = Nop>
__device__ __forceinline__ bool wait_until(Ready ready, int* err_word, long long t0, long long tlimit,
                                           OnTimeout on_timeout = {}) {
    static_assert(CHECK_EVERY > 0 && (CHECK_EVERY & (CHECK_EVERY - 1)) == 0, "CHECK_EVERY: a power of two");
    for (int spins = 1;; spins++) {
        if (ready()) return true;
        if (CHECK_EVERY == 1 || (spins & (CHECK_EVERY - 1)) == 0) {
            if (ld_uni(err_word)) return false;
            if (wall_clock64() - t0 > tlimit) {
                on_timeout();
                st_agent(err_word, 1);
                return false;
            }
        }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

// ---- publish -----------------------------------------------------------------------------------
// every wave's stores complete, then wave 0 releases and publishes *flag = v.  Wave 0 acts
// with ALL its lanes (same value to the same word): no lane-divergent code near the task
// loop's back edge, where the structurizer was seen to sink a `lane == 0` block past the
// next iteration's barrier (a hang).
//
// release = false: every handed-off byte was stored sc1 (tile_gemm), so draining the stores
// (vmcnt(0) in every wave, then the barrier) is the release; the consumer still acquires.
__device__ __forceinline__ void publish(int* flag, int v, bool release) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave_id() == 0) {
        if (release) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        st_agent(flag, v);
    }
}

// two counters after one drain (a paired update's tiles)
__device__ __forceinline__ void publish2(int* f1, int* f2, int v) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave_id() == 0) {
        st_agent(f1, v);
        st_agent(f2, v);
    }
}

// The drain-barrier-flag sequence with the flag stores left to the caller: every wave drains its
// (written-through) stores, the barrier, then wave 0 runs store() with all its lanes.
template <class Store>
__device__ __forceinline__ void publish_by(Store store) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave_id() == 0) store();
}

// one flag of a chain whose data went out with st_sc1 / st_nc
__device__ __forceinline__ void publish_flag(int* flag, int v) {
    publish_by([=] { st_agent(flag, v); });
}

// stores of this workgroup visible to its own later loads (same CU); also the drain and barrier
// of a publish whose flag store the caller places itself (k_append.hip: one lane, no loop after)
__device__ __forceinline__ void local_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// ---- agree -------------------------------------------------------------------------------------
// After waits that each wave (or lane) made on its own: true in every thread when all of them
// succeeded.  Two barriers; the second also publishes what the threads wrote to LDS before the
// call.  (Any failing lane stores: a per-lane poll fails per lane.)
__device__ __forceinline__ bool agree(bool ok, int* s_slot) {
    if (threadIdx.x == 0) *s_slot = 0;
    __syncthreads();
    if (!ok) *s_slot = 1;
    __syncthreads();
    return *s_slot == 0;
}

}  // namespace ho
}  // namespace gprx
