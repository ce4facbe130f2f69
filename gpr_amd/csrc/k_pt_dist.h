// k_pt_dist.h — the device side of the sharded factorisation's transport (potrf_tiles_kernel<T,
// true>; host side and layout: gprx_dist.h, gprx_dist.cpp): this rank's packed tile storage, the
// other ranks' mailboxes, windows and flag words, the push of a finished tile to its consumers,
// the window releases, and the record a timed-out wait leaves for the host's error message.
#pragma once
#include "gprx_dist.h"
#include "k_pt_ops.h"

namespace gprx {
namespace pt {

static_assert(C_NCTL == C_NCTL_DIST, "counter block layout shared with gprx_dist.cpp");

template <typename T>
struct Args;  // the launch arguments (k_ptiles.hip)

// A timed-out wait of the distributed factorisation leaves one record (the first) at
// check_err[DIST_TO_REC..+7]: kind (1 inputs, 2 window release), task type, i, j, b0 | nb << 16,
// detail (inputs: bit mask of the unmet conditions; release: the consumer rank), the value seen,
// the ticket.  gprx_dist.cpp prints it with the fit's timeout error.
constexpr int DIST_TO_REC = 132;
__device__ __forceinline__ void dist_note_timeout(int* rec, int kind, int type, int i, int j, int b0nb, int detail,
                                                  int seen) {
    if (!rec) return;
    if (__hip_atomic_fetch_add(rec, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    if (atomicCAS(rec, 0, kind) != 0) return;
    rec[1] = type;
    rec[2] = i;
    rec[3] = j;
    rec[4] = b0nb;
    rec[5] = detail;
    rec[6] = seen;
}

// ---- distributed factorisation (DIST): packed storage, mailbox pushes -----------------------
// tile (i, j) of this rank's own row block i in the packed storage (ld DB): matrix / label rows
// keep columns 0..i, identity row E_a = nc + 1 + a columns a..nc-1, then C columns E_0..E_a
template <typename T>
__device__ __forceinline__ T* dist_tile(T* A, const PtDist<T>& D, int i, int j) {
    const int li = __builtin_amdgcn_readfirstlane(D.loc[i]);
    int col = j;
    if (i > D.nc) {
        const int aa = i - D.nc - 1;
        col = (j < D.nc) ? j - aa : D.nc - aa + (j - D.nc - 1);
    }
    const int64_t ro = D.roff[li];
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)ro), hi = __builtin_amdgcn_readfirstlane((uint32_t)(ro >> 32));
    return A + (int64_t)(((uint64_t)hi << 32) | lo) + (int64_t)col * DB * DB;
}
// counter column of tile (i, j): the C tiles (j = E_c) after the nc matrix columns
__device__ __forceinline__ int dist_col(int nc, int j) { return j > nc ? j - 1 : j; }

template <typename T>
__device__ __forceinline__ unsigned* dist_flags(const PtDist<T>& D, int q) {
    const uint64_t b = D.mb[q] + (uint64_t)D.o_flags;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return reinterpret_cast<unsigned*>(((uint64_t)hi << 32) | lo);
}
// window slot t (= (b mod ww) nr + j) of rank q
template <typename T>
__device__ __forceinline__ char* dist_win(const PtDist<T>& D, int q, int64_t t) {
    const int64_t tpp = D.tpp;
    const int64_t pc = t / tpp;
    const uint64_t b = D.wpc[(int64_t)q * D.npc + pc] + (uint64_t)((t - pc * tpp) * DB * DB * (int64_t)sizeof(T));
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return reinterpret_cast<char*>(((uint64_t)hi << 32) | lo);
}
template <typename T>
__device__ __forceinline__ char* dist_mb(const PtDist<T>& D, int q, int64_t off) {
    const uint64_t b = D.mb[q] + (uint64_t)off;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return reinterpret_cast<char*>(((uint64_t)hi << 32) | lo);
}

// ranks other than r that consume row block j (bit q)
template <typename T>
__device__ __forceinline__ unsigned dist_consumers(const PtDist<T>& D, int j) {
    unsigned m = 0;
    for (int q = 0; q < D.g; q++)
        if (q != D.r && D.cons[(int64_t)q * D.nr + j]) m |= 1u << q;
    return __builtin_amdgcn_readfirstlane(m);
}

// Wave 0: wait until every rank in `mask` released panel p (its window slot may be refilled);
// ranks with no window-reading chunk on p never store the flag and are not waited for.
template <typename T>
__device__ bool dist_wait_release(const Args<T>& a, const PtDist<T>& D, unsigned mask, int p) {
    if (p < 0) return true;
    const unsigned* fl = dist_flags(D, D.r) + dist_f_rel(D.nr, D.nc);
    const long long t0 = wall_clock64();
    for (int q = 0; q < D.g; q++) {
        if (!((mask >> q) & 1) || __builtin_amdgcn_readfirstlane(D.need[(int64_t)q * D.nc + p]) == 0) continue;
        unsigned seen;
        if (!wait_until<2>([&] { return (seen = __builtin_amdgcn_readfirstlane(ld_sys(fl + (int64_t)q * D.nc + p))) == D.ep; },
                           a.ctl + C_ERR, t0, a.tlimit, [&] {
                               if ((threadIdx.x & 63) == 0)
                                   dist_note_timeout(D.check_err + DIST_TO_REC, 2, -1, D.r, p, 0, q, (int)seen);
                           }))
            return false;
    }
    return true;
}

// The whole workgroup: copy one DB x DB tile (contiguous, written by this workgroup and
// drained: its stores are visible to this CU) to byte offset `off` of the mailbox of every
// rank in `mask` (off < 0: to window slot tag_idx), then set each one's flag word `fidx` to the
// epoch.  Across devices (D.wt) the
// copies are 16-byte `sc0 sc1` stores (written through to the destination, not left dirty in
// this XCD's L2), so the flag needs only every wave's s_waitcnt vmcnt(0) and a barrier -- no
// buffer_wbl2, which would write back every dirty line of the XCD's L2 (the update tasks'
// tiles) on each push (MI355X_MICROARCH.md, the {sc0 sc1 stores} form; the consumer acquires
// before its loads).  Ranks of one device: plain stores and one system-scope release.
template <typename T>
__device__ void dist_push(const T* src, const PtDist<T>& D, unsigned mask, int64_t off, int64_t fidx, const int t,
                          int64_t tag_idx = -1, unsigned tag = 0) {
    if (!mask) return;
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    constexpr int NV = DB * DB * (int)sizeof(T) / 16 / NT;  // 16-byte vectors per thread
    constexpr int CH = 4;
    const bool wt = __builtin_amdgcn_readfirstlane(D.wt) != 0;
    if (wave_id() == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // this CU's L1: no stale lines of src
    __syncthreads();
    const u4* s4 = reinterpret_cast<const u4*>(src);
#pragma unroll
    for (int c = 0; c < NV; c += CH) {
        u4 v[CH];
#pragma unroll
        for (int u = 0; u < CH; u++) v[u] = s4[t + (c + u) * NT];
        for (int q = 0; q < D.g; q++) {
            if (!((mask >> q) & 1)) continue;
            u4* d4 = reinterpret_cast<u4*>(off < 0 ? dist_win(D, q, tag_idx) : dist_mb(D, q, off));
            if (wt) {
#pragma unroll
                for (int u = 0; u < CH; u++)
                    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(d4 + t + (c + u) * NT), "v"(v[u])
                                 : "memory");
            } else {
#pragma unroll
                for (int u = 0; u < CH; u++) d4[t + (c + u) * NT] = v[u];
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave_id() == 0) {
        if (!wt) {  // ranks of one device: plain stores, one release
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (D.check && tag_idx >= 0)
            for (int q = 0; q < D.g; q++)
                if ((mask >> q) & 1) st_sys(reinterpret_cast<unsigned*>(dist_mb(D, q, D.o_tags)) + tag_idx, tag);
        for (int q = 0; q < D.g; q++)
            if ((mask >> q) & 1) st_sys(dist_flags(D, q) + fidx, D.ep);
    }
}

// GPRX_DIST_CHECK: the window slots of row j, panels b0.. b0 + nb - 1, hold exactly those tiles
// of this fit (tag = epoch << 16 | panel + 1); counts mismatches into check_err[which]
template <typename T>
__device__ void dist_check_tags(const PtDist<T>& D, int j, int b0, int nb, int which) {
    const int lane = threadIdx.x & 63;
    if (lane < nb) {
        const int b = b0 + lane;
        const unsigned* tg = reinterpret_cast<const unsigned*>(dist_mb(D, D.r, D.o_tags)) + (int64_t)(b % D.ww) * D.nr + j;
        const unsigned want = (D.ep << 16) | (unsigned)(b + 1);
        const unsigned got = ld_sys(tg);
        if (got != want) {
            atomicAdd(D.check_err + which, 1);
            const int e = atomicAdd(D.check_err + 2, 1);
            if (e < 32) {  // log: which, row, panel, time
                int* lg = D.check_err + 4 + 4 * e;
                lg[0] = which;
                lg[1] = j;
                lg[2] = b;
                lg[3] = (int)(wall_clock64() & 0x7fffffff);
            }
        }
    }
}

// Wave 0 of an update that read row j from the window: count the chunk on its panels; the
// chunk completing a panel's count stores the release flag into every other rank's mailbox.
template <typename T>
__device__ void dist_release(const PtDist<T>& D, int b0, int nb) {
    // lane l < nb counts the chunk on panel b0 + l (its own counter word); the others add 0.
    // Integer masks throughout: the 64-bit ballot / count-trailing-zeros form of this loop was
    // seen to release panel b0 + 32 together with panel b0 (lane 32 of a 32-wide chunk).
    const int lane = threadIdx.x & 63;
    const int valid = lane < nb ? 1 : 0;
    const int p = b0 + (valid ? lane : 0);
    const int old = __hip_atomic_fetch_add(D.ucnt + p, valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int needv = D.need[(int64_t)D.r * D.nc + p];
    const int dn = valid & (old + 1 == needv ? 1 : 0);
    for (int l = 0; l < nb; l++) {
        if (!__builtin_amdgcn_readfirstlane(__shfl(dn, l))) continue;
        for (int q = 0; q < D.g; q++)
            if (q != D.r) st_sys(dist_flags(D, q) + dist_f_rel(D.nr, D.nc) + (int64_t)D.r * D.nc + b0 + l, D.ep);
    }
}

}  // namespace pt
}  // namespace gprx
