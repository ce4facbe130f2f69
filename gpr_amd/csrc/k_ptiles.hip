// k_ptiles.hip — tile-dataflow Cholesky in ONE persistent launch (gfx950).
//
// Replaces the reference's factorise/invert step (lapack::lu_invert -> dgetrf_+dgetri_,
// include/LAPACKUtils.h:38-56, 85-97, called from GaussianProcess::InvertKernelMatrix,
// lib/GaussianProcess.cpp:545-559) with K + sigma^2 I = L L^T, the forward solve z = L^{-1} Y
// riding along as extra row blocks, scheduled on the device.
//
// Why: in a stream formulation (one kernel per step; removed) every step of the
// panel chain (diagonal factor -> trsm -> next-column update) is a kernel that must wait for CU
// slots held by the bulk trailing GEMM, so at N = 16384 the chain (18 ms alone) stretched to
// most of the 37 ms factorisation.  Here one workgroup per CU runs a loop over a ticket list of 128x128 TILE
// TASKS (pt_sched.h: T_DIAGX .. T_UPD2) with per-tile dependency counters in HBM:
//
//   BUILD(i,j)       the covariance tile A_ij from the pair statistics (k_pairs.h build_tile_sum)
//   DIAGX(k)         factor A_kk = L_kk L_kk^T and form Linv_k (k_pt_diag.h).  Unsplit, k > 0:
//                    first T = A_{k,k-1} Linv_{k-1}^T and A_kk -= T T^T, the whole critical step
//                    in one task (f64: diagx_ts, S left in the factor's LDS image).  Split: the
//                    parts have formed T and S; the task fetches S and factors (diagx_split)
//   TPART(k,p)       split diagonal step (k_pt_split.h): part p of T = L_{k,k-1} and of
//                    S = A_kk - T T^T; tp_parts parts per step (f64 eight, f32 four)
//   TRSM(i,k)        L_ik = A_ik Linv_k^T                  (i >= k+2, and the label rows)
//   UPD(i,j,b0,nb)   A_ij -= sum_{b0<=b<b0+nb} L_ib L_jb^T  (nb = W for far-behind panels; the
//                    label row block of a fit with <= 16 labels: its 16 live rows only)
//   UPD2(i,j,b0,nb)  the same for tiles (i,j) and (i+1,j) as one 256 x 128 product (one GPU)
//
// Counters: ver[i][j] = number of b already applied to tile (i,j) (-1: not built); lcnt[i] =
// number of final blocks L_i0..L_i,lcnt-1 of row block i; tflag[k][p] = TPART(k,p)'s phase.
// Wait conditions (wait_inputs; DIST: a dependency that lives on another rank is its flag
// words in this rank's mailbox instead, k_pt_dist.h):
//   BUILD:     none
//   DIAGX(0):  ver[0][0] == 0
//   DIAGX(k):  ver[k][k-1] == k-1, ver[k][k] == k-1, lcnt[k-1] >= k
//              split: ver[k][k] == k-1; inside the task every tflag[k][p] == 3
//   TPART(k,p): ver[k][k-1] == k-1; inside the task lcnt[k-1] >= k (Linv_{k-1}), the sibling
//              parts' tflag (1 before T's in-place stores, 2 before S) and ver[k][k] == k-1
//   TRSM(i,k): ver[i][k] == k, lcnt[k] >= k+1
//   UPD:       ver[i][j] == b0, lcnt[i] >= b0+nb, lcnt[j] >= b0+nb
//   UPD2:      UPD's for both tiles: also ver[i+1][j] == b0, lcnt[i+1] >= b0+nb
// The ticket order is a list schedule computed on the host (pt_sched.cpp: critical-path priorities,
// simulated on P workers): every task's producers hold earlier tickets, and a workgroup that
// holds a ticket is running, so the smallest unfinished ticket can always proceed -- no
// deadlock whatever the real durations.  Every wait is also bounded in wall-clock time: a
// timeout raises an error flag that drains every workgroup and is reported as info = -1.
//
// Hand-offs follow k_handoff.h: every handed-off tile leaves in write-through (sc1) stores, so
// no L2 write-back is owed; every storing wave drains its stores (s_waitcnt vmcnt(0)), the
// workgroup meets at a barrier, and only then wave 0 stores the counter (publish).  Consumer:
// wave 0 polls with sc1 loads, acquires, and the workgroup meets at a barrier before it reads.
// (The f32 diagonal factor stores plainly and publishes with the agent release: diag_factor.)
//
// Tile GEMM (k_mma.h): 512 threads = 8 waves of 64x32 (v_mfma_f64_16x16x4f64 /
// _f32_16x16x4f32), operands brought by LDS-DMA into a ring of 4 stage buffers of 16 k-columns
// (f32: 32), three stages in flight ahead of the MFMAs; 147 KB of LDS per workgroup also keeps
// the launch at one workgroup per CU, so the critical DIAGX step has a whole CU.
//
// The task loop sits at 256 VGPRs: what it calls out of line (diag_factor,
// tpart_run, tpart_run8, diagx_split) is out of line on purpose, and nothing here is compiled
// in more than one form.  `make codeobj` hashes the device code: a refactor leaves it unchanged.
//
// This file: the launch arguments, wait_inputs, the task loop (potrf_tiles_kernel), the
// diagonal factors' microbenchmark kernel, and the host launcher with its per-context state.
//   k_pt_ops.h    the tile products: tile_gemm, tile_trsm, tile_gemm_rows16, tile_gemm_tall
//   k_pt_diag.h   the 128 x 128 diagonal factors: rank-8 image, blocked, blocked with look-ahead
//   k_pt_dist.h   the device side of the sharded transport: packed tiles, mailbox pushes, releases
//   k_pt_split.h  the split diagonal step: diagx_ts, the TPART parts, diagx_split
#include "gprx_dist.h"
#include "gprx_internal.h"
#include "k_handoff.h"
#include "k_pairs.h"
#include "k_pt_diag.h"
#include "k_pt_dist.h"
#include "k_pt_ops.h"
#include "k_pt_split.h"
#include "pt_sched.h"

#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

namespace gprx {
namespace pt {

// Developer microbenchmark (gprx_dev_bench what 11 / 12): one workgroup factors `reps` fresh
// 128 x 128 blocks (A + r * DB * ld) back to back with variant V (0 rank-8, 1 blocked, 2 look-ahead); prof
// accumulates the variant's phase ticks (wall clock, 100 MHz) over the reps.
template <typename T, int V>
__global__ __launch_bounds__(NT) void diag_bench_kernel(T* A, int64_t ld, T* Linv, int* info, long long* prof,
                                                        int reps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    long long acc[5] = {0, 0, 0, 0, 0};
    long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // [4..6]: fact32 core-clock split (GPRX_FACT32_PROF)
    for (int r = 0; r < reps; r++) {
        const long long t0 = wall_clock64();
        if (V == 0) diag_factor_rank8<T>(A + (int64_t)r * DB * ld, ld, Linv, info, 0, smem_raw, threadIdx.x, nullptr, ph);
        else if (V == 1) diag_factor_blocked<T>(A + (int64_t)r * DB * ld, ld, Linv, info, 0, smem_raw, threadIdx.x, ph);
        else diag_factor_la<T>(A + (int64_t)r * DB * ld, ld, Linv, info, 0, smem_raw, threadIdx.x, ph);
        __syncthreads();
        const long long t1 = wall_clock64();
        acc[0] += ph[0];
        acc[1] += ph[1];
        acc[2] += ph[2];
        acc[3] += ph[3];
        acc[4] += t1 - t0;
    }
    if (threadIdx.x == 0) {
        for (int u = 0; u < 5; u++) prof[u] = acc[u];
        for (int u = 0; u < 3; u++) prof[5 + u] = ph[4 + u];
    }
}

template <typename T>
void launch_diag_bench(int variant, T* A, int64_t ld, T* Linv, int* info, long long* prof, int reps, hipStream_t s) {
    const size_t lds = diag_lds<T>() + 64;
    auto go = [&](auto kfn) {
        GPRX_HIP(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kfn, dim3(1), dim3(NT), lds, s, A, ld, Linv, info, prof, reps);
    };
    if (variant == 0 || !std::is_same<T, double>::value) go(diag_bench_kernel<T, 0>);
    else if (variant == 1) go(diag_bench_kernel<T, 1>);
    else go(diag_bench_kernel<T, 2>);
    GPRX_HIP(hipGetLastError());
}
template void launch_diag_bench<double>(int, double*, int64_t, double*, int*, long long*, int, hipStream_t);
template void launch_diag_bench<float>(int, float*, int64_t, float*, int*, long long*, int, hipStream_t);

template <typename T>
constexpr size_t pt_lds_bytes() {
    return gemm_lds<T>() > diag_lds<T>() ? gemm_lds<T>() : diag_lds<T>();
}
static_assert(tall_lds<double>() <= pt_lds_bytes<double>() && tall_lds<float>() <= pt_lds_bytes<float>(),
              "the paired update's ring exceeds the LDS of the launch");

template <typename T>
struct Args {
    T* A;
    int64_t ld;
    T* Linv;
    const int4* tasks;
    int ntasks;
    int nc;        // column blocks (= diagonal blocks)
    int nv;        // columns of the ver counter array (nc; 2 nc with the C tiles of DIST LML mode)
    int* ctl;      // [C_NCTL] control words, then lcnt[nr], then ver[nr * nc]
    int* lcnt;
    int* ver;
    int* info;
    long long tlimit;  // wall-clock ticks (100 MHz) a single wait may take
    int* dbg;          // GPRX_PT_DEBUG: per-workgroup {ticket, phase, i, j} in pinned host memory
    int variant;       // GPRX_PT_VARIANT debug bits: 1 no TRSM math, 2 no UPD math, 4 no diag factor
    long long* trace;  // GPRX_PT_TRACE: per ticket {ticket taken, inputs ready, published, workgroup}
    long long* xt;     // GPRX_PT_TRACE, one GPU: the split step's phase stamps (TpCtx::xt)
    const TileBuild<T>* tb;  // BUILD tasks: covariance tiles from pair statistics (device copy,
                             // read per task: as kernel arguments they stayed live in SGPRs and
                             // pushed the whole kernel into spills)
    const PtDist<T>* dist;   // distributed factorisation (potrf_tiles_kernel<T, true> only)
    // split diagonal step (f64): TPART(k, p) tasks form L_{k,k-1} and S = A_kk - L L^T in
    // quarters; DIAGX(k) copies S and factors it (diagx_split)
    int split;
    T* pbuf;     // DB x DB: S, its lower tiles written by the parts
    int* tflag;  // [nc][TP_STRIDE] TPART(k, p) state: 1 its A operand is read, 2 its T stored, 3 its S quarter
                 // stored
    int lab_rows;  // live rows of the label row block nc (one GPU): <= LAB_NARROW, its updates take
                   // the 16-row product (tile_gemm_rows16); GT = the full tile
};
constexpr int LAB_NARROW = 16;


// Wave 0 waits until the task's inputs are final (all lanes load the same words; the values
// are made wave-uniform, so the loop is a scalar loop with no divergence).  Returns false on
// timeout or when another workgroup raised the error flag.
template <typename T, bool DIST>
__device__ bool wait_inputs(const Args<T>& a, int type, int i, int j, int b0, int nb) {
    const int* vp;
    int vwant;
    const int* vp2;
    int vwant2;
    const int* lp1;
    int lwant1;
    const int* lp2;
    int lwant2;
    // DIST: one dependency may be data of another rank: its flag words in this rank's mailbox
    // (Linv_k: one word; the tiles of a remote row: one word per panel of the chunk)
    const unsigned* rp = nullptr;
    int rn = 0;
    unsigned ep = 0;
    const int* lp3 = nullptr;  // T_UPD2: the second row's final blocks (>= lwant1)
    if (type == T_TPART) {  // its A operand final (Linv_{i-1} is waited for inside the task)
        vp = a.ver + (int64_t)i * a.nv + (i - 1);
        vwant = i - 1;
        vp2 = vp;
        vwant2 = vwant;
        lp1 = a.lcnt + i;
        lwant1 = 0;
        lp2 = lp1;
        lwant2 = 0;
    } else if (type == T_DIAGX && i > 0 && a.split) {  // A_ii through panel i-2
        vp = a.ver + (int64_t)i * a.nv + i;
        vwant = i - 1;
        vp2 = vp;
        vwant2 = vwant;
        lp1 = a.lcnt + i;
        lwant1 = 0;
        lp2 = lp1;
        lwant2 = 0;
        // (A_kk only: the TPART products are waited for inside the task, A_kk loads meanwhile)
    } else if (type == T_DIAGX && i == 0) {  // the first diagonal tile is built
        vp = a.ver;
        vwant = 0;
        vp2 = vp;
        vwant2 = 0;
        lp1 = a.lcnt;
        lwant1 = 0;
        lp2 = lp1;
        lwant2 = 0;
    } else if (type == T_BUILD) {
        return true;
    } else if (type == T_DIAGX) {
        vp = a.ver + (int64_t)i * a.nv + (i - 1);
        vwant = i - 1;
        vp2 = a.ver + (int64_t)i * a.nv + i;
        vwant2 = i - 1;
        lp1 = a.lcnt + (i - 1);
        lwant1 = i;
        lp2 = lp1;
        lwant2 = lwant1;
        if constexpr (DIST) {
            const PtDist<T>& D = *a.dist;
            if (__builtin_amdgcn_readfirstlane(D.loc[i - 1]) < 0) {  // Linv_{i-1} pushed by its rank
                lp1 = lp2 = a.lcnt + i;
                lwant1 = lwant2 = 0;
                rp = dist_flags(D, D.r) + dist_f_linv(D.nr, D.nc) + (i - 1);
                rn = 1;
                ep = D.ep;
            }
        }
    } else if (!DIST && type == T_UPD2) {  // tiles (i, j), (i + 1, j); rows i, i + 1 and j final through the chunk
        vp = a.ver + (int64_t)i * a.nv + j;
        vwant = b0;
        vp2 = a.ver + (int64_t)(i + 1) * a.nv + j;
        vwant2 = b0;
        lp1 = a.lcnt + i;
        lwant1 = b0 + nb;
        lp2 = a.lcnt + j;
        lwant2 = b0 + nb;
        lp3 = a.lcnt + i + 1;
    } else if (type == T_TRSM) {
        vp = a.ver + (int64_t)i * a.nv + j;
        vwant = j;
        vp2 = vp;
        vwant2 = vwant;
        lp1 = a.lcnt + j;
        lwant1 = j + 1;
        lp2 = lp1;
        lwant2 = lwant1;
        if constexpr (DIST) {
            const PtDist<T>& D = *a.dist;
            if (__builtin_amdgcn_readfirstlane(D.loc[j]) < 0) {  // Linv_j pushed by its rank
                lp1 = lp2 = a.lcnt + i;
                lwant1 = lwant2 = 0;
                rp = dist_flags(D, D.r) + dist_f_linv(D.nr, D.nc) + j;
                rn = 1;
                ep = D.ep;
            }
        }
    } else {
        const int jc = DIST ? dist_col(a.dist->nc, j) : j;
        vp = a.ver + (int64_t)i * a.nv + jc;
        vwant = b0;
        vp2 = vp;
        vwant2 = vwant;
        lp1 = a.lcnt + i;
        lwant1 = b0 + nb;
        lp2 = a.lcnt + j;
        lwant2 = b0 + nb;
        if constexpr (DIST) {
            const PtDist<T>& D = *a.dist;
            if (__builtin_amdgcn_readfirstlane(D.loc[j]) < 0) {  // row j's tiles: pushed, one flag per panel
                lp2 = lp1;
                rp = dist_flags(D, D.r) + dist_f_tile() + (int64_t)j * D.nc + b0;
                rn = nb;
                ep = D.ep;
            }
        }
    }
    const int lane = threadIdx.x & 63;
    const long long t0 = wall_clock64();
    for (;;) {
        // bitwise: all four loads are issued before any compare resolves
        int ok = int(ld_uni(vp) == vwant) & int(ld_uni(vp2) == vwant2) & int(ld_uni(lp1) >= lwant1) &
                 int(ld_uni(lp2) >= lwant2);
        if (!DIST && lp3) ok &= int(ld_uni(lp3) >= lwant1);
        if constexpr (DIST) {
            if (rp) {  // lane l checks flag l (l < rn): one vector load, one ballot
                const bool good = lane >= rn || ld_sys(rp + (lane < rn ? lane : 0)) == ep;
                ok &= int(__builtin_amdgcn_readfirstlane((uint32_t)(__ballot(!good) == 0)));
            }
        }
        if (ok) return true;
        if (ld_uni(a.ctl + C_ERR)) return false;
        if (wall_clock64() - t0 > a.tlimit) {
            if constexpr (DIST) {
                int miss = int(ld_uni(vp) != vwant) | (int(ld_uni(vp2) != vwant2) << 1) | (int(ld_uni(lp1) < lwant1) << 2) |
                           (int(ld_uni(lp2) < lwant2) << 3);
                int seen = ld_uni(vp);
                if (rp) {
                    const bool good = lane >= rn || ld_sys(rp + (lane < rn ? lane : 0)) == ep;
                    const unsigned long long bad = __ballot(!good);
                    if (bad) {
                        miss |= 16 | ((int)__builtin_ctzll(bad) << 8);
                        seen = (int)__builtin_amdgcn_readfirstlane(ld_sys(rp + (int)__builtin_ctzll(bad)));
                    }
                }
                if (lane == 0) dist_note_timeout(a.dist->check_err + DIST_TO_REC, 1, type, i, j, b0 | (nb << 16), miss, seen);
            }
            st_agent(a.ctl + C_ERR, 1);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

template <typename T>
__device__ __forceinline__ TpCtx<T> tp_ctx(const Args<T>& a) {
    return TpCtx<T>{a.ctl, a.lcnt, a.tflag, a.pbuf, a.dist, a.tlimit, a.xt, a.nc, a.ver, a.nv};
}
// the split step's context lives in LDS after the ticket words (written once per launch):
// the out-of-line calls take one pointer (by value, its ten fields cost the task loop spills)
template <typename T>
constexpr size_t pt_lds_ctx_off() {
    return pt_lds_bytes<T>() + 16;
}
template <typename T>
constexpr size_t pt_lds_total() {
    return pt_lds_ctx_off<T>() + sizeof(TpCtx<T>);
}

template <typename T, bool DIST>
__global__ __launch_bounds__(NT) void potrf_tiles_kernel(Args<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // ONE __shared__ array (a second __shared__ object can make hipcc drain the LDS-DMA
    // pipeline with vmcnt(0)); the ticket word sits after the largest per-task image
    int& s_q = *reinterpret_cast<int*>(smem_raw + pt_lds_bytes<T>());
    int& s_ok = *reinterpret_cast<int*>(smem_raw + pt_lds_bytes<T>() + sizeof(int));
    TpCtx<T>* tpc = reinterpret_cast<TpCtx<T>*>(smem_raw + pt_lds_ctx_off<T>());
    if (threadIdx.x == 0) *tpc = tp_ctx(a);  // (visible after the task loop's first barrier)
    T* smem = reinterpret_cast<T*>(smem_raw);
    const int t = threadIdx.x;
    const int wv = wave_id();
    const int64_t ld = a.ld;
    for (;;) {
        if (wv == 0) {  // one ticket per workgroup: lane 0 adds 1, the other lanes 0
            // (not taken ahead of time: a ticket claimed while the previous task still runs
            // delays critical-path tasks behind long updates -- measured 28.8 -> 33.2 ms)
            const int v = __hip_atomic_fetch_add(a.ctl + C_TICKET, (t == 0) ? 1 : 0, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            s_q = __builtin_amdgcn_readfirstlane(v);
        }
        __syncthreads();
        // everything below is wave-uniform: keep it in SGPRs so the task dispatch is scalar
        const int q = __builtin_amdgcn_readfirstlane(s_q);
        if (q >= a.ntasks) break;
        const long long tr0 = a.trace ? wall_clock64() : 0;
        const int4 tk = a.tasks[q];
        const int type = __builtin_amdgcn_readfirstlane(tk.x & 0xff), nb = __builtin_amdgcn_readfirstlane(tk.x >> 8);
        const int i = __builtin_amdgcn_readfirstlane(tk.y), j = __builtin_amdgcn_readfirstlane(tk.z),
                  b0 = __builtin_amdgcn_readfirstlane(tk.w);
        dbg_mark(a.dbg, q, 1 + 10 * type, i, j);
        // wave 0 alone polls the task's counters (the other waves sleep in the barrier: eight
        // times fewer loads on the counters -- hundreds of workgroups polling the transport's
        // uncached words measured 10x slower distributed fits), then acquires for the
        // workgroup (invalidates this CU's L1).  All of wave 0's lanes store the same word.
        if (wv == 0) {
            const bool ok0 = wait_inputs<T, DIST>(a, type, i, j, b0, nb);
            if (ok0 && !(a.variant & 32)) {
                bool remote = false;  // DIST: an input pushed by another rank (system-scope acquire)
                if constexpr (DIST) {
                    const PtDist<T>& D = *a.dist;
                    const int dep = (type == T_DIAGX) ? i - 1 : ((type == T_BUILD || type == T_TPART) ? -1 : j);
                    remote = dep >= 0 && __builtin_amdgcn_readfirstlane(D.loc[dep]) < 0 &&
                             !__builtin_amdgcn_readfirstlane(D.acq_agent);
                }
                if (remote) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            s_ok = ok0 ? 1 : 0;
        }
        __syncthreads();
        if (!__builtin_amdgcn_readfirstlane(s_ok)) break;
        const long long tr1 = a.trace ? wall_clock64() : 0;
        const long long tc1 = a.trace ? (long long)__builtin_amdgcn_s_memtime() : 0;
        dbg_mark(a.dbg, q, 2 + 10 * type, i, j);
        // opaque copy of the thread index: keeps the per-task address arithmetic inside the
        // task instead of hoisted (and held in registers) across the whole task loop
        int tid = t;
        asm volatile("" : "+v"(tid));
        if constexpr (DIST) {
            // ---- one rank of the distributed factorisation: packed own rows (ld DB), remote
            // rows from the window, final tiles pushed to their consumers' mailboxes ----------
            const PtDist<T>& D = *a.dist;
            bool ok = true;
            if (type == T_TPART) {
                ok = tpart_task<T, true>(tpc, dist_tile(a.A, D, i, i - 1), dist_tile(a.A, D, i, i), DB,
                                         a.Linv + (int64_t)(i - 1) * DB * DB, i, j, smem, s_ok, tid);
            } else if (type == T_BUILD) {
                T* tij = dist_tile(a.A, D, i, j);
                // build_tile_sum addresses element (gi, gj) at base + gi + gj ld (global indices)
                const TileBuild<T>& b = *a.tb;
                const bool bad = pr::build_tile_sum<T, 1, true>(
                    b.Kd, b.FU, b.FV, b.nf, b.Kr, b.Kp, b.hd, tij - (int64_t)i * GT - (int64_t)j * GT * DB, DB, b.n,
                    b.sigma2, (int64_t)i * GT, (int64_t)j * GT, smem, tid);
                if (__builtin_amdgcn_readfirstlane(__any(bad))) atomicOr(a.tb->flag, 1);
                publish(a.ver + (int64_t)i * a.nv + j, 0, false);
            } else if (type == T_UPD) {
                // row j of this rank: its stored tiles; of another rank: the window, one tile per
                // panel (one call site: two inlined mainloops crashed hipcc 7.2)
                const int lj = __builtin_amdgcn_readfirstlane(D.loc[j]);
                const bool loc = lj >= 0;
                const T* Bop = loc ? dist_tile(a.A, D, j, b0) : nullptr;
                const uint64_t* bp = loc ? nullptr : D.tptr + (int64_t)j * D.nc + b0;
                if (D.check && !loc && wv == 0) dist_check_tags(D, j, b0, nb, 0);
                tile_gemm<T, true>(dist_tile(a.A, D, i, j), DB, dist_tile(a.A, D, i, b0), DB, Bop, DB, nb * GT, i == j,
                                   smem, tid, false, bp);
                publish(a.ver + (int64_t)i * a.nv + dist_col(D.nc, j), b0 + nb, false);
                if (D.check && !loc && wv == 0) dist_check_tags(D, j, b0, nb, 1);
                if (!loc && wv == 0) dist_release(D, b0, nb);  // this chunk's window reads are done
            } else if (type == T_TRSM) {
                T* Cik = dist_tile(a.A, D, i, j);
                tile_trsm<T>(Cik, DB, Cik, DB, a.Linv + (int64_t)j * DB * DB, DB, smem, tid);
                publish(a.lcnt + i, j + 1, false);
                if (i == D.nc) {  // the label rows z^T: every other rank's z area (the solves read it)
                    const unsigned all = ((1u << D.g) - 1u) & ~(1u << D.r);
                    dist_push(Cik, D, all, D.o_z + (int64_t)j * DB * DB * (int64_t)sizeof(T),
                              dist_f_tile() + (int64_t)i * D.nc + j, tid);
                } else {
                    const unsigned cm = dist_consumers(D, i);
                    if (wv == 0) ok = dist_wait_release(a, D, cm, j - D.ww);
                    if (wv == 0) s_ok = ok ? 1 : 0;
                    __syncthreads();
                    ok = __builtin_amdgcn_readfirstlane(s_ok) != 0;
                    if (ok)
                        dist_push(Cik, D, cm, -1, dist_f_tile() + (int64_t)i * D.nc + j, tid,
                                  (int64_t)(j % D.ww) * D.nr + i, (D.ep << 16) | (unsigned)(j + 1));
                }
            } else {  // DIAGX(k = i)
                const int k = i;
                T* Akk = dist_tile(a.A, D, k, k);
                T* Akm = k > 0 ? dist_tile(a.A, D, k, k - 1) : nullptr;
                if (k > 0 && a.split) {
                    if constexpr (diag_la<T>) ok = diagx_split<T>(tpc, k, smem, s_ok, tid);
                    else ok = diagx_split_wait<T>(tpc, k, s_ok);
                    if (!ok) break;
                } else if (diag_la<T> && k > 0) {
                    diagx_ts<T>(Akm, Akk, DB, a.Linv + (int64_t)(k - 1) * DB * DB, a.lcnt + k, k, smem, tid, false);
                } else if (k > 0) {
                    tile_trsm<T>(Akm, DB, Akm, DB, a.Linv + (int64_t)(k - 1) * DB * DB, DB, smem, tid);
                    publish(a.lcnt + k, k, false);
                    tile_gemm<T, true, 2>(Akk, DB, Akm, DB, Akm, DB, GT, true, smem, tid);
                    local_sync();
                }
                diag_factor<T>(Akk, DB, a.Linv + (int64_t)k * DB * DB, a.info, (int64_t)k * DB, smem_raw, tid, a.dbg,
                               nullptr, diag_la<T> && k > 0, a.lcnt + k, k + 1);  // (publishes Linv_k locally)
                // pushes after the local publication (this rank's chain goes on meanwhile): the
                // next diagonal step's rank first, L_{k,k-1} before Linv_k
                const unsigned cm = k > 0 ? dist_consumers(D, k) : 0u;
                const unsigned all = ((1u << D.g) - 1u) & ~(1u << D.r);
                const int nx = (k + 1 < D.nc) ? __builtin_amdgcn_readfirstlane(D.own[k + 1]) : D.r;
                const unsigned first = (nx != D.r) ? (1u << nx) : 0u;
                if (k > 0) {
                    if (wv == 0) ok = dist_wait_release(a, D, cm, k - 1 - D.ww);
                    if (wv == 0) s_ok = ok ? 1 : 0;
                    __syncthreads();
                    ok = __builtin_amdgcn_readfirstlane(s_ok) != 0;
                }
                const int64_t owin = -1;  // the window slot tix
                const int64_t olinv = D.o_linv + (int64_t)k * DB * DB * (int64_t)sizeof(T);
                const int64_t tix = (int64_t)((k - 1 + D.ww) % D.ww) * D.nr + k;
                const unsigned tgv = (D.ep << 16) | (unsigned)k;
                if (ok && k > 0)
                    dist_push(Akm, D, cm & first, owin, dist_f_tile() + (int64_t)k * D.nc + (k - 1), tid, tix, tgv);
                if (ok) dist_push(a.Linv + (int64_t)k * DB * DB, D, all & first, olinv, dist_f_linv(D.nr, D.nc) + k, tid);
                if (ok && k > 0)
                    dist_push(Akm, D, cm & ~first, owin, dist_f_tile() + (int64_t)k * D.nc + (k - 1), tid, tix, tgv);
                if (ok) dist_push(a.Linv + (int64_t)k * DB * DB, D, all & ~first, olinv, dist_f_linv(D.nr, D.nc) + k, tid);
            }
            if (!ok) break;
        } else {
        T* Ci = a.A + (int64_t)i * GT;  // row block i, column 0
        // (a failed wait inside a task has raised C_ERR: the task ends on garbage, which the
        // launch reports as info = -1, and the next wait_inputs drains the workgroup)
        if (type == T_TPART) {
            (void)tpart_task<T, false>(tpc, Ci + (int64_t)(i - 1) * GT * ld, Ci + (int64_t)i * GT * ld, ld,
                                       a.Linv + (int64_t)(i - 1) * DB * DB, i, j, smem, s_ok, tid);
        } else if (type == T_BUILD) {
            // ver[i][j] goes from -1 (not built) to 0; the tile's values go out write-through
            // one instantiation for every mode: an absent statistic has a zero-depth product
            // (its accumulators stay 0) and no leaves of its class
            // (inline: out of line, its register saves cost the C3 fit 0.35 ms and the sharded
            // fit 1%, more than the task loop's few spills at task level, none in a mainloop)
            const TileBuild<T>& b = *a.tb;
            const bool bad = pr::build_tile_sum<T, 1, true>(b.Kd, b.FU, b.FV, b.nf, b.Kr, b.Kp, b.hd, a.A, ld, b.n,
                                                            b.sigma2, (int64_t)i * GT, (int64_t)j * GT, smem, tid);
            if (__builtin_amdgcn_readfirstlane(__any(bad))) atomicOr(a.tb->flag, 1);  // wave-uniform branch
            publish(a.ver + (int64_t)i * a.nv + j, 0, false);
        } else if (type == T_UPD) {
            // variant 64 (timing experiment, wrong results): every update streams the same
            // L2-resident operands, to separate memory-feed from MFMA limits
            const int64_t oa = (a.variant & 64) ? 0 : (int64_t)i * GT + (int64_t)b0 * GT * ld;
            const int64_t ob = (a.variant & 64) ? GT : (int64_t)j * GT + (int64_t)b0 * GT * ld;
            // variant 128 (timing experiment, wrong results): operand stride 0 along k, every
            // k-slice of the update re-reads the same 1 KB column -- a truly cache-resident feed
            const int64_t lop = (a.variant & 128) ? 0 : ld;
            // (the narrow label row is a call of its own, not a row bound inside tile_mma's mainloop)
            if (a.variant & 2) {  // (timing experiment: no update math)
            } else if (i == a.nc && a.lab_rows <= LAB_NARROW) {
                tile_gemm_rows16<T>(Ci + (int64_t)j * GT * ld, ld, a.A + oa, lop, a.A + ob, lop, nb * GT, smem, tid);
            } else {
                tile_gemm<T, true>(Ci + (int64_t)j * GT * ld, ld, a.A + oa, lop, a.A + ob, lop, nb * GT, i == j, smem,
                                   tid);
            }
            publish(a.ver + (int64_t)i * a.nv + j, b0 + nb, false);
        } else if (type == T_UPD2) {  // tiles (i, j) and (i + 1, j): one 256 x 128 update
            if (!(a.variant & 2))
                tile_gemm_tall<T>(Ci + (int64_t)j * GT * ld, ld, a.A + (int64_t)i * GT + (int64_t)b0 * GT * ld, ld,
                                  a.A + (int64_t)j * GT + (int64_t)b0 * GT * ld, ld, nb * GT, smem, tid);
            publish2(a.ver + (int64_t)i * a.nv + j, a.ver + (int64_t)(i + 1) * a.nv + j, b0 + nb);
        } else if (type == T_TRSM) {
            T* Cik = Ci + (int64_t)j * GT * ld;
            if (!(a.variant & 1))
                tile_trsm<T>(Cik, ld, Cik, ld, a.Linv + (int64_t)j * DB * DB, DB, smem, tid);
            publish(a.lcnt + i, j + 1, false);
        } else {  // DIAGX(k = i)
            const int k = i;
            T* Akk = Ci + (int64_t)k * GT * ld;
            long long dt[4] = {0, 0, 0, 0};
            if (k > 0 && a.split) {
                if constexpr (diag_la<T>) (void)diagx_split<T>(tpc, k, smem, s_ok, tid);
                else (void)diagx_split_wait<T>(tpc, k, s_ok);
                if (a.trace) dt[0] = dt[1] = wall_clock64();
            } else if (diag_la<T> && k > 0) {
                T* Akm = Ci + (int64_t)(k - 1) * GT * ld;
                dt[0] = diagx_ts<T>(Akm, Akk, ld, a.Linv + (int64_t)(k - 1) * DB * DB, a.lcnt + k, k, smem, tid,
                                    a.trace != nullptr);
                dt[1] = dt[0];
            } else if (k > 0) {
                T* Akm = Ci + (int64_t)(k - 1) * GT * ld;
                tile_trsm<T>(Akm, ld, Akm, ld, a.Linv + (int64_t)(k - 1) * DB * DB, DB, smem, tid);
                if (a.trace) dt[0] = wall_clock64();
                publish(a.lcnt + k, k, false);  // L_{k,k-1} final: unblocks the updates of column k
                if (a.trace) dt[1] = wall_clock64();
                tile_gemm<T, true, 2>(Akk, ld, Akm, ld, Akm, ld, GT, true, smem, tid);
                local_sync();
            }
            if (a.trace) dt[2] = wall_clock64();
            diag_factor<T>(Akk, ld, a.Linv + (int64_t)k * DB * DB, a.info, (int64_t)k * DB, smem_raw, tid, a.dbg,
                           a.trace ? a.trace + 4 * (int64_t)(a.ntasks + a.nc) + 4 * (int64_t)k : nullptr,
                           diag_la<T> && k > 0, a.lcnt + k, k + 1);  // (publishes Linv_k: lcnt[k] = k + 1)
            if (a.trace) dt[3] = wall_clock64();
            if (a.trace && wv == 0) {
                long long* dp = a.trace + 4 * (int64_t)a.ntasks + 4 * (int64_t)k;
                for (int u = 0; u < 4; u++) dp[u] = dt[u];
            }
        }
        }
        if (a.trace && wv == 0) {
            long long* tp = a.trace + 4 * (int64_t)q;
            tp[0] = tr0;
            tp[1] = tr1;
            tp[2] = wall_clock64();
            tp[3] = (long long)blockIdx.x | (((long long)__builtin_amdgcn_s_memtime() - tc1) << 16);
        }
    }
    dbg_mark(a.dbg, -1, 9, 0, 0);
    // the error flag of a timed-out wait ends up in info (reported by the caller)
    if (wv == 0 && ld_agent(a.ctl + C_ERR)) atomicMin(a.info, -1);
}

}  // namespace pt

// Per-context state: cached schedules (host + device copies) and the counter block.
struct PtState {
    struct Dev {
        int4* list = nullptr;
        int64_t n = 0;
        double est_us = 0;
        bool ident_even = false;  // (Schedule::ident_even)
        std::vector<int4> host;
    };
    std::map<std::tuple<int, int, bool, int, bool, int>, Dev> sched;  // (nc, nr, fused, ni, split, sizeof(T))
    int* ctr = nullptr;
    void* pbuf = nullptr;  // the split diagonal step's four TPART products (DB x DB each)
    size_t ctr_ints = 0;
    int ncu = 0;
    int* dbg = nullptr;  // pinned host status words (GPRX_PT_DEBUG)
    long long* trace = nullptr;  // GPRX_PT_TRACE timeline of the last launch (+ DIAGX phases)
    int64_t trace_n = 0, trace_nc = 0;
    const std::vector<int4>* last_list = nullptr;
    void* tb = nullptr;  // device copy of the launch's TileBuild
    std::vector<unsigned char> tb_last;  // its bytes (re-uploaded only when they change)
    ~PtState() {
        if (tb) (void)hipFree(tb);
        if (pbuf) (void)hipFree(pbuf);
        if (trace) (void)hipFree(trace);
        if (dbg) (void)hipHostFree(dbg);
        for (auto& kv : sched) (void)hipFree(kv.second.list);
        if (ctr) (void)hipFree(ctr);
    }
};

void pt_state_free(PtState* p) { delete p; }

// timeline of the last traced launch (GPRX_PT_TRACE): per ticket {type|nb<<8, i, j, b0} and
// {taken, ready, published, workgroup} (100 MHz wall clock)
static PtState* g_pt_state = nullptr;
int64_t pt_trace_copy(int32_t* tasks, long long* times, int64_t max) {
    if (!g_pt_state || !g_pt_state->trace || !g_pt_state->last_list) return 0;
    // rows: one per ticket, then nc DIAGX phase rows, nc diagonal-factor rows, 4 nc TPART stamp rows,
    // nc split-DIAGX stamp rows
    const int64_t n = std::min<int64_t>(max, g_pt_state->trace_n + 7 * g_pt_state->trace_nc);
    GPRX_HIP(hipDeviceSynchronize());
    GPRX_HIP(hipMemcpy(times, g_pt_state->trace, sizeof(long long) * 4 * n, hipMemcpyDeviceToHost));
    const int64_t nl = std::min<int64_t>(n, (int64_t)g_pt_state->last_list->size());
    std::memcpy(tasks, g_pt_state->last_list->data(), sizeof(int4) * nl);
    return n;
}

// debug snapshot of the last launch's per-workgroup status (GPRX_PT_DEBUG)
static int* g_pt_dbg = nullptr;
static int g_pt_dbg_n = 0;
static std::mutex g_pt_dbg_mu;
int pt_debug_snapshot(int* out, int max_wg) {
    std::lock_guard<std::mutex> lk(g_pt_dbg_mu);
    if (!g_pt_dbg) return 0;
    const int n = std::min(max_wg, g_pt_dbg_n);
    for (int k = 0; k < 4 * n; k++) out[k] = __atomic_load_n(g_pt_dbg + k, __ATOMIC_RELAXED);
    return n;
}
// a distributed rank's launch (GPRX_PT_DEBUG, one rank per process): its status words, owned by
// the engine; n = 0 unregisters `dbg` if it is the registered buffer (the engine's teardown)
void pt_debug_register(int* dbg, int n) {
    std::lock_guard<std::mutex> lk(g_pt_dbg_mu);
    if (n > 0) {
        g_pt_dbg = dbg;
        g_pt_dbg_n = n;
    } else if (g_pt_dbg == dbg) {
        g_pt_dbg = nullptr;
        g_pt_dbg_n = 0;
    }
}

// ctr[i] = -1 for i in [v0, v1), 0 elsewhere (i < n)
__global__ void pt_init_counters(int* __restrict__ ctr, int64_t n, int64_t v0, int64_t v1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ctr[i] = (i >= v0 && i < v1) ? -1 : 0;
}

// counters of the identity row blocks (the inverse riding along): block a = i - nr0 has its
// first a panels "applied" (they are zero) and its first a L blocks "final"
// (even: the schedule pairs the identity rows, Schedule::ident_even -- an odd block's updates,
// and so its ver counters, start one panel early)
__global__ void pt_init_identity_counters(int* __restrict__ lcnt, int* __restrict__ ver, int nc, int nr0, int ni,
                                          int even) {
    const int a = blockIdx.x, j = threadIdx.x;
    if (a >= ni) return;
    if (j == 0) lcnt[nr0 + a] = a;
    const int v = even ? a - (a & 1) : a;
    for (int c = j; c < nc; c += blockDim.x) ver[(int64_t)(nr0 + a) * nc + c] = v;
}

// identity rows: A[row0 + r][c] = (r == c) for the columns at or right of r's block (even: an
// odd block from the block left of its own, a zero tile its paired updates read)
template <typename T>
__global__ void pt_init_identity_rows(T* __restrict__ A, int64_t ld, int64_t row0, int64_t nid, int64_t ncol,
                                      int even) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t c = blockIdx.y;
    const int64_t rb = r / GT, c0 = (even ? rb - (rb & 1) : rb) * GT;
    if (r >= nid || c >= ncol || c < c0) return;
    A[row0 + r + c * ld] = (r == c) ? T(1) : T(0);
}

template <typename T>
void potrf_tiles(T* A, int64_t ld, int64_t np, int64_t nrows, T* Linv, int* info, Exec& ex, const TileBuild<T>* build,
                 int ni, bool build_only, int lab_live) {
    using namespace pt;
    if (!ex.pt) ex.pt = new PtState();
    PtState& st = *ex.pt;
    if (st.ncu == 0) {
        int dev = 0;
        GPRX_HIP(hipGetDevice(&dev));
        hipDeviceProp_t prop;
        GPRX_HIP(hipGetDeviceProperties(&prop, dev));
        st.ncu = prop.multiProcessorCount;
    }
    GPRX_REQUIRE(np % DB == 0 && nrows % GT == 0 && nrows >= np, GPRX_ERR_ARG, "potrf_tiles: bad sizes");
    const int nc = (int)(np / DB), nr = (int)(nrows / GT);
    const bool fused = build && build->mode != 0;
    GPRX_REQUIRE(ni >= 0 && ni <= nr - nc, GPRX_ERR_ARG, "potrf_tiles: bad identity row blocks");
    GPRX_REQUIRE(!build_only || fused, GPRX_ERR_ARG, "potrf_tiles: build_only needs a fused build");
    // build_only (a parity hook, gprx_dev_build_matrix): the ticket list holds the BUILD tasks
    // alone, so the launch writes exactly the covariance tiles the fused factorisation starts from
    const bool split = split_for(std::is_same<T, double>::value, st.ncu);
    // the narrow label row: one label row block with at most LAB_NARROW live rows (GPRX_PT_LABEL=0: off)
    const bool narrow = !build_only && lab_live <= LAB_NARROW && nr - ni == nc + 1 && params().label != 0;
    auto key = std::make_tuple(nc, nr, fused, build_only ? -1 : ni, split, (int)sizeof(T) | (narrow ? 256 : 0));
    auto it = st.sched.find(key);
    if (it == st.sched.end()) {
        const Params& pr = params();
        Schedule S;
        if (build_only) {
            for (int i = 0; i < nc; i++)
                for (int j = 0; j <= i; j++) S.list.push_back(make_int4(T_BUILD, i, j, 0));
        } else {
            S = best_schedule(nc, nr, pr, st.ncu, fused, ni, split, std::is_same<T, double>::value, narrow);
        }
        PtState::Dev d;
        d.n = (int64_t)S.list.size();
        d.est_us = S.est_us;
        d.ident_even = S.ident_even;
        GPRX_HIP(dev_malloc(&d.list, sizeof(int4) * std::max<int64_t>(1, d.n)));
        GPRX_HIP(hipMemcpy(d.list, S.list.data(), sizeof(int4) * d.n, hipMemcpyHostToDevice));
        d.host = S.list;
        it = st.sched.emplace(key, d).first;
    }
    const PtState::Dev& sd = it->second;
    const size_t need = (size_t)C_NCTL + nr + (size_t)nr * nc + TP_STRIDE * (size_t)nc;  // + the split step's states
    if (st.ctr_ints < need) {
        if (st.ctr) GPRX_HIP(hipFree(st.ctr));
        st.ctr = nullptr;
        GPRX_HIP(dev_malloc(&st.ctr, sizeof(int) * need));
        st.ctr_ints = need;
    }
    hipStream_t s = ex.s0;
    // counters zeroed, and (fused build) ver = -1 (not built) for the tiles of the leading
    // block (the label rows are built): one launch (the two memsets of odd sizes were five
    // fill kernels, each with its dispatch gap, on every fit)
    {
        const int64_t v0 = fused ? (int64_t)C_NCTL + nr : 0, v1 = fused ? v0 + (int64_t)nc * nc : 0;
        hipLaunchKernelGGL(pt_init_counters, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, s, st.ctr,
                           (int64_t)need, v0, v1);
        GPRX_HIP(hipGetLastError());
    }
    if (ni > 0) {
        hipLaunchKernelGGL(pt_init_identity_counters, dim3((unsigned)ni), dim3(128), 0, s, st.ctr + C_NCTL,
                           st.ctr + C_NCTL + nr, nc, nr - ni, ni, sd.ident_even ? 1 : 0);
        hipLaunchKernelGGL(pt_init_identity_rows<T>, dim3((unsigned)((ni * (int64_t)GT + 255) / 256), (unsigned)np),
                           dim3(256), 0, s, A, ld, (int64_t)(nr - ni) * GT, (int64_t)ni * GT, np, sd.ident_even ? 1 : 0);
    }
    Args<T> a;
    a.A = A;
    a.ld = ld;
    a.Linv = Linv;
    a.tasks = sd.list;
    a.ntasks = (int)sd.n;
    a.nc = nc;
    a.nv = nc;
    a.ctl = st.ctr;
    a.lcnt = st.ctr + C_NCTL;
    a.ver = st.ctr + C_NCTL + nr;
    a.info = info;
    a.tb = nullptr;
    a.dist = nullptr;
    a.split = split ? 1 : 0;
    a.tflag = st.ctr + C_NCTL + nr + (size_t)nr * nc;
    if (split && !st.pbuf) GPRX_HIP(dev_malloc(&st.pbuf, sizeof(T) * 4 * DB * DB));
    a.pbuf = static_cast<T*>(st.pbuf);
    a.lab_rows = narrow ? lab_live : GT;
    if (fused) {
        GPRX_REQUIRE(build->nf == np, GPRX_ERR_ARG, "potrf_tiles: build features must have np rows");
        if (!st.tb) GPRX_HIP(dev_malloc(&st.tb, sizeof(TileBuild<double>)));
        // (a pageable copy blocks the host until the stream reaches it: skipped when unchanged)
        const unsigned char* tbb = reinterpret_cast<const unsigned char*>(build);
        if (st.tb_last.size() != sizeof(TileBuild<T>) || std::memcmp(st.tb_last.data(), tbb, sizeof(TileBuild<T>)) != 0) {
            GPRX_HIP(hipMemcpyAsync(st.tb, build, sizeof(TileBuild<T>), hipMemcpyHostToDevice, s));
            st.tb_last.assign(tbb, tbb + sizeof(TileBuild<T>));
        }
        a.tb = reinterpret_cast<const TileBuild<T>*>(st.tb);
    }
    a.dbg = nullptr;
    a.trace = nullptr;
    a.xt = nullptr;
    static const bool tracing = std::getenv("GPRX_PT_TRACE") != nullptr;
    if (tracing) {
        if (st.trace_n + 7 * st.trace_nc < sd.n + 7 * nc) {  // + the split step's 5 nc stamp rows
            if (st.trace) GPRX_HIP(hipFree(st.trace));
            GPRX_HIP(dev_malloc(&st.trace, sizeof(long long) * 4 * (sd.n + 7 * nc)));
        }
        st.trace_n = sd.n;
        st.trace_nc = nc;
        a.trace = st.trace;
        a.xt = st.trace + 4 * (sd.n + 2 * nc);
        GPRX_HIP(hipMemsetAsync(a.xt, 0, sizeof(long long) * 4 * 5 * nc, s));
        g_pt_state = &st;
        st.last_list = &sd.host;
    }
    static const int variant = std::getenv("GPRX_PT_VARIANT") ? std::atoi(std::getenv("GPRX_PT_VARIANT")) : 0;
    a.variant = variant;
    static const bool debug = std::getenv("GPRX_PT_DEBUG") != nullptr;
    if (debug) {
        if (!st.dbg) GPRX_HIP(hipHostMalloc((void**)&st.dbg, sizeof(int) * 4 * st.ncu, hipHostMallocCoherent));
        std::memset(st.dbg, 0xff, sizeof(int) * 4 * st.ncu);
        g_pt_dbg = st.dbg;
        g_pt_dbg_n = st.ncu;
        a.dbg = st.dbg;
    }
    // one wait may take at most 2 s + 20x the whole predicted factorisation
    a.tlimit = (long long)(1e8 * (2.0 + 20.0 * sd.est_us * 1e-6));
    // + the ticket word; at least 96 KB so the launch stays at one workgroup per CU
    auto lds_of = [](size_t b) { return std::max<size_t>(b, 96 * 1024); };
    const size_t lds = lds_of(pt_lds_total<T>());
    static bool attr = false;
    if (!attr) {
        GPRX_HIP(hipFuncSetAttribute((const void*)potrf_tiles_kernel<double, false>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(pt_lds_total<double>())));
        GPRX_HIP(hipFuncSetAttribute((const void*)potrf_tiles_kernel<float, false>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(pt_lds_total<float>())));
        attr = true;
    }
    const double nn = (double)np;
    ProfScope ps(KC_TILES, s,
                 nn * nn * nn / 3.0 + (double)(nrows - np - (int64_t)ni * GT) * nn * nn + (ni ? nn * nn * nn / 3.0 : 0.0),
                 0.0);
    hipLaunchKernelGGL((potrf_tiles_kernel<T, false>), dim3((unsigned)st.ncu), dim3(NT), lds, s, a);
    GPRX_HIP(hipGetLastError());
}

// ---- distributed factorisation: one rank's launch ------------------------------------------------
template <typename T>
void potrf_tiles_dist_launch(const DistLaunch<T>& L) {
    using namespace pt;
    Args<T> a;
    std::memset(&a, 0, sizeof(a));
    a.A = L.A;
    a.ld = DB;
    a.Linv = L.Linv;
    a.tasks = L.list;
    a.ntasks = L.ntasks;
    a.nc = L.nc;
    a.nv = L.nci;
    a.ctl = L.ctr;
    a.lcnt = L.ctr + C_NCTL;
    a.ver = L.ctr + C_NCTL + L.nr;
    a.info = L.info;
    a.tlimit = L.tlimit;
    a.tb = L.tb_dev;
    a.dist = L.dist_dev;
    a.dbg = L.dbg;
    a.trace = L.trace;
    a.xt = nullptr;
    a.split = L.split;
    a.pbuf = L.pbuf;
    a.tflag = L.tflag;
    a.lab_rows = GT;  // (the sharded engine's label rows keep the full tile)
    auto lds_of = [](size_t b) { return std::max<size_t>(b, 96 * 1024); };
    const size_t lds = lds_of(pt_lds_total<T>());
    static bool attr = false;
    if (!attr) {
        GPRX_HIP(hipFuncSetAttribute((const void*)potrf_tiles_kernel<double, true>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(pt_lds_total<double>())));
        GPRX_HIP(hipFuncSetAttribute((const void*)potrf_tiles_kernel<float, true>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(pt_lds_total<float>())));
        attr = true;
    }
    hipLaunchKernelGGL((potrf_tiles_kernel<T, true>), dim3((unsigned)L.P), dim3(NT), lds, L.s, a);
    GPRX_HIP(hipGetLastError());
}
template void potrf_tiles_dist_launch<double>(const DistLaunch<double>&);
template void potrf_tiles_dist_launch<float>(const DistLaunch<float>&);

template void potrf_tiles<double>(double*, int64_t, int64_t, int64_t, double*, int*, Exec&, const TileBuild<double>*,
                                  int, bool, int);
template void potrf_tiles<float>(float*, int64_t, int64_t, int64_t, float*, int*, Exec&, const TileBuild<float>*, int,
                                 bool, int);

}  // namespace gprx
