// k_append.hip — thin-panel forward substitution V L^T = R in ONE launch (gfx950).
//
// Appending samples to a fitted model (gprx_model_append, gprx_api.cpp) needs two solves of a
// panel of at most 128 right-hand sides against a large factor: the new samples' rows
// K(Xnew, X) L00^{-T} of the factor, and the labels z = L^{-1} Y against the whole new factor.
// trsm_rows (k_predict.hip) takes ~2 N / 128 GEMM launches of mostly one output tile for such a
// panel, forward_chain_kernel (k_bsolve.hip) one launch but a VALU GEMV and a pass over L per
// right-hand side.  Here the panel is one MFMA operand:
//     V_b = (R_b - sum_{j < b} V_j L_bj^T) Linv_b^T                 (128-column blocks b)
// with one workgroup per block b.  R is column-major (rows x ncols, ldr), so V_j is 128
// columns of `rows` values; the eight waves own 16 output columns each and all the panel's
// 16-row groups: per streamed tile L_bj a lane keeps its 32 operand values (row 16 w + lr,
// k-columns 4 q + lk) in registers and V_j comes through LDS.
//
// Blocks are claimed first block first and chained by the hand-off protocol of k_handoff.h
// (tickets, sc1 stores and loads, one flag per block, bounded waits).  Specific to this file:
// the loads of tile L_bj go out before V_j is waited for (and tile j + 1's before tile j is
// multiplied); every consuming wave polls the flag itself; the launch asks for more than half a
// CU's LDS, so one workgroup per CU (the table's first row requires it).
#include "gprx_internal.h"
#include "k_handoff.h"
#include "k_mma.h"

#include <algorithm>
#include <cstring>

namespace gprx {

namespace ap {

using namespace ho;

constexpr int NT = 512;  // 8 waves
constexpr size_t LDS_MIN = 84 * 1024;  // more than half of the CU's 160 KB: one workgroup per CU

// LDS leading dimension of a staged panel of RG 16-row groups: the four k-columns a fragment
// read touches (lk = 0..3) land 16 elements apart modulo 32
constexpr int ldv_of(int RG) { return (RG * 16) % 32 == 16 ? RG * 16 : RG * 16 + 16; }
template <typename T, int RG>
constexpr size_t panel_lds() {
    const size_t need = sizeof(T) * (size_t)DB * ldv_of(RG) * (RG <= 2 ? 2 : 1);
    return need > LDS_MIN ? need : LDS_MIN;
}

// Wait until *f != 0; false on timeout or another workgroup's error (every wave polls on its
// own and the workgroup agrees through LDS at its next barrier).
__device__ __forceinline__ bool wait_flag(const int* f, int* ctl, long long t0, long long tlimit) {
    // (the error word and the clock every 16th poll: each is a round trip of its own between two
    // looks at the flag)
    return wait_until<1, 16>([=] { return ld_uni(f) != 0; }, ctl + C_ERR, t0, tlimit);
}

template <typename T>
struct Args {
    const T* A;       // factor, column-major, ld: tile (b, j) at A + 128 b + 128 j ld
    int64_t ld;
    int nb;           // 128-column blocks
    const T* Linv;    // DB x DB inverse of each diagonal block, column-major
    T* R;             // the panel: rows x 128 nb, column-major, ldr; solved in place
    int64_t ldr;
    int rows;         // <= 16 RG; rows beyond it are neither read nor written
    int* ctl;         // [C_NCTL] then one flag per block
    int* info;        // set to -1 (atomicMin) when a wait timed out
    long long tlimit; // wall-clock ticks (100 MHz) per wait
    long long* trace; // GPRX_BS_TRACE: per block {start, streamed tiles done, V_{b-1} seen, published}
};

// A lane's operand values of one 128 x 128 tile: row 16 w + lr, k-columns 4 q + lk
template <typename T>
struct TileFrag {
    T x[32];
    __device__ __forceinline__ void load(const T* __restrict__ tile, int64_t ld, int w, int lr, int lk) {
        const T* p = tile + 16 * w + lr + (int64_t)lk * ld;
#pragma unroll
        for (int q = 0; q < 32; q++) x[q] = p[(int64_t)(4 * q) * ld];
    }
};

template <typename T, int RG>
__global__ __launch_bounds__(NT) void forward_panel_kernel(Args<T> a) {
    typedef mm::Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    constexpr int LDV = ldv_of(RG);
    constexpr int R16 = RG * 16;
    constexpr bool DBUF = RG <= 2;          // two stage buffers: one barrier per streamed tile
    constexpr int SBUF = DB * LDV;
    // tile j + 1's operand registers beside tile j's (64 more f64 VGPRs) while the accumulators
    // leave room; wider f64 panels load each tile at the top of its own step
    constexpr bool PRE = sizeof(T) * RG <= 16;
    // the thinnest panels also hold the diagonal block's inverse and R_b from the start: their
    // loads are off the chain (behind V_{b-1} they were a global round trip per block)
    constexpr bool EARLY = sizeof(T) * RG <= 8;
    __shared__ int s_int[3];                // ticket, fail word of even / odd streamed tiles
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* s_v = reinterpret_cast<T*>(smem_raw);  // staged panel block: (row r, k-column kk) at kk LDV + r
    const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int lr = lane & 15, lk = lane >> 4;
    int* flags = a.ctl + C_NCTL;
    if (w == 0) {
        s_int[1] = 0;
        s_int[2] = 0;
    }
    const int b = claim_ticket(a.ctl, &s_int[0]);
    if (b >= a.nb) return;
    if (a.trace && t == 0) a.trace[4 * b] = wall_clock64();
    const long long t0 = wall_clock64();

    acc_t acc[RG];
#pragma unroll
    for (int g = 0; g < RG; g++) acc[g] = acc_t{0};

    // acc[g][reg] += sum_kk tile(16 w + orow(lk, reg), kk) * staged(16 g + lr, kk)
    auto multiply = [&](const TileFrag<T>& f, const T* sv) {
#pragma unroll
        for (int q = 0; q < 32; q++) {
            const T* col = sv + (4 * q + lk) * LDV + lr;
#pragma unroll
            for (int g = 0; g < RG; g++) acc[g] = Tr::mma(f.x[q], col[16 * g], acc[g]);
        }
    };
    // block j of the panel (published by its workgroup: sc1 loads only) into a stage buffer
    auto stage_block = [&](int j, T* sv) {
        const T* src = a.R + (int64_t)j * DB * a.ldr;
#pragma unroll
        for (int i = 0; i < R16 * DB / NT; i++) {
            const int e = t + NT * i, r = e % R16, kk = e / R16;
            sv[kk * LDV + r] = (r < a.rows) ? ld_sc1(src + r + (int64_t)kk * a.ldr) : T(0);
        }
    };

    const T* rowA = a.A + (int64_t)b * DB;  // tile (b, j) at rowA + 128 j ld
    T* Rb = a.R + (int64_t)b * DB * a.ldr;
    TileFrag<T> fd;
    T rb[RG][4];
    auto load_rb = [&]() {
#pragma unroll
        for (int g = 0; g < RG; g++) {
            const int r = 16 * g + lr;
#pragma unroll
            for (int reg = 0; reg < 4; reg++)
                rb[g][reg] = (r < a.rows) ? Rb[r + (int64_t)(16 * w + Tr::orow(lk, reg)) * a.ldr] : T(0);
        }
    };
    if (EARLY) {
        fd.load(a.Linv + (int64_t)b * DB * DB, DB, w, lr, lk);
        load_rb();
    }
    bool ok = true;
    // One streamed tile: its loads are already in flight in `cur`; the next tile's go out into
    // `nxt` before this one is multiplied.  Every wave runs the same barriers whether its wait
    // failed or not, and all leave together.
    auto step = [&](int j, TileFrag<T>& cur, TileFrag<T>& nxt) -> bool {
        T* sv = s_v + (DBUF ? (j & 1) * SBUF : 0);
        if (!PRE) cur.load(rowA + (int64_t)j * DB * a.ld, a.ld, w, lr, lk);
        ok = wait_flag(flags + j, a.ctl, t0, a.tlimit);
        if (!ok) s_int[1 + (j & 1)] = 1;
        if (!DBUF) __syncthreads();  // the previous tile's fragment reads are done
        if (ok) stage_block(j, sv);
        __builtin_amdgcn_sched_barrier(0);  // (the next tile's loads stay behind the staged block's)
        if (PRE && j + 1 < b) nxt.load(rowA + (int64_t)(j + 1) * DB * a.ld, a.ld, w, lr, lk);
        __syncthreads();
        if (s_int[1 + (j & 1)]) return false;
        multiply(cur, sv);
        return true;
    };
    {
        TileFrag<T> f0, f1;
        if (PRE && b > 0) f0.load(rowA, a.ld, w, lr, lk);
        int j = 0;
        if constexpr (PRE) {
            for (; j + 1 < b; j += 2) {
                if (!step(j, f0, f1)) {
                    ok = false;
                    break;
                }
                if (!step(j + 1, f1, f0)) {
                    ok = false;
                    break;
                }
            }
            if (ok && j < b && !step(j, f0, f1)) ok = false;
        } else {
            for (; j < b; j++)
                if (!step(j, f0, f0)) {
                    ok = false;
                    break;
                }
        }
    }
    if (ok) {
        if (a.trace && t == 0) a.trace[4 * b + 1] = a.trace[4 * b + 2] = wall_clock64();
        // v = R_b - acc into the stage buffer, then V_b = v Linv_b^T (the same product with the
        // diagonal block's inverse as the tile)
        if (!EARLY) fd.load(a.Linv + (int64_t)b * DB * DB, DB, w, lr, lk);
        __syncthreads();  // the last tile's fragment reads are done
#pragma unroll
        for (int g = 0; g < RG; g++) {
            const int r = 16 * g + lr;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int c = 16 * w + Tr::orow(lk, reg);
                const T rv = EARLY ? rb[g][reg] : ((r < a.rows) ? Rb[r + (int64_t)c * a.ldr] : T(0));
                s_v[c * LDV + r] = rv - acc[g][reg];
                acc[g][reg] = 0;
            }
        }
        __syncthreads();
        multiply(fd, s_v);
#pragma unroll
        for (int g = 0; g < RG; g++) {
            const int r = 16 * g + lr;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int c = 16 * w + Tr::orow(lk, reg);
                if (r < a.rows) st_sc1(Rb + r + (int64_t)c * a.ldr, acc[g][reg]);
            }
        }
        // the publish of k_handoff.h with the flag stored from ONE lane (the guide's first row; no
        // loop follows it here): publish_flag's wave-0 form cost the 8-group f64 panel, which sits
        // at 256 VGPRs, a 12-byte spill
        local_sync();
        if (t == 0) {
            st_agent(flags + b, 1);
            if (a.trace) a.trace[4 * b + 3] = wall_clock64();
        }
    }
    if (t == 0 && ld_uni(a.ctl + C_ERR)) atomicMin(a.info, -1);
}

// rows [0, rows) of the panel P (ldp) into rows r0 .. of A (ld), columns [0, ncols)
template <typename T>
__global__ void panel_rows_kernel(const T* __restrict__ P, int64_t ldp, int64_t rows, int64_t ncols, T* __restrict__ A,
                                  int64_t ld, int64_t r0) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * ncols) return;
    const int64_t r = e % rows, c = e / rows;
    A[r0 + r + c * ld] = P[r + c * ldp];
}

// S (lower tiles of an n x n block, lds) += the P split-K partials (n x n each, ld n), in order
template <typename T>
__global__ void schur_sum_kernel(T* __restrict__ S, int64_t lds, const T* __restrict__ part, int64_t n, int P) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int64_t i = e % n, j = e / n;
    if (i / DB < j / DB) return;  // (tiles above the diagonal are not computed)
    T v = S[i + j * lds];
    for (int p = 0; p < P; p++) v += part[(int64_t)p * n * n + e];
    S[i + j * lds] = v;
}

}  // namespace ap

// GPRX_BS_TRACE timeline of the last panel launch
static BlockTrace g_ap_trace;
int64_t ap_trace_copy(long long* out, int64_t max_blocks) { return g_ap_trace.copy(out, max_blocks); }

template <typename T, int RG>
static void launch_panel_rg(const ap::Args<T>& a, hipStream_t s) {
    using namespace ap;
    static bool attr = false;
    const size_t lds = panel_lds<T, RG>();
    if (!attr) {
        const void* fn = (const void*)forward_panel_kernel<T, RG>;
        GPRX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = true;
    }
    hipLaunchKernelGGL((forward_panel_kernel<T, RG>), dim3((unsigned)a.nb), dim3(NT), lds, s, a);
    GPRX_HIP(hipGetLastError());
}

template <typename T>
void launch_forward_panel_chain(const T* A, int64_t ldA, int64_t ncols, const T* Linv, T* R, int64_t ldr, int rows,
                                int* info, Exec& ex, hipStream_t s) {
    using namespace ap;
    GPRX_REQUIRE(ncols >= 0 && ncols % DB == 0 && rows >= 0 && rows <= DB && ldr >= rows && ldA >= ncols, GPRX_ERR_ARG,
                 "launch_forward_panel_chain: bad sizes");
    if (ncols == 0 || rows == 0) return;
    const int nb = (int)(ncols / DB);
    const size_t need = (size_t)C_NCTL + (size_t)nb;
    int* scratch = ex.scratch_ints(need);
    ProfScope ps(KC_TRSM, s, (double)rows * ncols * ncols, (double)sizeof(T) * ncols * (ncols + 1) / 2.0);
    GPRX_HIP(hipMemsetAsync(scratch, 0, sizeof(int) * need, s));
    Args<T> a;
    std::memset(&a, 0, sizeof(a));
    a.A = A;
    a.ld = ldA;
    a.nb = nb;
    a.Linv = Linv;
    a.R = R;
    a.ldr = ldr;
    a.rows = rows;
    a.ctl = scratch;
    a.info = info;
    a.tlimit = CHAIN_TLIMIT_TICKS;
    static const bool tracing = std::getenv("GPRX_BS_TRACE") != nullptr;
    if (tracing) a.trace = g_ap_trace.ensure(nb);
    const int rg = (rows + 15) / 16;
    if (rg <= 1) launch_panel_rg<T, 1>(a, s);
    else if (rg <= 2) launch_panel_rg<T, 2>(a, s);
    else if (rg <= 4) launch_panel_rg<T, 4>(a, s);
    else launch_panel_rg<T, 8>(a, s);
}

template <typename T>
void launch_panel_rows(const T* P, int64_t ldp, int64_t rows, int64_t ncols, T* A, int64_t ld, int64_t r0,
                       hipStream_t s) {
    const int64_t e = rows * ncols;
    if (e <= 0) return;
    hipLaunchKernelGGL(ap::panel_rows_kernel<T>, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, P, ldp, rows,
                       ncols, A, ld, r0);
    GPRX_HIP(hipGetLastError());
}

template <typename T>
void launch_schur_sum(T* S, int64_t lds, const T* part, int64_t n, int P, hipStream_t s) {
    const int64_t e = n * n;
    if (e <= 0 || P <= 0) return;
    hipLaunchKernelGGL(ap::schur_sum_kernel<T>, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, S, lds, part, n, P);
    GPRX_HIP(hipGetLastError());
}

#define GPRX_INST(T)                                                                                               \
    template void launch_forward_panel_chain<T>(const T*, int64_t, int64_t, const T*, T*, int64_t, int, int*, Exec&, \
                                                hipStream_t);                                                       \
    template void launch_panel_rows<T>(const T*, int64_t, int64_t, int64_t, T*, int64_t, int64_t, hipStream_t);   \
    template void launch_schur_sum<T>(T*, int64_t, const T*, int64_t, int, hipStream_t);
GPRX_INST(double)
GPRX_INST(float)
#undef GPRX_INST

}  // namespace gprx
