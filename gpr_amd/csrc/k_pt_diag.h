// k_pt_diag.h — the 128 x 128 diagonal factors of the tile-dataflow factorisation (k_ptiles.hip):
// A_kk = L L^T in place and Linv = L^{-1}, by one workgroup of 512 threads.  Three forms:
//   diag_factor_rank8    the block as a register image, rank-8 steps (the f32 factor)
//   diag_factor_blocked  32-column panels through an LDS image (f64; the microbenchmark only)
//   diag_factor_la       the same with look-ahead: wave 0 factors block p (fact32) while the
//                        others finish panel p-1's side work (the f64 factor)
// diag_factor picks by precision (pt_sched.h diag_la) and is the task loop's out-of-line entry;
// diag_bench_kernel (k_ptiles.hip, tests/test_gpu_diag.py) runs all three.
#pragma once
#include "k_pt_ops.h"

namespace gprx {
namespace pt {

// ------------------------------------------------------------------------------------------
// Diagonal 128x128 block: L (in place, lower) and Linv (DB x DB, column-major), 512 threads.
//
// The block lives in REGISTERS as a square image S: lower triangle = A (becoming L), strict
// upper triangle = rows of B = L^{-T} (diagonal in Bd).  B comes from the identity appended
// below A riding along the elimination; being upper triangular it fills the unused half.
// Thread t owns rows R0..R0+3 (R0 = 4*(lane&31)) of the 8-column block cb = 2w + (lane>>5).
// Right-looking over 8-column steps:
//   1  waves 0-1 (one row each) factor the 8x8 pivot redundantly (rsq + Newton, no divide)
//      and solve their row x = v Ld^{-T}, v read from the column block published in sV;
//   2  threads with trailing columns apply S -= x_r x_c^T (unmasked: right of the diagonal
//      in rows not yet reached is scratch, zeroed when those rows become pivot rows); the
//      owners of the next column block publish it.
// The image is then staged through LDS so L and Linv leave in coalesced column stores.
// ------------------------------------------------------------------------------------------
constexpr int SPL = DB + 4;
constexpr int SIL = DB + 2;

// v_rsq_f64 (relative error ~2^-23) refined by ONE Halley step, y (1 + e/2 + 3e^2/8) with
// e = 1 - x y^2 (cubic convergence: error ~2^-69 before rounding): 4 dependent f64 operations
// after the rsq against the 6 of two Newton steps -- the pivot chain is latency-bound
__device__ __forceinline__ double rsqrt_full(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    const double e = fma(-x * y, y, 1.0);
    return fma(y * e, fma(e, 0.375, 0.5), y);
}
__device__ __forceinline__ float rsqrt_full(float x) {
    float y = __builtin_amdgcn_rsqf(x);
    const float h = 0.5f * x;
    y = y * fmaf(-h * y, y, 1.5f);
    return y;
}

template <typename T>
constexpr size_t diag_lds() {
    // (DB + 2 diagonal words: diag_factor_la keeps a zero after sDi)
    return sizeof(T) * ((size_t)DB * SIL + DB + 2) > sizeof(T) * (2 * 8 * SPL + 144)
               ? sizeof(T) * ((size_t)DB * SIL + DB + 2)
               : sizeof(T) * (2 * 8 * SPL + 144);
}

__device__ __forceinline__ void dbg_mark(int* dbg, int q, int phase, int i, int j) {
    if (dbg && __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0) {
        int* p = dbg + 4 * blockIdx.x;
        __hip_atomic_store(p + 0, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p + 2, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p + 3, j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(p + 1, phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <typename T>
__device__ __forceinline__ void diag_factor_rank8(T* __restrict__ A, int64_t ld, T* __restrict__ Linv,
                                                  int* __restrict__ info, int64_t col0, unsigned char* smem_raw,
                                                  const int t, int* dbg = nullptr, long long* prof = nullptr) {
    long long pt0 = prof ? wall_clock64() : 0, pacc1 = 0, pacc2 = 0, pm = 0;
    T(*sV)[SPL] = reinterpret_cast<T(*)[SPL]>(smem_raw);
    T(*sP)[SPL] = reinterpret_cast<T(*)[SPL]>(smem_raw + sizeof(T) * 8 * SPL);
    T(*sLdW)[8][9] = reinterpret_cast<T(*)[8][9]>(smem_raw + sizeof(T) * 16 * SPL);  // per wave 0/1
    T(*sLd)[9] = sLdW[0];

    const int w = t >> 6, l = t & 63;
    const int R0 = (l & 31) * 4;
    const int cbi = 2 * w + (l >> 5);
    const int C0 = cbi * 8;

    T S[4][8];
    T Bd[4];
#pragma unroll
    for (int b = 0; b < 8; b++)
#pragma unroll
        for (int a = 0; a < 4; a++) S[a][b] = A[R0 + a + (int64_t)(C0 + b) * ld];
#pragma unroll
    for (int a = 0; a < 4; a++) Bd[a] = T(1);
    if (cbi == 0) {
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 8; b++) sV[b][R0 + a] = S[a][b];
    }
    __syncthreads();
    if (prof) pm = wall_clock64();
    const long long pload = pm;

    int fail_col = -1;
    for (int j0 = 0; j0 < DB; j0 += 8) {
        const int jn = j0 + 8;
        if (t < DB) {
            // every lane of waves 0-1 factors the pivot (identical values) in registers and
            // solves its row with it; wave 0 also leaves the factor in LDS for the pivot rows
            T(*myLd)[9] = sLdW[w];
            const int row = t;
            const bool piv = row >= j0 && row < jn;
            T x[8];
            {
                // the whole pivot block and this row's segment are read up front (one LDS
                // latency: the compiler cannot move these reads above the myLd stores), the
                // factor runs in place in registers, and the stores follow in one branch
                T Ld[8][8], ri[8], vr[8];
#pragma unroll
                for (int c = 0; c < 8; c++)
#pragma unroll
                    for (int r = c; r < 8; r++) Ld[r][c] = sV[c][j0 + r];
#pragma unroll
                for (int q = 0; q < 8; q++) vr[q] = sV[q][row];
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    T dsum = Ld[c][c];
#pragma unroll
                    for (int k = 0; k < c; k++) dsum = fma(-Ld[c][k], Ld[c][k], dsum);
                    if (!(dsum > T(0)) && fail_col < 0) fail_col = j0 + c;
                    ri[c] = rsqrt_full(dsum);
                    Ld[c][c] = dsum * ri[c];
#pragma unroll
                    for (int r = c + 1; r < 8; r++) {
                        T v = Ld[r][c];
#pragma unroll
                        for (int k = 0; k < c; k++) v = fma(-Ld[r][k], Ld[c][k], v);
                        Ld[r][c] = v * ri[c];
                    }
                }
                // one lane per wave writes (64 lanes storing one word serialise in the LDS)
                if (l == 0) {
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        myLd[c][8] = ri[c];
#pragma unroll
                        for (int r = c; r < 8; r++) myLd[r][c] = Ld[r][c];
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    T v = piv ? ((row - j0 == q) ? T(1) : T(0)) : vr[q];
#pragma unroll
                    for (int q2 = 0; q2 < q; q2++) v = fma(-x[q2], Ld[q][q2], v);
                    x[q] = v * ri[q];
                }
            }
#pragma unroll
            for (int q = 0; q < 8; q++) sP[q][row] = x[q];
        }
        __syncthreads();
        if (prof) {
            const long long tn = wall_clock64();
            pacc1 += tn - pm;
            pm = tn;
        }
        const bool pivrows = R0 >= j0 && R0 < jn;
        if (cbi == (j0 >> 3)) {
            if (pivrows) {
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    const int p = R0 + a - j0;
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const T xq = sP[q][R0 + a];
                        S[a][q] = (q <= p) ? sLd[p][q] : xq;
                        if (q == p) Bd[a] = xq;
                    }
                }
            } else {
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int q = 0; q < 8; q++) S[a][q] = sP[q][R0 + a];
            }
        }
        if (C0 >= jn && (R0 < jn || R0 + 3 >= C0)) {
            if (pivrows) {
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 8; b++) S[a][b] = T(0);
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                T u[4], v[8];
#pragma unroll
                for (int a = 0; a < 4; a++) u[a] = sP[q][R0 + a];
#pragma unroll
                for (int b = 0; b < 8; b++) v[b] = sP[q][C0 + b];
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 8; b++) S[a][b] = fma(-u[a], v[b], S[a][b]);
            }
        }
        if (jn < DB && cbi == (jn >> 3)) {
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 8; b++) sV[b][R0 + a] = S[a][b];
        }
        __syncthreads();
        if (prof) {
            const long long tn = wall_clock64();
            pacc2 += tn - pm;
            pm = tn;
        }
    }
    if (prof && t == 0) {
        prof[0] = pload - pt0;
        prof[1] = pacc1;
        prof[2] = pacc2;
    }
    if (fail_col >= 0) atomicMin(info, (int)(col0 + fail_col + 1));  // same value in every lane of waves 0-1

    T(*sI)[SIL] = reinterpret_cast<T(*)[SIL]>(smem_raw);
    T* sBd = reinterpret_cast<T*>(smem_raw + sizeof(T) * DB * SIL);
#pragma unroll
    for (int a = 0; a < 4; a++) {
#pragma unroll
        for (int b = 0; b < 8; b++) sI[R0 + a][C0 + b] = S[a][b];
        if (R0 + a >= C0 && R0 + a < C0 + 8) sBd[R0 + a] = Bd[a];
    }
    __syncthreads();
    {
        const int r = t & (DB - 1);
        for (int c = t >> 7; c < DB; c += NT / DB) {
            if (r >= c) A[r + (int64_t)c * ld] = sI[r][c];
            Linv[r + c * DB] = (r > c) ? sI[c][r] : ((r == c) ? sBd[r] : T(0));
        }
    }
}

// ------------------------------------------------------------------------------------------
// Diagonal 128x128 block, blocked: four 32-column panels, the panel's 32 x 32 diagonal block
// factored by ONE wave in registers and everything else on the MFMA units.
//
// The block lives in LDS (column-major, stride SIL): lower triangle = A becoming L; the
// strict upper triangle collects Linv^T (Linv = L^{-1}), its diagonal goes to sDi.  Per panel
// p (c0 = 32 p):
//   1  wave 0: D = L_pp L_pp^T in registers -- lane l < 32 holds row l of D, lane 32 + i row
//      i of the identity riding along (it ends as row i of L_pp^{-T}); column step c: the
//      pivot and the scaled column are broadcast by readlane (scalar operands), no barrier.
//      L_pp -> lower, Dinv_p = L_pp^{-1} -> upper (transposed) + sDi
//   2  all waves: panel rows below, L_rp = A_rp Dinv_p^T (16x16 MFMA tiles, K = 32)
//   3  all waves: trailing lower tiles A_rr' -= L_rp L_r'p^T
// then the off-diagonal 32-blocks of Linv by distance d = 1..3:
//   Linv_ij = -Dinv_i sum_{k=j}^{i-1} L_ik Linv_kj  (i = j + d; S staged in Linv_ij's slot)
// and L, Linv leave in coalesced column stores.  Replaces the rank-8 in-register image
// (diag_factor_rank8: 16 serial pivot steps of 2 barriers each, 52 us per DIAGX task).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double rl_lane(double v, int lane) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float rl_lane(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// GPRX_FACT32_PROF (a profiling build only): core-clock split of fact32's steps into the pivot
// block (readlanes, 4 x 4 factor, its inverse), the panel solve and the trailing MFMAs; each
// mark first makes the wave wait for the phase's last result (readfirstlane)
#ifdef GPRX_FACT32_PROF
#define F32_MARK(acc_, x_)                                                                           \
    do {                                                                                             \
        const int d_ = __builtin_amdgcn_readfirstlane((int)__builtin_bit_cast(unsigned long long, (double)(x_))); \
        asm volatile("" ::"s"(d_) : "memory");                                                       \
        const long long n_ = (long long)__builtin_amdgcn_s_memtime();                               \
        acc_ += n_ - f32_t;                                                                          \
        f32_t = n_;                                                                                  \
    } while (0)
#else
#define F32_MARK(acc_, x_) (void)0
#endif

// One wave factors the 32 x 32 diagonal block D at (c0, c0) of the LDS image: L_D -> lower,
// Dinv = L_D^{-1} -> upper (transposed, Dinv[j][i] at row c0 + i, column c0 + j) and sDi.
//
// (f64; f32 keeps diag_factor_rank8.)  The augmented [D; I] (64 x 32) lives in eight 16x16 MFMA accumulator tiles
// (acc[tr][tc][reg] = row 16 tr + lane % 16, column 16 tc + lane / 16 + 4 reg).  Column steps
// of 4: the 4 x 4 pivot block comes out by readlane, its factor and inverse are formed
// uniformly, the 4 panel columns -- ONE register of the tile column, lanes (row, column) --
// are solved by three shuffles and four FMAs per lane, and the trailing update is one
// v_mfma_f64_16x16x4f64 per tile straight from those panel registers (their (row, k) lane
// layout is the MFMA operand layout), with the finished columns masked to zero in the
// operand.  The identity rows (tiles 2, 3) end as L_D^{-T}.
template <typename T>
__device__ __forceinline__ void fact32(T* __restrict__ sS, T* __restrict__ sDi, int c0, int& fail,
                                       long long* fprof = nullptr) {
    constexpr int SL = SIL;
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    if constexpr (std::is_same<T, double>::value) {
        typedef Mfma<double> Tr;
        // tiles (tile row tr: 0, 1 = D, 2, 3 = identity; tile column tc) that can be nonzero:
        // (0, 1) is above the diagonal and (3, 1)'s partner (3, 0) stays zero (L^{-T} is upper)
        constexpr int TI[4][2] = {{0, -1}, {1, 2}, {3, 4}, {-1, 5}};
        d4_t acc[6];
#pragma unroll
        for (int tr = 0; tr < 4; tr++)
#pragma unroll
            for (int tc = 0; tc < 2; tc++) {
                if (TI[tr][tc] < 0) continue;
#pragma unroll
                for (int rg = 0; rg < 4; rg++) {
                    const int R = 16 * tr + lr, C = 16 * tc + Tr::orow(lk, rg);
                    double v;
                    if (tr < 2) v = (C <= R) ? sS[(c0 + R) + (c0 + C) * SL] : 0.0;
                    else v = (R - 32 == C) ? 1.0 : 0.0;
                    acc[TI[tr][tc]][rg] = v;
                }
            }
#ifdef GPRX_FACT32_PROF
        long long f32_t = (long long)__builtin_amdgcn_s_memtime(), f32_piv = 0, f32_pan = 0, f32_trl = 0;
#endif
        // Trailing MFMAs of step st: tiles (tr, tcp) for tcp = tc..1 (see f32_mfma_on).  Only the
        // one that updates the NEXT pivot tile is issued at once; the others are deferred into
        // the next step's pivot phase, one between each column of its 4 x 4 factor
        // (sched_barrier): issued back to back they held the wave's in-order issue for ~6 x 64
        // cycles in front of the pivot chain, the latency-bound critical path of the factor.
        double pa[2] = {0.0, 0.0}, pb[4] = {0.0, 0.0, 0.0, 0.0};  // the previous step's operands
#pragma unroll
        for (int st = 0; st < 8; st++) {
            const int k0 = 4 * st, tc = k0 / 16, rg = (k0 % 16) / 4, pl = k0 % 16;
            // deferred MFMA number m of step st - 1 (compile-time: the loop is unrolled)
            auto deferred = [&](int m) {
                if (st == 0) return;
                const int tcq = (4 * (st - 1)) / 16, tcn = tc;
                int cnt = 0;
#pragma unroll
                for (int tcp = tcq; tcp < 2; tcp++)
#pragma unroll
                    for (int tr = 0; tr < 4; tr++) {
                        if (TI[tr][tcp] < 0 || TI[tr][tcq] < 0) continue;
                        if (tr < 2 && tr < tcp) continue;
                        if (tr == tcn && tcp == tcn) continue;  // the critical one, already issued
                        if (cnt++ == m) acc[TI[tr][tcp]] = Tr::mma(pa[tcp], pb[tr], acc[TI[tr][tcp]]);
                    }
            };
            // the 4 x 4 pivot block (lower) of tile (tc, tc): P[i][j] at lane (pl + i) + 16 j;
            // its factor, then Q = L_P^{-1}, reduced to this lane's row qr = Q[lk][.]
            double qr[4];
            // the panel operands a[r][k0 + i] of every row, gathered to the lanes of column i: their
            // shuffles go out right after the last deferred MFMA of step st - 1 (the last write to
            // this tile column), so their LDS latency hides under the pivot chain of column 3 and the
            // 4 x 4 inverse instead of following them
            double sv[4][4];
            auto gather_panel = [&]() {
#pragma unroll
                for (int tr = 0; tr < 4; tr++) {
                    if (TI[tr][tc] < 0) continue;
#pragma unroll
                    for (int i = 0; i < 4; i++) sv[tr][i] = __shfl(acc[TI[tr][tc]][rg], lr + 16 * i, 64);
                }
            };
            {
                double Lp[4][4], rq[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    __builtin_amdgcn_sched_barrier(0);
                    deferred(i == 0 ? 0 : i + 1);
                    if (i == 0) deferred(1);
                    if (i == 3) gather_panel();
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < i; j++) {
                        double v = rl_lane(acc[TI[tc][tc]][rg], pl + i + 16 * j);
#pragma unroll
                        for (int k = 0; k < j; k++) v = fma(-Lp[i][k], Lp[j][k], v);
                        Lp[i][j] = v * rq[j];
                    }
                    double dsum = rl_lane(acc[TI[tc][tc]][rg], pl + i + 16 * i);
#pragma unroll
                    for (int k = 0; k < i; k++) dsum = fma(-Lp[i][k], Lp[i][k], dsum);
                    rq[i] = rsqrt_full(dsum);  // (a non-positive or NaN dsum gives a NaN L_ii: checked at the end)
                    Lp[i][i] = dsum * rq[i];
                }
                __builtin_amdgcn_sched_barrier(0);
                // L_P goes to the image directly (lane 0; the output stage below skips the
                // diagonal 4 x 4 blocks): the pivot rows' panel values A_P Q^T would cost
                // accuracy on ill-conditioned blocks, and a per-lane select of L_P cost ~26
                // instructions on the latency-bound pivot chain
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int j = 0; j <= i; j++) sS[(c0 + k0 + i) + (c0 + k0 + j) * SL] = Lp[i][j];
                }
                double Q[4][4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    Q[i][i] = rq[i];
#pragma unroll
                    for (int j = 0; j < i; j++) {
                        double v = 0.0;
#pragma unroll
                        for (int k = j; k < i; k++) v = fma(Lp[i][k], Q[k][j], v);
                        Q[i][j] = -v * rq[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    double v = 0.0;
#pragma unroll
                    for (int j = i; j < 4; j++) v = (lk == j) ? Q[j][i] : v;
                    qr[i] = v;
                }
            }
            F32_MARK(f32_piv, qr[0] + qr[1] + qr[2] + qr[3]);
            // panel: L[r][k0 + lk] = sum_{i <= lk} a[r][k0 + i] Q[lk][i] (D rows above k0 kept)
            double pv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int tr = 0; tr < 4; tr++) {
                if (TI[tr][tc] < 0) continue;
                const double v = acc[TI[tr][tc]][rg];
                double nv = 0.0;
#pragma unroll
                for (int i = 0; i < 4; i++) nv = fma(sv[tr][i], qr[i], nv);
                const bool keep = tr < 2 && 16 * tr + lr < k0;
                pv[tr] = keep ? v : nv;  // (pivot rows: masked out of the trailing operands)
                acc[TI[tr][tc]][rg] = pv[tr];
            }
            F32_MARK(f32_pan, pv[0] + pv[1] + pv[2] + pv[3]);
            // trailing: tile (tr, tcp) -= panel(tr) panel_D(tcp)^T over the columns > k0 + 3:
            // operands for this step's MFMAs; the next pivot tile's one now, the rest deferred
#pragma unroll
            for (int tcp = 0; tcp < 2; tcp++) pa[tcp] = (16 * tcp + lr > k0 + 3) ? -pv[tcp] : 0.0;
#pragma unroll
            for (int tr = 0; tr < 4; tr++) pb[tr] = (tr < 2 && 16 * tr + lr < k0 + 4) ? 0.0 : pv[tr];
            if (st < 7) {
                const int tcn = (k0 + 4) / 16;
                acc[TI[tcn][tcn]] = Tr::mma(pa[tcn], pb[tcn], acc[TI[tcn][tcn]]);
            } else {  // last step: everything now
#pragma unroll
                for (int tcp = tc; tcp < 2; tcp++)
#pragma unroll
                    for (int tr = 0; tr < 4; tr++) {
                        if (TI[tr][tcp] < 0 || TI[tr][tc] < 0) continue;
                        if (tr < 2 && tr < tcp) continue;
                        acc[TI[tr][tcp]] = Tr::mma(pa[tcp], pb[tr], acc[TI[tr][tcp]]);
                    }
            }
        }
#ifdef GPRX_FACT32_PROF
        F32_MARK(f32_trl, acc[0][3] + acc[2][3] + acc[5][3]);
        if (fprof) {
            fprof[0] += f32_piv;
            fprof[1] += f32_pan;
            fprof[2] += f32_trl;
        }
#endif
        // out: L_D (lower incl. diagonal); Dinv from the identity rows (X = L_D^{-T},
        // Dinv[j][i] = X[i][j]) transposed into the upper triangle, its diagonal into sDi
#pragma unroll
        for (int tr = 0; tr < 4; tr++)
#pragma unroll
            for (int tc = 0; tc < 2; tc++) {
                if (TI[tr][tc] < 0) continue;
#pragma unroll
                for (int rg = 0; rg < 4; rg++) {
                    const int R = 16 * tr + lr, C = 16 * tc + Tr::orow(lk, rg);
                    const double v = acc[TI[tr][tc]][rg];
                    if (tr < 2) {
                        if (C <= R && (R >> 2) != (C >> 2)) sS[(c0 + R) + (c0 + C) * SL] = v;  // L_P: above
                    } else {
                        const int i = R - 32;
                        if (C > i) sS[(c0 + i) + (c0 + C) * SL] = v;
                        else if (C == i) sDi[c0 + i] = v;
                    }
                }
            }
        // info: the first column whose pivot was not positive (its L_ii and every later one NaN)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const double dg = sS[(c0 + (lane & 31)) * (SL + 1)];
        const unsigned long long bad = __ballot(lane < 32 && !(dg > 0.0));
        if (bad && fail < 0) fail = c0 + (int)__builtin_ctzll(bad);
    }
}

template <typename T>
__device__ __forceinline__ void diag_factor_blocked(T* __restrict__ A, int64_t ld, T* __restrict__ Linv,
                                                    int* __restrict__ info, int64_t col0, unsigned char* smem_raw,
                                                    const int t, long long* prof = nullptr) {
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    constexpr int SL = SIL;
    T* sS = reinterpret_cast<T*>(smem_raw);
    T* sDi = sS + (size_t)DB * SL;
    const int w = t >> 6, lane = t & 63, lr = lane & 15, lk = lane >> 4;
    long long pt0 = prof ? wall_clock64() : 0, pf = 0, pm = 0, pinv = 0;
    // ---- load (column c, rows r: coalesced; all loads in flight before the LDS stores) --
    {
        const int r = t & (DB - 1), cq = t >> 7;
        T v[DB / (NT / DB)];
#pragma unroll
        for (int u = 0; u < DB / (NT / DB); u++) v[u] = A[r + (int64_t)(cq + u * (NT / DB)) * ld];
#pragma unroll
        for (int u = 0; u < DB / (NT / DB); u++) sS[r + (cq + u * (NT / DB)) * SL] = v[u];
    }
    __syncthreads();
    const long long pload = prof ? wall_clock64() : 0;
    int fail = -1;
#pragma unroll 1
    for (int p = 0; p < 4; p++) {
        const int c0 = 32 * p;
        const long long tf0 = prof ? wall_clock64() : 0;
        // ---- 1: the 32 x 32 diagonal block, wave 0 -----------------------------------------
        if (w == 0) fact32<T>(sS, sDi, c0, fail);
        __syncthreads();
        if (prof) {
            const long long tn = wall_clock64();
            pf += tn - tf0;
            pm = tn;
        }
        if (p == 3) break;
        // ---- 2: L_rp = A_rp Dinv_p^T for the rows below (output tiles 16 x 16) -------------
        const int r0 = c0 + 32, nrt = (DB - r0) / 16;
        {
            acc_t acc[2];
            int tl[2];
            int nt = 0;
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int tt = w + 8 * u;
                tl[u] = tt;
                acc[u] = acc_t{0};
                if (tt < nrt * 2) {
                    nt = u + 1;
                    const int rt = tt >> 1, ct = tt & 1;
                    const int cc = ct * 16 + lr;  // output column (Dinv row)
#pragma unroll
                    for (int kq = 0; kq < 8; kq++) {
                        const int k = kq * 4 + lk;
                        const T av = (k < cc) ? sS[(c0 + k) + (c0 + cc) * SL] : (k == cc ? sDi[c0 + cc] : T(0));
                        const T bv = sS[(r0 + rt * 16 + lr) + (c0 + k) * SL];
                        acc[u] = Tr::mma(av, bv, acc[u]);
                    }
                }
            }
            __syncthreads();  // every read of A_rp done before the panel is overwritten
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (u < nt) {
                    const int rt = tl[u] >> 1, ct = tl[u] & 1;
#pragma unroll
                    for (int reg = 0; reg < 4; reg++)
                        sS[(r0 + rt * 16 + lr) + (c0 + ct * 16 + Tr::orow(lk, reg)) * SL] = acc[u][reg];
                }
            }
        }
        __syncthreads();
        // ---- 3: trailing lower tiles A_rr' -= L_rp L_r'p^T ---------------------------------
        {
            const int ntl = nrt * (nrt + 1) / 2;
#pragma unroll 1
            for (int tt = w; tt < ntl; tt += 8) {
                int rt = 0;
                while ((rt + 1) * (rt + 2) / 2 <= tt) rt++;
                const int ct = tt - rt * (rt + 1) / 2;
                acc_t acc = acc_t{0};
#pragma unroll
                for (int kq = 0; kq < 8; kq++) {
                    const int k = kq * 4 + lk;
                    const T av = sS[(r0 + ct * 16 + lr) + (c0 + k) * SL];
                    const T bv = sS[(r0 + rt * 16 + lr) + (c0 + k) * SL];
                    acc = Tr::mma(av, bv, acc);
                }
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    T& dst = sS[(r0 + rt * 16 + lr) + (r0 + ct * 16 + Tr::orow(lk, reg)) * SL];
                    dst -= acc[reg];
                }
            }
        }
        __syncthreads();
    }
    if (prof) pinv = wall_clock64();
    if (fail >= 0) atomicMin(info, (int)(col0 + fail + 1));  // wave 0, every lane the same value
    // ---- the off-diagonal 32-blocks of Linv, by distance --------------------------------------
    // Linv_ij (i > j) is kept transposed in the upper block (j, i): element (r, c) of Linv_ij at
    // sS[(32 j + c) + (32 i + r) SL].  Dinv_j's elements: (kk > c) upper of block (j, j), sDi.
#pragma unroll 1
    for (int dd = 1; dd < 4; dd++) {
        const int nb = 4 - dd, ntt = nb * 4;  // blocks j = 0 .. nb-1, four 16x16 tiles each
        // ntt <= 12 tiles: wave w takes tile w and tile w + 8
        // S = sum_{k=j}^{i-1} L_ik Linv_kj: out[r][c], b = L_i k-block rows, a = Linv_kj cols
        acc_t acc = acc_t{0}, acc2 = acc_t{0};
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int tt = w + 8 * u;
            if (tt >= ntt) continue;
            const int j = tt >> 2, i = j + dd, rt = (tt >> 1) & 1, ct = tt & 1;
            acc_t a0 = acc_t{0};
#pragma unroll 1
            for (int kb = j; kb < i; kb++) {
#pragma unroll
                for (int kq = 0; kq < 8; kq++) {
                    const int kk = kq * 4 + lk, cc = ct * 16 + lr;
                    T av;  // Linv_{kb, j}[kk][cc]
                    if (kb == j) av = (kk > cc) ? sS[(32 * j + cc) + (32 * j + kk) * SL] : (kk == cc ? sDi[32 * j + cc] : T(0));
                    else av = sS[(32 * j + cc) + (32 * kb + kk) * SL];
                    const T bv = sS[(32 * i + rt * 16 + lr) + (32 * kb + kk) * SL];  // L_{i,kb}[r][kk]
                    a0 = Tr::mma(av, bv, a0);
                }
            }
            if (u == 0) acc = a0;
            else acc2 = a0;
        }
        __syncthreads();  // reads of the previous level's blocks done
        // stage S (transposed, like Linv) in block (j, i)'s slot
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int tt = w + 8 * u;
            if (tt >= ntt) continue;
            const int j = tt >> 2, i = j + dd, rt = (tt >> 1) & 1, ct = tt & 1;
            const acc_t& a0 = u == 0 ? acc : acc2;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int r = rt * 16 + lr, c = ct * 16 + Tr::orow(lk, reg);
                sS[(32 * j + c) + (32 * i + r) * SL] = a0[reg];
            }
        }
        __syncthreads();
        // Linv_ij = -Dinv_i S: out[r][c] = -sum_k Dinv_i[r][k] S[k][c]
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int tt = w + 8 * u;
            if (tt >= ntt) continue;
            const int j = tt >> 2, i = j + dd, rt = (tt >> 1) & 1, ct = tt & 1;
            acc_t a0 = acc_t{0};
#pragma unroll
            for (int kq = 0; kq < 8; kq++) {
                const int kk = kq * 4 + lk, rr = rt * 16 + lr, cc = ct * 16 + lr;
                const T av = sS[(32 * j + cc) + (32 * i + kk) * SL];  // S[kk][cc]
                const T bv = (kk < rr) ? sS[(32 * i + kk) + (32 * i + rr) * SL]
                                       : (kk == rr ? sDi[32 * i + rr] : T(0));  // Dinv_i[rr][kk]
                a0 = Tr::mma(av, bv, a0);
            }
            if (u == 0) acc = a0;
            else acc2 = a0;
        }
        __syncthreads();  // S read before it is overwritten by Linv_ij
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int tt = w + 8 * u;
            if (tt >= ntt) continue;
            const int j = tt >> 2, i = j + dd, rt = (tt >> 1) & 1, ct = tt & 1;
            const acc_t& a0 = u == 0 ? acc : acc2;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int r = rt * 16 + lr, c = ct * 16 + Tr::orow(lk, reg);
                sS[(32 * j + c) + (32 * i + r) * SL] = -a0[reg];
            }
        }
        __syncthreads();
    }
    if (prof && t == 0) {
        const long long te = wall_clock64();
        prof[0] = pload - pt0;
        prof[1] = pf;
        prof[2] = pinv - pload - pf;
        prof[3] = te - pinv;
        (void)pm;
    }
    // ---- L and Linv out: coalesced columns ------------------------------------------------
    {
        const int r = t & (DB - 1);
        for (int c = t >> 7; c < DB; c += NT / DB) {
            if (r >= c) A[r + (int64_t)c * ld] = sS[r + c * SL];
            Linv[r + c * DB] = (r > c) ? sS[c + r * SL] : ((r == c) ? sDi[r] : T(0));
        }
    }
}

// ------------------------------------------------------------------------------------------
// Diagonal 128x128 block, blocked with LOOK-AHEAD (f64): the same LDS image and 32-column
// panels as diag_factor_blocked, but only the critical chain stays serial.  Per panel p
// (c0 = 32 p), 16 x 16 tile indices R, C = 0..7:
//   F(p)   wave 0: fact32 (the 32 x 32 diagonal block: L_pp, Dinv_p)
//          waves 1-7 meanwhile: the far trailing tiles of panel p-1 (C >= 2p + 2) and Linv's
//          row block p-1 (Linv_{p-1,j} = -Dinv_{p-1} sum_{k=j}^{p-2} L_{p-1,k} Linv_kj, one wave
//          per (j, 16-column) unit: S staged in the unit's own slot, wave-private, no barrier)
//   P(p)   all waves: L_rp = A_rp Dinv_p^T for the rows below
//   Ua(p)  all waves: the trailing tiles of the NEXT panel's columns only (C = 2p+2, 2p+3)
// so F(p+1) starts after a panel solve and a 32-column update instead of the whole trailing
// update and the Linv assembly.  Linv's last row block follows F(3).  Every region a phase
// writes is disjoint from what the concurrent waves read or write (see the phase comments).
// ------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T linv_at(const T* __restrict__ sS, const T* __restrict__ sDi, int R, int C) {
    // Linv[R][C] of the LDS image: strict lower part kept transposed in the upper triangle, the
    // diagonal in sDi (= sS + DB SIL), a zero in sDi[DB].  One unconditional load from a selected
    // address: a conditional load compiles to an exec-masked branch per element.
    (void)sDi;
    const int idx = (R > C) ? C + R * SIL : DB * SIL + (R == C ? R : DB);
    return sS[idx];
}

// one 16 x 16 lower tile (R, C) of the trailing matrix: A_RC -= L_{R,panel} L_{C,panel}^T (K = 32)
template <typename T>
__device__ __forceinline__ void la_trail_tile(T* __restrict__ sS, int c0, int R, int C, int lr, int lk) {
    typedef Mfma<T> Tr;
    typename Tr::acc_t acc = typename Tr::acc_t{0};
#pragma unroll
    for (int kq = 0; kq < 8; kq++) {
        const int k = c0 + kq * 4 + lk;
        acc = Tr::mma(sS[(16 * C + lr) + k * SIL], sS[(16 * R + lr) + k * SIL], acc);
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++) sS[(16 * R + lr) + (16 * C + Tr::orow(lk, reg)) * SIL] -= acc[reg];
}

// Linv row block p, column block j, 16-column half ct (rows 32 p .. 32 p + 31): one wave.
// S = sum_{kb_lo <= kb < kb_hi} L_{p,kb} Linv_{kb,j} (LA_LOAD: plus the partial S staged by an
// earlier call), staged transposed in the unit's own Linv slot; LA_FINISH: Linv_pj = -Dinv_p S.
enum { LA_LOAD = 1, LA_FINISH = 2 };
// gout (LA_FINISH): the finished Linv_pj half also goes straight to global memory (Linv,
// column-major, ld DB; write-through) from the registers
template <typename T>
__device__ __forceinline__ void la_linv_unit(T* __restrict__ sS, const T* __restrict__ sDi, int p, int j, int ct,
                                             int kb_lo, int kb_hi, int mode, int lr, int lk, T* gout = nullptr) {
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    acc_t s0 = acc_t{0}, s1 = acc_t{0};
    const int cc = 32 * j + 16 * ct + lr;  // Linv column this lane feeds
    if (mode & LA_LOAD) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int c = 32 * j + 16 * ct + Tr::orow(lk, reg);
            s0[reg] = sS[c + (32 * p + lr) * SIL];
            s1[reg] = sS[c + (32 * p + 16 + lr) * SIL];
        }
    }
#pragma unroll 1
    for (int kb = kb_lo; kb < kb_hi; kb++) {
#pragma unroll
        for (int kq = 0; kq < 8; kq++) {
            const int kk = 32 * kb + kq * 4 + lk;
            const T av = linv_at(sS, sDi, kk, cc);  // Linv[kk][cc]
            s0 = Tr::mma(av, sS[(32 * p + lr) + kk * SIL], s0);
            s1 = Tr::mma(av, sS[(32 * p + 16 + lr) + kk * SIL], s1);
        }
    }
    // stage S (rows 32p + r, columns 32j + 16ct + c) transposed in the unit's own Linv slot
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int c = 32 * j + 16 * ct + Tr::orow(lk, reg);
        sS[c + (32 * p + lr) * SIL] = s0[reg];
        sS[c + (32 * p + 16 + lr) * SIL] = s1[reg];
    }
    if (!(mode & LA_FINISH)) return;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // Linv_pj = -Dinv_p S
    acc_t o0 = acc_t{0}, o1 = acc_t{0};
#pragma unroll
    for (int kq = 0; kq < 8; kq++) {
        const int kk = kq * 4 + lk;
        const T av = sS[cc + (32 * p + kk) * SIL];  // S[kk][cc]
        o0 = Tr::mma(av, linv_at(sS, sDi, 32 * p + lr, 32 * p + kk), o0);
        o1 = Tr::mma(av, linv_at(sS, sDi, 32 * p + 16 + lr, 32 * p + kk), o1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int c = 32 * j + 16 * ct + Tr::orow(lk, reg);
        sS[c + (32 * p + lr) * SIL] = -o0[reg];
        sS[c + (32 * p + 16 + lr) * SIL] = -o1[reg];
        if (gout) {
            st_sc1(gout + (32 * p + lr) + (int64_t)c * DB, -o0[reg]);
            st_sc1(gout + (32 * p + 16 + lr) + (int64_t)c * DB, -o1[reg]);
        }
    }
}

// global stores of finished pieces, spread over the threads tid0 .. tid0 + nth - 1:
// L's panel q (rows 32 q .. 127, columns 32 q .. 32 q + 31)
template <typename T>
__device__ __forceinline__ void la_store_lpanel(T* __restrict__ A, int64_t ld, const T* __restrict__ sS, int q, int tid,
                                                int nth) {
    const int nr = DB - 32 * q;
    for (int e = tid; e < 32 * nr; e += nth) {
        const int c = 32 * q + e / nr, r = 32 * q + e % nr;
        st_sc1(A + r + (int64_t)c * ld, sS[r + c * SIL]);  // write-through: no release fence needed
    }
}

// row block q of Linv, columns 32 q .. 127 (Dinv_q and the zeros right of it); its columns < 32 q
// go out from the registers of the units that finish them (la_linv_unit gout), so the whole
// row block is stored during the next F phase, not in the factor's tail
template <typename T>
__device__ __forceinline__ void la_store_linv_diag(T* __restrict__ Linv, const T* __restrict__ sS,
                                                   const T* __restrict__ sDi, int q, int tid, int nth) {
    const int nc = DB - 32 * q;
    for (int e = tid; e < 32 * nc; e += nth) {
        const int r = 32 * q + (e & 31), c = 32 * q + (e >> 5);
        st_sc1(Linv + r + c * DB, linv_at(sS, sDi, r, c));
    }
}

// F(p)'s side phase, waves wlo..7: the stores of what panel p-1 finished (L panel p-1; Linv row
// block p-1 right of column 32 (p-1), Dinv_{p-1} included), then the jobs -- Linv row block p-1
// (2 (p-1) units, each storing its finished half from its registers), at p = 3 also the partial
// sums of Linv row block 3 over kb < 2 (4 units), then the far trailing tiles of panel p-1
// (C >= 2p + 2, R >= C).  (Row block p-2 was stored here whole, and row block 2 in the factor's
// tail: 4096 of the tail's 6144 stores; chain step 53.0 -> 51.6 us, C2 523 -> 529 fits/s,
// profiles/r05r.  Also moving row block 3's kb = 2 term into F(3)'s side phase, by the waves
// that finish Linv_{2,j}, lengthened the F and P phases: 53.1 us.)
template <typename T>
__device__ __forceinline__ void la_side(T* __restrict__ A, int64_t ld, T* __restrict__ Linv, T* __restrict__ sS,
                                        const T* __restrict__ sDi, int p, int t, int w, int wlo, int lr, int lk) {
    const int nth = NT - 64 * wlo, tid = t - 64 * wlo;
    la_store_lpanel<T>(A, ld, sS, p - 1, tid, nth);
    la_store_linv_diag<T>(Linv, sS, sDi, p - 1, tid, nth);
    const int pl = p - 1, nl = 2 * pl, np3 = (p == 3) ? 4 : 0;
    const int cmin = 2 * p + 2, nc = 8 - cmin, nt = nc > 0 ? nc * (nc + 1) / 2 : 0;
    const int nw = 8 - wlo;
#pragma unroll 1
    for (int job = w - wlo; job < nl + np3 + nt; job += nw) {
        if (job < nl) {
            la_linv_unit<T>(sS, sDi, pl, job >> 1, job & 1, job >> 1, pl, LA_FINISH, lr, lk, Linv);
        } else if (job < nl + np3) {
            const int u = job - nl;
            la_linv_unit<T>(sS, sDi, 3, u >> 1, u & 1, u >> 1, 2, 0, lr, lk);
        } else {
            const int tt = job - nl - np3;  // lower tiles of the C >= cmin square, row-major
            int rr = 0;
            while ((rr + 1) * (rr + 2) / 2 <= tt) rr++;
            const int cc = tt - rr * (rr + 1) / 2;
            la_trail_tile<T>(sS, 32 * pl, cmin + rr, cmin + cc, lr, lk);
        }
    }
}

// from_lds: the block is already in the LDS image (diagx_ts left the syrk result there)
template <typename T>
__device__ __forceinline__ void diag_factor_la(T* __restrict__ A, int64_t ld, T* __restrict__ Linv,
                                               int* __restrict__ info, int64_t col0, unsigned char* smem_raw,
                                               const int t, long long* prof = nullptr, bool from_lds = false) {
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    constexpr int SL = SIL;
    T* sS = reinterpret_cast<T*>(smem_raw);
    T* sDi = sS + (size_t)DB * SL;
    const int w = t >> 6, lane = t & 63, lr = lane & 15, lk = lane >> 4;
    long long pt0 = prof ? wall_clock64() : 0, pf = 0, pside = 0, pfw = 0;
    if (!from_lds) {
        const int r = t & (DB - 1), cq = t >> 7;
        T v[DB / (NT / DB)];
#pragma unroll
        for (int u = 0; u < DB / (NT / DB); u++) v[u] = A[r + (int64_t)(cq + u * (NT / DB)) * ld];
#pragma unroll
        for (int u = 0; u < DB / (NT / DB); u++) sS[r + (cq + u * (NT / DB)) * SL] = v[u];
    }
    if (t == 0) sDi[DB] = T(0);  // linv_at's zero
    __syncthreads();
    const long long pload = prof ? wall_clock64() : 0;
    int fail = -1;
#pragma unroll 1
    for (int p = 0; p < 4; p++) {
        const int c0 = 32 * p;
        const long long tf0 = prof ? wall_clock64() : 0;
        // ---- F(p): wave 0 factors the diagonal block; the others finish panel p-1's side work
        // (fact32 touches block (p, p) only; the far trailing tiles have C >= 2p + 2; the Linv
        // units write rows 32 (p - 1) .. 32 p - 1 (p = 3: also 96 .. 127) of columns < 32 (p - 1),
        // transposed: LDS columns >= 32 (p - 1), rows < 32 (p - 1); the stores only read)
        if (w == 0) {
            fact32<T>(sS, sDi, c0, fail, prof ? prof + 4 : nullptr);
            if (prof) pfw += wall_clock64() - tf0;
        } else if (p > 0) {
            la_side<T>(A, ld, Linv, sS, sDi, p, t, w, 1, lr, lk);
        }
        __syncthreads();
        if (prof) {
            const long long tn = wall_clock64();
            pf += tn - tf0;
        }
        if (p == 3) break;
        const long long ts0 = prof ? wall_clock64() : 0;
        // ---- P(p): L_rp = A_rp Dinv_p^T for the rows below; one 16-row tile per wave (both of
        // its 16-column halves), so a wave overwrites only what it read: no barrier inside.
        // The explicit inverse alone is not backward stable when L_pp is ill-conditioned (a
        // sparse-GP normal matrix with cond 1.5e13 lost positive definiteness at pivot 35):
        // one step of refinement, X += (A - X L_pp^T) Dinv_p^T, restores the substitution's
        // accuracy (numpy emulation: residual 5.8e-10 against 4.7e-10 for dtrsm).
        const int r0 = c0 + 32, nrt = (DB - r0) / 16;
        if (w < nrt) {
            acc_t a0 = acc_t{0}, a1 = acc_t{0};
            const int rr = r0 + w * 16 + lr;
            T av0[4], av1[4];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {  // A_rp in the accumulator layout (for the residual)
                av0[reg] = sS[rr + (c0 + Tr::orow(lk, reg)) * SL];
                av1[reg] = sS[rr + (c0 + 16 + Tr::orow(lk, reg)) * SL];
            }
            T dmax = T(0);  // max |Dinv_p| over the entries this lane feeds
#pragma unroll
            for (int kq = 0; kq < 8; kq++) {
                const int k = kq * 4 + lk;
                const T bv = sS[rr + (c0 + k) * SL];
                const T d0 = linv_at(sS, sDi, c0 + lr, c0 + k), d1 = linv_at(sS, sDi, c0 + 16 + lr, c0 + k);
                dmax = fmax(dmax, fmax(fabs(d0), fabs(d1)));
                a0 = Tr::mma(d0, bv, a0);
                a1 = Tr::mma(d1, bv, a1);
            }
            // est = max|Dinv_p| max_i L_ii (<= cond_2(L_pp), within a factor 32^2 of it): a
            // well-conditioned block skips the refinement -- its explicit-inverse error is then
            // no larger than that of the 128-block TRSM tasks (which also use explicit inverses)
            // (min of the 32 diagonal words by broadcast LDS reads, the max test by one ballot:
            // two 6-step shuffle reductions cost ~0.45 us per panel on the chain)
            T dimin = sDi[c0];  // 1 / L_ii
#pragma unroll
            for (int i = 1; i < 32; i++) dimin = fmin(dimin, sDi[c0 + i]);
            const bool refine = __ballot(dmax > T(32) * dimin) != 0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {  // X0 (kept in a0, a1) through LDS to the operand layout
                sS[rr + (c0 + Tr::orow(lk, reg)) * SL] = a0[reg];
                sS[rr + (c0 + 16 + Tr::orow(lk, reg)) * SL] = a1[reg];
            }
            if (refine) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            acc_t q0 = acc_t{0}, q1 = acc_t{0};  // X0 L_pp^T
#pragma unroll
            for (int kq = 0; kq < 8; kq++) {
                const int k = kq * 4 + lk;
                const T xv = sS[rr + (c0 + k) * SL];
                const T l0v = sS[(c0 + lr) + (c0 + k) * SL], l1v = sS[(c0 + 16 + lr) + (c0 + k) * SL];
                const T l0 = (lr >= k) ? l0v : T(0), l1 = (16 + lr >= k) ? l1v : T(0);  // above: Dinv
                q0 = Tr::mma(l0, xv, q0);
                q1 = Tr::mma(l1, xv, q1);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {  // R = A - X0 L^T, to the operand layout
                sS[rr + (c0 + Tr::orow(lk, reg)) * SL] = av0[reg] - q0[reg];
                sS[rr + (c0 + 16 + Tr::orow(lk, reg)) * SL] = av1[reg] - q1[reg];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int kq = 0; kq < 8; kq++) {
                const int k = kq * 4 + lk;
                const T rv = sS[rr + (c0 + k) * SL];
                a0 = Tr::mma(linv_at(sS, sDi, c0 + lr, c0 + k), rv, a0);
                a1 = Tr::mma(linv_at(sS, sDi, c0 + 16 + lr, c0 + k), rv, a1);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                sS[rr + (c0 + Tr::orow(lk, reg)) * SL] = a0[reg];
                sS[rr + (c0 + 16 + Tr::orow(lk, reg)) * SL] = a1[reg];
            }
            }  // refine
        }
        __syncthreads();
        // ---- Ua(p): the next panel's columns (C = 2p+2, 2p+3; R >= C), all waves -------------
        {
            const int Cn = 2 * p + 2, n0 = 8 - Cn, ntl = n0 + (n0 - 1);
#pragma unroll 1
            for (int tt = w; tt < ntl; tt += 8) {
                const int C = tt < n0 ? Cn : Cn + 1;
                const int R = tt < n0 ? Cn + tt : Cn + 1 + (tt - n0);
                la_trail_tile<T>(sS, c0, R, C, lr, lk);
            }
        }
        __syncthreads();
        if (prof) pside += wall_clock64() - ts0;
    }
    if (fail >= 0) atomicMin(info, (int)(col0 + fail + 1));  // wave 0, every lane the same value
    // Linv's last row block: the kb = 2 term and -Dinv_3 S (6 units, waves 0-5), each storing its
    // half block to global memory from its registers; the stores of L panel 3 and the rest of row
    // block 3 (its diagonal block Dinv_3 and the zeros right of it) by waves 6-7 meanwhile
    if (w < 6) {
        const int j = w >> 1;
        la_linv_unit<T>(sS, sDi, 3, j, w & 1, 2, 3, (j < 2 ? LA_LOAD : 0) | LA_FINISH, lr, lk, Linv);
    } else {
        la_store_lpanel<T>(A, ld, sS, 3, t - 384, 128);
        // row block 3, columns 96..127 (Dinv_3, zeros above its diagonal)
        for (int e = t - 384; e < 32 * 32; e += 128) {
            const int r = 96 + (e & 31), c = 96 + (e >> 5);
            st_sc1(Linv + r + c * DB, linv_at(sS, sDi, r, c));
        }
    }
    __syncthreads();
    if (prof && t == 0) {  // load, F phases (barrier to barrier), P + Ua phases, fact32 alone
        prof[0] = pload - pt0;
        prof[1] = pf;
        prof[2] = pside;
        prof[3] = pfw;
    }
}

// from_lds (f64 look-ahead form only): the block is in the LDS image already (diagx_ts)
// (out of line: its registers (fact32's accumulators, the pivot block) no longer count against
// the task loop, which sits at 256 VGPRs -- inlined, any growth of the loop spilled, and a
// spill reload inside the update mainloop broke its counted vmcnt pipelining)
// pub (optional): publish *pub = pub_v when the block is stored, inside the call -- the
// callee-saved registers are restored after it (scratch loads), not before the chain goes on
template <typename T>
__device__ __noinline__ void diag_factor(T* __restrict__ A, int64_t ld, T* __restrict__ Linv, int* __restrict__ info,
                                         int64_t col0, unsigned char* smem_raw, const int t, int* dbg = nullptr,
                                         long long* prof = nullptr, bool from_lds = false, int* pub = nullptr,
                                         int pub_v = 0) {
    // f64: the blocked factor with look-ahead (diag_factor_la: 43 us per block in isolation
    // against 50.6 for the rank-8 image, scripts/diag_bench.py); its stores are write-through
    // (sc1), so the publication needs no release fence.  f32: the
    // rank-8 register image, plain stores and the release fence.
    if constexpr (diag_la<T>) diag_factor_la<T>(A, ld, Linv, info, col0, smem_raw, t, prof, from_lds);
    else diag_factor_rank8<T>(A, ld, Linv, info, col0, smem_raw, t, dbg, prof);
    if (pub) publish(pub, pub_v, !diag_la<T>);
}

}  // namespace pt
}  // namespace gprx
