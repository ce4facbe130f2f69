// k_remove.hip — rank-r UPDATE of a Cholesky factor by Givens rotations in ONE launch (gfx950).
//
// Removing rows [f, f + r) of a fitted model (gprx_model_remove, gprx_fit.cpp) leaves the
// factor [L11 0; L31 L33'] with L33' L33'^T = L33 L33^T + L32 L32^T: in the new coordinates
// L' L'^T = L L^T + X X^T with X = [0; L32] (n' x r), an addition, never a downdate.  X is
// eliminated column by column; for column j and vector v, in this order (j outer, v inner):
//     rho = sqrt(L_jj^2 + x_jv^2),  c = L_jj / rho,  s = x_jv / rho,  L_jj <- rho
// (computed with one reciprocal square root q = (L_jj^2 + x_jv^2)^(-1/2): c = L_jj q, s = x_jv q,
// rho = (L_jj^2 + x_jv^2) q)
//     every row i > j:  t = c L_ij + s x_iv;  x_iv <- c x_iv - s L_ij;  L_ij <- t
// Rows are independent of each other and carry their x_i along the columns; the (c, s) pairs of
// a 128-column block come from its diagonal block alone, once that block's rows have passed
// through every earlier column block.
//
// One workgroup per 128-row block i >= b0 = f / 128 of the NEW factor, one thread per row (two
// waves), claimed top block first and chained by the hand-off protocol of k_handoff.h (tickets,
// sc1 stores and loads of the (c, s) pairs, one flag per block, bounded waits).  Workgroup i
// applies block b's rotations to its tile (i, b) for b = b0 .. i - 1 with x_i in registers, then
// sweeps its own diagonal block (the serial part: 128 r rotations; wave 0 sweeps columns 0..63
// with lane broadcasts, wave 1 applies them and sweeps 64..127), publishes its 128 x r pairs
// and, off the chain, forms the diagonal block's inverse for Linv by substitution on the
// identity, one column per thread, in LDS.
//
// The source is read at the shifted position (new row / column g >= f is old g + shift) and the
// result is written tile-aligned into a SECOND buffer, with the identity padding beyond nlive
// written explicitly and zeros above the diagonal of the diagonal tiles: the fitted model stays
// intact until the status words are back, at the price of a second factor buffer.  Tiles are
// column-major, so a wave reads and writes 64 consecutive rows of a column; the next columns'
// loads are in flight while the current ones rotate.  RV vectors are carried per pass (x_i is RV
// registers per row); a wider update runs further passes in place on the new buffer, which is
// safe because a thread reads and writes only its own row.
#include "gprx_internal.h"
#include "k_handoff.h"

#include <algorithm>
#include <cstring>

namespace gprx {

namespace rm {

using namespace ho;

constexpr int NT = DB;  // one thread per row of a block
constexpr int HW = 64;  // rows (and diagonal-block columns) per wave
constexpr int PF = 8;   // columns per load group
// load groups in flight per thread, ahead of the rotations (also across tiles): 4, or 2 where x_i
// and the kept pairs already take 96 registers (f64, 16 vectors: 4 spilled)
template <typename T, int RV>
constexpr int ring_groups() { return sizeof(T) * RV >= 128 ? 2 : 4; }

template <typename T>
struct Args {
    const T* src;     // old factor, column-major
    int64_t lds;
    T* dst;           // new factor, column-major: lower tiles of blocks >= b0 written whole
    int64_t ldd;
    T* linv;          // 128 x 128 inverse of each new diagonal block (nullptr: not this pass)
    const T* X;       // x_iv at X[i + v ldx] for new rows f <= i < nlive; zero for the others
    int64_t ldx;
    int nv;           // vectors of this pass (<= RV)
    int64_t f;        // new rows and columns >= f are read at old index + shift
    int64_t shift;
    int64_t nlive;    // new rows >= nlive are identity padding
    int b0, nb;       // first block of the update, blocks of the new factor
    T* cs;            // (nb - b0) blocks of 128 x RV (c, s) pairs
    int* ctl;         // [C_NCTL] then one flag per block >= b0
    int* info;        // set to -1 (atomicMin) when a wait timed out
    long long tlimit; // wall-clock ticks (100 MHz) per wait
};

__device__ __forceinline__ float bcast(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float rsq(float v) { return rsqrtf(v); }
// f64: v_rsq_f64 and two Newton steps, y <- y + (y / 2)(1 - v y^2): about ten dependent
// instructions where the library's correctly scaled sqrt and divide are several times that, and
// the sweep of a diagonal block is one dependent chain of 128 r of these.  v = L_jj^2 + x^2 of a
// factor's entries: far from the denormals the library guards.
__device__ __forceinline__ double rsq(double v) {
    double y = __builtin_amdgcn_rsq(v);
    y = fma(0.5 * y, fma(-v * y, y, 1.0), y);
    y = fma(0.5 * y, fma(-v * y, y, 1.0), y);
    return y;
}
__device__ __forceinline__ double bcast(double v, int l) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// (every wave polls on its own; the workgroup agrees through LDS at its next barrier)
__device__ __forceinline__ bool wait_flag(const int* f, int* ctl, long long t0, long long tlimit) {
    return wait_until<1, 16>([=] { return ld_uni(f) != 0; }, ctl + C_ERR, t0, tlimit);
}

template <typename T, int RV>
__global__ __launch_bounds__(NT) void factor_update_kernel(Args<T> a) {
    constexpr int NG = ring_groups<T, RV>();
    constexpr int CSB = DB * RV * 2;  // one block's pairs: (c, s) of (column j, vector v) at (j RV + v) 2
    __shared__ int s_int[3];          // ticket, fail word of even / odd column blocks
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* s_cs = reinterpret_cast<T*>(smem_raw);  // two stage buffers of CSB; later the inverse (DB x DB)
    const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    int* flags = a.ctl + C_NCTL;
    if (w == 0) {
        s_int[1] = 0;
        s_int[2] = 0;
    }
    const int k = claim_ticket(a.ctl, &s_int[0]);
    const int i = a.b0 + k;
    if (i >= a.nb) return;
    const long long t0 = wall_clock64();
    const int64_t row = (int64_t)i * DB + t;
    const bool live = row < a.nlive;
    T* drow = a.dst + row;

    T x[RV];
#pragma unroll
    for (int v = 0; v < RV; v++) x[v] = (v < a.nv && live && row >= a.f) ? a.X[row + (int64_t)v * a.ldx] : T(0);

    // new (row, col) of the source: identity beyond nlive, zero above the diagonal
    // (branch-free: every lane loads a valid element -- its own diagonal entry for a column above
    // the diagonal, the last live row's for a padding row -- and drops what it does not need.
    // With the load inside a per-lane branch every load was waited for where the branches join)
    const int64_t lrow = live ? row : a.nlive - 1;  // (nlive >= 1)
    const int64_t lsrow = lrow < a.f ? lrow : lrow + a.shift;
    auto ldv = [&](int64_t col) -> T {
        const int64_t cc = col < lrow ? col : lrow;
        const T v = a.src[lsrow + (cc < a.f ? cc : cc + a.shift) * a.lds];
        // (v is a finite entry of the factor, so v * 0 + pad is pad; a select here is turned back
        // into a branch around the load)
        const T m = ((col <= row) & live) ? T(1) : T(0), pad = ((col == row) & !live) ? T(1) : T(0);
        return v * m + pad;
    };
    auto load_group = [&](T (&g)[PF], int64_t col0) {
#pragma unroll
        for (int q = 0; q < PF; q++) g[q] = ldv(col0 + q);
    };
    // PF columns from col0 on, rotated by the pairs at p (LDS), stored
    auto apply_group = [&](T (&g)[PF], int64_t col0, const T* p) {
#pragma unroll
        for (int q = 0; q < PF; q++) {
            T L = g[q];
#pragma unroll
            for (int v = 0; v < RV; v++)
                if (v < a.nv) {
                    const T c = p[(q * RV + v) * 2], s = p[(q * RV + v) * 2 + 1];
                    const T tt = c * L + s * x[v];
                    x[v] = c * x[v] - s * L;
                    L = tt;
                }
            drow[(col0 + q) * a.ldd] = L;
        }
    };
    // The row's columns as ONE stream from block b0's first column to the row's last: NG groups
    // are in flight, whatever tile they belong to.  The ring's slots are taken in turn with compile-time
    // indices (every section below takes a multiple of NG groups, so each starts at slot 0):
    // moving the groups along instead would wait for every load in flight.  Columns beyond the
    // row load nothing (ldv).
    T ring[NG][PF];
    int64_t colnext = (int64_t)a.b0 * DB;  // the first column not yet asked for
#pragma unroll
    for (int g = 0; g < NG; g++) {
        load_group(ring[g], colnext);
        colnext += PF;
    }
    auto refill = [&](T (&g)[PF]) {
        load_group(g, colnext);
        colnext += PF;
    };
    // the stream's next ncols columns (from col0 on; a multiple of NG PF), pairs at p
    auto apply_cols = [&](int64_t col0, int ncols, const T* p) {
#pragma nounroll
        for (int j0 = 0; j0 < ncols; j0 += NG * PF) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                apply_group(ring[g], col0 + j0 + g * PF, p + (j0 + g * PF) * RV * 2);
                refill(ring[g]);
            }
        }
    };

    // ---- column blocks b0 .. i - 1: the published rotations applied to tile (i, b) ----
    bool ok = true;
    for (int b = a.b0; b < i; b++) {
        T* sc = s_cs + (b & 1) * CSB;
        ok = wait_flag(flags + (b - a.b0), a.ctl, t0, a.tlimit);
        if (!ok) s_int[1 + (b & 1)] = 1;
        if (ok) {
            const T* g = a.cs + (int64_t)(b - a.b0) * CSB;
#pragma unroll
            for (int e = 0; e < CSB / NT; e++) sc[t + NT * e] = ld_sc1(g + t + NT * e);
        }
        __syncthreads();
        if (s_int[1 + (b & 1)]) {
            ok = false;
            break;
        }
        apply_cols((int64_t)b * DB, DB, sc);
    }

    if (ok) {
        // ---- the diagonal block: wave w sweeps its columns [64 w, 64 w + 64) ----
        const int64_t c0 = (int64_t)i * DB;
        T* sc = s_cs + (i & 1) * CSB;
        T* gcs = a.cs + (int64_t)k * CSB;
        T myc[RV], mys[RV];  // lane l keeps the pairs of column 64 w + l
#pragma unroll
        for (int v = 0; v < RV; v++) {
            myc[v] = T(1);
            mys[v] = T(0);
        }
        auto sweep_group = [&](T (&g)[PF], int64_t col0, int jj0) {
#pragma unroll
            for (int q = 0; q < PF; q++) {
                const int pl = jj0 + q;  // the pivot's lane
                T L = g[q];
#pragma unroll
                for (int v = 0; v < RV; v++)
                    if (v < a.nv) {
                        const T Lp = bcast(L, pl), xp = bcast(x[v], pl);
                        const T ss = Lp * Lp + xp * xp, ri = rsq(ss), rho = ss * ri;  // (one reciprocal square root)
                        const T c = Lp * ri, s = xp * ri;
                        const T tt = c * L + s * x[v], xn = c * x[v] - s * L;
                        x[v] = lane > pl ? xn : x[v];
                        L = lane > pl ? tt : (lane == pl ? rho : L);
                        myc[v] = lane == pl ? c : myc[v];
                        mys[v] = lane == pl ? s : mys[v];
                    }
                drow[(col0 + q) * a.ldd] = L;
            }
        };
        auto sweep_cols = [&](int64_t col0) {
#pragma nounroll
            for (int j0 = 0; j0 < HW; j0 += NG * PF) {
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    sweep_group(ring[g], col0 + j0 + g * PF, j0 + g * PF);
                    refill(ring[g]);
                }
            }
        };
        auto put_pairs = [&]() {  // this wave's 64 columns: into LDS (wave 1 reads wave 0's) and written through
#pragma unroll
            for (int v = 0; v < RV; v++) {
                const int e = ((HW * w + lane) * RV + v) * 2;
                sc[e] = myc[v];
                sc[e + 1] = mys[v];
                st_sc1(gcs + e, myc[v]);
                st_sc1(gcs + e + 1, mys[v]);
            }
        };
        // wave 0 sweeps, barrier, wave 1 applies wave 0's pairs and sweeps (one call site of the sweep)
#pragma nounroll
        for (int ph = 0; ph < 2; ph++) {
            if (w == ph) {
                if (ph == 1) apply_cols(c0, HW, sc);
                sweep_cols(c0 + HW * ph);
                put_pairs();
            }
            if (ph == 0) __syncthreads();
        }
        if (w == 0)
            for (int j = HW; j < DB; j++) drow[(c0 + j) * a.ldd] = T(0);  // above the diagonal
        publish_flag(flags + k, 1);  // (its drain and barrier: the block's stores are done, the pairs' LDS reads too)

        // ---- off the chain: the block's inverse, L x = e_c by substitution, column c = t ----
        if (a.linv) {
            T* sx = s_cs;  // x_r at sx[r DB + t]
            const T* D = a.dst + c0 + c0 * a.ldd;
            T* out = a.linv + (int64_t)i * DB * DB + (int64_t)t * DB;
            const int q0 = HW * w;  // (x_q = 0 for q < c)
            for (int r = 0; r < DB; r++) sx[r * DB + t] = (r == t) ? T(1) : T(0);
            for (int q = 0; q < q0; q++) out[q] = T(0);
            for (int q = q0; q < DB; q++) {
                const T xq = sx[q * DB + t] / ld_sc1(D + q + (int64_t)q * a.ldd);
                out[q] = xq;
                const T* col = D + (int64_t)q * a.ldd;
                // (eight loads out before the first is used: one by one, each was a round trip)
                for (int r0 = q + 1; r0 < DB; r0 += 8) {
                    T l[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) l[u] = ld_sc1(col + (r0 + u < DB ? r0 + u : DB - 1));
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (r0 + u < DB) sx[(r0 + u) * DB + t] -= l[u] * xq;
                }
            }
        }
    }
    if (t == 0 && ld_uni(a.ctl + C_ERR)) atomicMin(a.info, -1);
}

// vectors carried per pass: x_i is RV registers per row (twice that in f64) beside the 2 PF
// columns in flight
constexpr int RV_MAX = 16;
inline int width_for(int nv) { return nv <= 1 ? 1 : (nv <= 4 ? 4 : RV_MAX); }

template <typename T>
constexpr size_t lds_bytes() {
    return sizeof(T) * DB * DB;  // the inverse's columns; two stage buffers of RV_MAX fit in half of it
}

template <typename T, int RV>
static void launch_rv(const Args<T>& a, hipStream_t s) {
    static_assert(2 * DB * RV * 2 <= DB * DB, "stage buffers within the inverse's LDS");
    static bool attr = false;
    if (!attr) {
        const void* fn = (const void*)factor_update_kernel<T, RV>;
        GPRX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes<T>()));
        attr = true;
    }
    hipLaunchKernelGGL((factor_update_kernel<T, RV>), dim3((unsigned)(a.nb - a.b0)), dim3(NT), lds_bytes<T>(), s, a);
    GPRX_HIP(hipGetLastError());
}

}  // namespace rm

int factor_update_width() { return rm::RV_MAX; }

int64_t factor_update_ws_elems(int nblocks, int r) {
    return (int64_t)nblocks * DB * rm::width_for(std::min(r, rm::RV_MAX)) * 2;
}

template <typename T>
void launch_factor_update(const T* src, int64_t lds, T* dst, int64_t ldd, T* Linv, const T* X, int64_t ldx, int r,
                          int64_t f, int64_t shift, int64_t nlive, int b0, int nb, T* ws, int* info, Exec& ex,
                          hipStream_t s) {
    using namespace rm;
    GPRX_REQUIRE(r >= 1 && b0 >= 0 && b0 < nb && f >= (int64_t)b0 * DB && f < (int64_t)(b0 + 1) * DB && shift >= 0 &&
                     nlive >= 1 && nlive >= f && nlive <= (int64_t)nb * DB && ldd >= (int64_t)nb * DB && lds >= nlive + shift,
                 GPRX_ERR_ARG, "launch_factor_update: bad sizes");
    const int nblk = nb - b0;
    const size_t need = (size_t)C_NCTL + (size_t)nblk;
    int* scratch = ex.scratch_ints(need);
    const double tri = (double)nblk * (nblk + 1) / 2.0 * DB * DB;
    for (int v0 = 0; v0 < r; v0 += RV_MAX) {
        const int nv = std::min(RV_MAX, r - v0);
        ProfScope ps(KC_OTHER, s, 6.0 * nv * tri, 2.0 * sizeof(T) * tri);
        GPRX_HIP(hipMemsetAsync(scratch, 0, sizeof(int) * need, s));
        Args<T> a;
        std::memset(&a, 0, sizeof(a));
        a.src = v0 == 0 ? src : dst;  // further passes run in place on the new buffer
        a.lds = v0 == 0 ? lds : ldd;
        a.shift = v0 == 0 ? shift : 0;
        a.dst = dst;
        a.ldd = ldd;
        a.linv = v0 + nv == r ? Linv : nullptr;
        a.X = X + (int64_t)v0 * ldx;
        a.ldx = ldx;
        a.nv = nv;
        a.f = f;
        a.nlive = nlive;
        a.b0 = b0;
        a.nb = nb;
        a.cs = ws;
        a.ctl = scratch;
        a.info = info;
        a.tlimit = CHAIN_TLIMIT_TICKS;
        switch (width_for(nv)) {
            case 1: launch_rv<T, 1>(a, s); break;
            case 4: launch_rv<T, 4>(a, s); break;
            default: launch_rv<T, RV_MAX>(a, s); break;
        }
    }
}

#define GPRX_INST(T)                                                                                              \
    template void launch_factor_update<T>(const T*, int64_t, T*, int64_t, T*, const T*, int64_t, int, int64_t,      \
                                          int64_t, int64_t, int, int, T*, int*, Exec&, hipStream_t);
GPRX_INST(double)
GPRX_INST(float)
#undef GPRX_INST

}  // namespace gprx
