// k_gemm.hip — the general MFMA GEMM  C = beta C + alpha A B^T  on gfx950 (all column-major,
// M and N multiples of 128, K a multiple of 16).
//
// The GEMM of everything around the factorisation (which has its own tile mainloop, k_mma.h):
// the row solves of predict and the posterior (k_predict.hip trsm_rows), the explicit inverse of
// the LML gradient (k_lml.hip) and of a fit that asks for it (gprx_fit.cpp), the sparse GP
// (gprx_sparse.cpp, gprx_query.cpp), append's Schur complement (gprx_fit.cpp) and the LU
// fallback's trailing update (k_getrf.hip).
//   launch_gemm_nt         full or lower-triangle product, optional accumulation (beta)
//   launch_gemm_nt_splitk  P partial products over slices of K in one launch (grid.y)
//   launch_gemm_nt_kskip   lower C = V V^T with V upper triangular (skips the zero columns)
// gemm_nt_kernel is LDS double-buffered: v_mfma_f64_16x16x4_f64 (fp64) or v_mfma_f32_16x16x4_f32
// (fp32), one output tile per 256-thread workgroup, K staged 16 deep.  Tile rule (launch_gemm_nt):
// 128 x 128 tiles (4 waves of 64 x 64) when they give at least GPRX_SMALL_TILE_WG (1024)
// workgroups, 64 x 64 tiles (4 waves of 32 x 32, four times the workgroups) below that, so a small
// product still spreads over the chip; an in-place product always takes 128-row tiles (see there).
// A full product of at least twice that many tiles goes to launch_gemm_tall's 256 x 128 tiles
// (k_syrk.hip) when its shape allows.
#include "gprx_internal.h"

#include <cstdlib>

namespace gprx {

constexpr int BK = 16;
constexpr int PADT = 16;

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));
typedef float f4v_t __attribute__((ext_vector_type(4)));

template <typename T>
struct MfmaTraits;
template <>
struct MfmaTraits<double> {
    typedef d4_t acc_t;
    typedef d2_t vec_t;  // 16-byte global/LDS move
    static constexpr int VEC = 2;
    __device__ static inline acc_t mma(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // output row (within the 16x16 block) of accumulator register `reg` for lane group lk
    __device__ static inline int orow(int lk, int reg) { return lk + 4 * reg; }
};
template <>
struct MfmaTraits<float> {
    typedef f4_t acc_t;
    typedef f4v_t vec_t;
    static constexpr int VEC = 4;
    __device__ static inline acc_t mma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    __device__ static inline int orow(int lk, int reg) { return 4 * lk + reg; }
};

// TM = 128: 4 waves of 64x64 (4x4 MFMA blocks each) -- the large products.
// TM = 64:  4 waves of 32x32 (2x2 blocks) -- small products, 4x the workgroups so a short
//           launch spreads over the whole chip instead of running 64-128 long tiles.
template <typename T, bool LOWER, bool BETA, bool KSKIP, int TM = 128>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(T* __restrict__ C, int64_t ldc, const T* __restrict__ A,
                                                         int64_t lda, const T* __restrict__ B, int64_t ldb,
                                                         int64_t K, T alpha, T beta, int64_t ntm, int64_t ntn,
                                                         int64_t cstride = 0) {
    typedef MfmaTraits<T> Tr;
    typedef typename Tr::acc_t acc_t;
    typedef typename Tr::vec_t vec_t;
    constexpr int VEC = Tr::VEC;
    constexpr int SR = TM + PADT;       // LDS row (one k) length in elements
    constexpr int TPC = TM / VEC;       // threads per staged column
    constexpr int CPP = 256 / TPC;      // columns per pass
    constexpr int PASSES = (BK + CPP - 1) / CPP;
    constexpr int NB = TM / 32;         // 16x16 MFMA blocks per wave edge (4 or 2)
    constexpr int WT = TM / 2;          // wave tile edge

    // split-K: blockIdx.y = p works on k in [p*K, (p+1)*K) and writes its own C + p*cstride
    if (gridDim.y > 1) {
        const int64_t p = blockIdx.y;
        A += p * K * lda;
        B += p * K * ldb;
        C += p * cstride;
    }

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* sA = reinterpret_cast<T*>(smem_raw);            // [2][BK][SR]
    T* sB = sA + 2 * BK * SR;                            // [2][BK][SR]

    // ---- tile coordinates ---------------------------------------------------------------
    int64_t ti, tj;
    {
        const int64_t b = blockIdx.x;
        if (LOWER) {
            const int64_t tri = ntn * (ntn + 1) / 2;
            if (b < tri) {
                int64_t i = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
                while ((i + 1) * (i + 2) / 2 <= b) i++;
                while (i * (i + 1) / 2 > b) i--;
                ti = i;
                tj = b - i * (i + 1) / 2;
            } else {
                const int64_t b2 = b - tri;
                ti = ntn + b2 / ntn;
                tj = b2 % ntn;
            }
        } else {
            ti = b % ntm;
            tj = b / ntm;
        }
    }
    const int64_t i0 = ti * TM, j0 = tj * TM;
    // KSKIP: both operands are zero left of column i0 (C = V V^T with V upper triangular)
    const int64_t kbeg = KSKIP ? i0 : 0;
    const T* Ablk = A + i0 + kbeg * lda;
    const T* Bblk = B + j0 + kbeg * ldb;

    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int lr = lane & 15, lk = lane >> 4;

    // staging coordinates
    const int st_row = (t % TPC) * VEC;
    const int st_col = t / TPC;

    vec_t ra[PASSES], rb[PASSES];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int64_t kk = k0 + st_col + p * CPP;
            if (st_col + p * CPP < BK) {
                ra[p] = *reinterpret_cast<const vec_t*>(Ablk + st_row + kk * lda);
                rb[p] = *reinterpret_cast<const vec_t*>(Bblk + st_row + kk * ldb);
            }
        }
    };
    auto lstore = [&](int buf) {
        T* a = sA + buf * BK * SR;
        T* bb = sB + buf * BK * SR;
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const int kk = st_col + p * CPP;
            if (kk < BK) {
                *reinterpret_cast<vec_t*>(a + kk * SR + st_row) = ra[p];
                *reinterpret_cast<vec_t*>(bb + kk * SR + st_row) = rb[p];
            }
        }
    };

    acc_t acc[NB][NB];
#pragma unroll
    for (int x = 0; x < NB; x++)
#pragma unroll
        for (int y = 0; y < NB; y++) acc[x][y] = acc_t{0};

    const int nstage = (int)((K - kbeg) / BK);
    gload(0);
    lstore(0);
    __syncthreads();
    for (int sidx = 0; sidx < nstage; sidx++) {
        const int buf = sidx & 1;
        if (sidx + 1 < nstage) gload((int64_t)(sidx + 1) * BK);
        const T* a = sA + buf * BK * SR;
        const T* bb = sB + buf * BK * SR;
#pragma unroll
        for (int kq = 0; kq < BK / 4; kq++) {
            const int kr = kq * 4 + lk;
            T fa[NB], fb[NB];
#pragma unroll
            for (int x = 0; x < NB; x++) fb[x] = bb[kr * SR + wc * WT + x * 16 + lr];  // MFMA A: our columns
#pragma unroll
            for (int y = 0; y < NB; y++) fa[y] = a[kr * SR + wr * WT + y * 16 + lr];   // MFMA B: our rows
#pragma unroll
            for (int x = 0; x < NB; x++)
#pragma unroll
                for (int y = 0; y < NB; y++) acc[x][y] = Tr::mma(fb[x], fa[y], acc[x][y]);
        }
        if (sidx + 1 < nstage) lstore(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: acc[x][y][reg] = C(i = ... y*16 + lr, j = ... x*16 + orow(lk, reg)) ----
    const bool diag_tile = LOWER && (ti == tj);
#pragma unroll
    for (int x = 0; x < NB; x++) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int jl = wc * WT + x * 16 + Tr::orow(lk, reg);
            T* ccol = C + (j0 + jl) * ldc + i0;
#pragma unroll
            for (int y = 0; y < NB; y++) {
                const int il = wr * WT + y * 16 + lr;
                if (diag_tile && il < jl) continue;
                T v = alpha * acc[x][y][reg];
                if (BETA) v = fma(beta, ccol[il], v);
                ccol[il] = v;
            }
        }
    }
}

template <typename T, int TM = 128>
static size_t gemm_lds_bytes() {
    return sizeof(T) * 4 * BK * (TM + PADT);
}

template <typename T, int TM>
static void gemm_launch(T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t M, int64_t N,
                        int64_t K, T alpha, T beta, bool lower, hipStream_t s) {
    const int64_t ntm = M / TM, ntn = N / TM;
    const int64_t ntiles = lower ? ntn * (ntn + 1) / 2 + (ntm - ntn) * ntn : ntm * ntn;
    const size_t lds = gemm_lds_bytes<T, TM>();
    const bool use_beta = beta != T(0);
#define GPRX_GEMM(L, Bt)                                                                                  \
    do {                                                                                                  \
        static bool attr_done = false;                                                                    \
        if (!attr_done) {                                                                                 \
            hipFuncSetAttribute((const void*)gemm_nt_kernel<T, L, Bt, false, TM>,                         \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                    \
            attr_done = true;                                                                             \
        }                                                                                                 \
        hipLaunchKernelGGL((gemm_nt_kernel<T, L, Bt, false, TM>), dim3((unsigned)ntiles), dim3(256), lds, s, C, ldc, \
                           A, lda, B, ldb, K, alpha, beta, ntm, ntn, (int64_t)0);                         \
    } while (0)
    if (lower) {
        if (use_beta) GPRX_GEMM(true, true);
        else GPRX_GEMM(true, false);
    } else {
        if (use_beta) GPRX_GEMM(false, true);
        else GPRX_GEMM(false, false);
    }
#undef GPRX_GEMM
}

// Tile choice: 128x128 tiles when they give at least GPRX_SMALL_TILE_WG workgroups, 64x64 tiles
// otherwise (the latency-bound small launches); the largest full products go to launch_gemm_tall.
template <typename T>
void launch_gemm_nt(T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t M, int64_t N,
                    int64_t K, T alpha, T beta, bool lower, hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    const bool use_beta = beta != T(0);
    const double elems = lower ? ((double)N * (N + 1) / 2 + (double)(M - N) * N) : (double)M * N;
    ProfScope ps(lower ? KC_UPDATE : (use_beta ? KC_OTHER : KC_TRSM), s, 2.0 * elems * K,
                 (double)sizeof(T) * (elems * (use_beta ? 2 : 1) + (double)(M + N) * K));
    static const int64_t small_tiles = [] {
        const char* e = std::getenv("GPRX_SMALL_TILE_WG");
        return e ? (int64_t)std::atoll(e) : (int64_t)1024;
    }();
    const int64_t ntm = M / GT, ntn = N / GT;
    const int64_t nt128 = lower ? ntn * (ntn + 1) / 2 + (ntm - ntn) * ntn : ntm * ntn;
    // in place (C = A B^T over A's own columns: the row solves' diagonal-block products, k_predict.hip
    // trsm_rows, k_lml.hip): every workgroup must own WHOLE rows, so that no
    // other workgroup still reads the columns it overwrites -- with 64 x 64 tiles the workgroup of
    // columns 64..127 could read columns 0..63 after its neighbour stored them (an intermittent
    // error in a 64-row block of the result).  128 columns at most, the 128 (or 256) row tile.
    const bool inplace = (const void*)C == (const void*)A;
    GPRX_REQUIRE(!inplace || (ldc == lda && N <= GT && !lower), GPRX_ERR_ARG,
                 "gprx: launch_gemm_nt in place needs ldc == lda, N <= 128, a full product");
    if (!lower && nt128 >= 2 * small_tiles && launch_gemm_tall<T>(C, ldc, A, lda, B, ldb, M, N, K, alpha, beta, s))
        return;
    if (nt128 < small_tiles && !inplace)
        gemm_launch<T, 64>(C, ldc, A, lda, B, ldb, M, N, K, alpha, beta, lower, s);
    else
        gemm_launch<T, 128>(C, ldc, A, lda, B, ldb, M, N, K, alpha, beta, lower, s);
}

// Split-K form: P partial products, partial p = A[:, pK:(p+1)K] B[:, pK:(p+1)K]^T accumulated
// (beta = 1) into C + p*cstride, all in one launch (grid.y = P); K is the slice depth.
template <typename T>
void launch_gemm_nt_splitk(T* C, int64_t ldc, int64_t cstride, const T* A, int64_t lda, const T* B, int64_t ldb,
                           int64_t M, int64_t N, int64_t K, int P, T alpha, bool lower, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0) return;
    const int64_t ntm = M / GT, ntn = N / GT;
    const int64_t ntiles = lower ? ntn * (ntn + 1) / 2 + (ntm - ntn) * ntn : ntm * ntn;
    const size_t lds = gemm_lds_bytes<T, 128>();
    const double elems = lower ? ((double)N * (N + 1) / 2 + (double)(M - N) * N) : (double)M * N;
    ProfScope ps(KC_OTHER, s, 2.0 * elems * K * P, (double)sizeof(T) * (2 * elems * P + (double)(M + N) * K * P));
#define GPRX_GEMM_SK(L)                                                                                      \
    do {                                                                                                     \
        static bool attr_done = false;                                                                       \
        if (!attr_done) {                                                                                    \
            hipFuncSetAttribute((const void*)gemm_nt_kernel<T, L, true, false>,                              \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                       \
            attr_done = true;                                                                                \
        }                                                                                                    \
        hipLaunchKernelGGL((gemm_nt_kernel<T, L, true, false>), dim3((unsigned)ntiles, (unsigned)P), dim3(256), \
                           lds, s, C, ldc, A, lda, B, ldb, K, alpha, T(1), ntm, ntn, cstride);               \
    } while (0)
    if (lower) GPRX_GEMM_SK(true);
    else GPRX_GEMM_SK(false);
#undef GPRX_GEMM_SK
}

// C (lower) = A B^T where both operands vanish left of their row (LAUUM shape).
template <typename T>
void launch_gemm_nt_kskip(T* C, int64_t ldc, const T* A, int64_t lda, const T* B, int64_t ldb, int64_t M, int64_t N,
                          int64_t K, hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    const int64_t ntm = M / GT, ntn = N / GT;
    const int64_t ntiles = ntn * (ntn + 1) / 2 + (ntm - ntn) * ntn;
    const size_t lds = gemm_lds_bytes<T, 128>();
    ProfScope ps(KC_INVERSE, s, 2.0 * (double)N * N * N / 6.0, 0.0);
    static bool attr_done = false;
    if (!attr_done) {
        hipFuncSetAttribute((const void*)gemm_nt_kernel<T, true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
        attr_done = true;
    }
    hipLaunchKernelGGL((gemm_nt_kernel<T, true, false, true>), dim3((unsigned)ntiles), dim3(256), lds, s, C, ldc, A, lda,
                       B, ldb, K, T(1), T(0), ntm, ntn);
}

#define GPRX_INST(T) \
    template void launch_gemm_nt_splitk<T>(T*, int64_t, int64_t, const T*, int64_t, const T*, int64_t,   \
                                           int64_t, int64_t, int64_t, int, T, bool, hipStream_t);         \
    template void launch_gemm_nt<T>(T*, int64_t, const T*, int64_t, const T*, int64_t, int64_t, int64_t, \
                                    int64_t, T, T, bool, hipStream_t);                                    \
    template void launch_gemm_nt_kskip<T>(T*, int64_t, const T*, int64_t, const T*, int64_t, int64_t, int64_t,   \
                                          int64_t, hipStream_t);
GPRX_INST(double)
GPRX_INST(float)
#undef GPRX_INST

}  // namespace gprx
