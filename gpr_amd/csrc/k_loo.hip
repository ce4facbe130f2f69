// k_loo.hip — leave-one-out cross-validation of a fitted model on gfx950 (Rasmussen & Williams,
// GPML 5.4.2; not in the reference).
//
// With C = (K + sigma^2 I)^{-1}, c = diag(C) and alpha = C y the held-out predictions are
//   mu_i = y_i - alpha_i / c_i,   s2_i = 1 / c_i,
//   L    = sum_i log c_i / 2 - alpha_i^2 / (2 c_i) - log(2 pi) / 2
// and the gradient (m = 1) is sum_kl dK_kl/dp (a_k alpha_l - H_kl / 2) with u = alpha / c,
// a = C u, w = (1 + alpha^2 / c) / c, H = B B^T, B = C diag(sqrt w).  What this file computes:
//   - diag(C) WITHOUT C: c_i = sum_{k >= i} V_ik^2 over the rows of V = L^{-T} (upper,
//     column-major: threads along the rows, the zero triangle skipped);
//   - the vectors mu, s2, u, sqrt w and the value;
//   - B as the full square from the lower triangle of C (mirror and column scale in one pass
//     through LDS tiles, as sym_fill_kernel) and a = B (u / sqrt w) by its rows.
// H is a SYRK on the tile mainloop (launch_syrk_splitk) and the pair sum runs in the gradient
// kernels' two-vector mode (k_pairs.hip grad_mma_kernel2, k_lml.hip lml_grad_kernel2).
// Every reduction here has a fixed order, accumulates in double and uses no atomics: the
// results are the same bits on every call.
#include "gprx_internal.h"

namespace gprx {
namespace loo {

constexpr int CH = 128;  // rows per workgroup and columns per chunk of the row reductions

// part[c * np + i] = sum over the columns k of chunk c (k >= i when TRI) of
//   TRI: M[i + k ld]^2 (the squared row norms of an upper-triangular M; chunks left of the
//        row block hold zeros only and are neither read nor written)
//   else M[i + k ld] * r[k]
template <typename T, bool TRI>
__global__ __launch_bounds__(CH) void row_chunk_kernel(const T* __restrict__ M, int64_t ld, int64_t np,
                                                       const T* __restrict__ r, double* __restrict__ part) {
    const int64_t rb = blockIdx.x, c = blockIdx.y;
    if (TRI && c < rb) return;
    const int64_t i = rb * CH + threadIdx.x;  // (np is a multiple of CH: i < np)
    const int64_t k0 = c * CH, k1 = k0 + CH;
    double acc = 0.0;
    if (TRI) {
        for (int64_t k = (i > k0 ? i : k0); k < k1; k++) {
            const double v = (double)M[i + k * ld];
            acc = fma(v, v, acc);
        }
    } else {
#pragma unroll 8
        for (int64_t k = k0; k < k1; k++) acc = fma((double)M[i + k * ld], (double)r[k], acc);
    }
    part[c * np + i] = acc;
}

// out[i] = sum over the chunks c of part[c * np + i], in chunk order
template <typename T>
__global__ __launch_bounds__(256) void chunk_sum_kernel(const double* __restrict__ part, int64_t np, int nch,
                                                        T* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    double v = 0.0;
    for (int c = 0; c < nch; c++) v += part[(int64_t)c * np + i];
    out[i] = (T)v;
}

// One thread per sample (rows n .. np - 1: the gradient vectors' zero padding only).
template <typename T>
__global__ __launch_bounds__(256) void vectors_kernel(const T* __restrict__ alpha, const T* __restrict__ Y, int64_t n,
                                                      int64_t np, int m, const double* __restrict__ cpart,
                                                      const T* __restrict__ C, int64_t ldc, T* __restrict__ mean,
                                                      T* __restrict__ var, T* __restrict__ u, T* __restrict__ sw,
                                                      T* __restrict__ r, double* __restrict__ vpart) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + t;
    double term = 0.0;
    if (i < n) {
        double c = 0.0;
        if (cpart) {  // the chunks from the row's own on (row_chunk_kernel<TRI>), in order
            const int nch = (int)(np / CH);
            for (int ch = (int)(i / CH); ch < nch; ch++) c += cpart[(int64_t)ch * np + i];
        } else {
            c = (double)C[i + i * ldc];
        }
        const double ic = 1.0 / c, lc = 0.5 * log(c) - 0.91893853320467274178;  // log(2 pi) / 2
        if (var) var[i] = (T)ic;
        for (int q = 0; q < m; q++) {
            const double a = (double)alpha[i * m + q];
            if (mean) mean[i * m + q] = (T)((double)Y[i * m + q] - a * ic);
            term += lc - 0.5 * a * a * ic;
        }
        if (u) {  // (m = 1)
            const double a = (double)alpha[i], uu = a * ic, w = (1.0 + a * a * ic) * ic, s = sqrt(w);
            u[i] = (T)uu;
            sw[i] = (T)s;
            r[i] = (T)(uu / s);
        }
    } else if (i < np && u) {
        u[i] = sw[i] = r[i] = T(0);
    }
    red[t] = term;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) vpart[blockIdx.x] = red[0];
}

// value[0] = sum of the workgroups' partials, in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void value_sum_kernel(const double* __restrict__ vpart, int64_t nblk,
                                                        double* __restrict__ value) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double v = 0.0;
    for (int64_t b = t; b < nblk; b += 256) v += vpart[b];
    red[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) value[0] = red[0];
}

// B(i, j) = sym(C)(i, j) sw[j] for the 32 x 32 tile (rows bx, columns by) of the full square:
// the tile of the lower triangle it comes from goes through LDS, transposed when the destination
// lies above the diagonal, so the reads and the writes are both column runs.  Of a diagonal tile
// only the entries on and below the diagonal are read (the upper triangle of C is never written).
template <typename T>
__global__ __launch_bounds__(256) void sym_scale_kernel(const T* __restrict__ C, int64_t ldc,
                                                        const T* __restrict__ sw, T* __restrict__ B, int64_t ldb) {
    const int64_t bx = blockIdx.x, by = blockIdx.y;
    __shared__ T sh[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const bool upper = bx < by;
    const int64_t sr = (upper ? by : bx) * 32, sc = (upper ? bx : by) * 32;  // the source tile (lower)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = ty + 8 * k;
        if (bx != by || tx >= c) sh[c][tx] = C[sr + tx + (sc + c) * ldc];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = ty + 8 * k;
        T v;
        if (upper) v = sh[tx][c];
        else if (bx == by && tx < c) v = sh[tx][c];
        else v = sh[c][tx];
        B[bx * 32 + tx + (by * 32 + c) * ldb] = v * sw[by * 32 + c];
    }
}

}  // namespace loo

int64_t loo_part_elems(int64_t np) { return (np / loo::CH) * np; }

template <typename T>
void launch_loo_diag(const T* V, int64_t np, double* part, hipStream_t s) {
    if (np <= 0) return;
    GPRX_REQUIRE(np % loo::CH == 0, GPRX_ERR_ARG, "launch_loo_diag: the padded size must be a multiple of 128");
    const unsigned nb = (unsigned)(np / loo::CH);
    ProfScope ps(KC_OTHER, s, (double)np * np, (double)sizeof(T) * (double)np * np / 2);
    hipLaunchKernelGGL((loo::row_chunk_kernel<T, true>), dim3(nb, nb), dim3(loo::CH), 0, s, V, np, np,
                       (const T*)nullptr, part);
    GPRX_HIP(hipGetLastError());
}

template <typename T>
void launch_loo_vectors(const T* alpha, const T* Y, int64_t n, int64_t np, int m, const double* cpart, const T* C,
                        int64_t ldc, T* mean, T* var, T* u, T* sw, T* r, double* vpart, double* value, hipStream_t s) {
    if (np <= 0) return;
    const unsigned nblk = (unsigned)((np + 255) / 256);
    hipLaunchKernelGGL(loo::vectors_kernel<T>, dim3(nblk), dim3(256), 0, s, alpha, Y, n, np, m, cpart, C, ldc, mean, var,
                       u, sw, r, vpart);
    hipLaunchKernelGGL(loo::value_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)vpart, (int64_t)nblk, value);
    GPRX_HIP(hipGetLastError());
}

template <typename T>
void launch_loo_weights(const T* C, int64_t ldc, int64_t np, const T* sw, const T* r, T* B, double* part, T* a,
                        hipStream_t s) {
    if (np <= 0) return;
    GPRX_REQUIRE(np % loo::CH == 0, GPRX_ERR_ARG, "launch_loo_weights: the padded size must be a multiple of 128");
    const unsigned nt = (unsigned)(np / 32), nb = (unsigned)(np / loo::CH);
    ProfScope ps(KC_OTHER, s, 2.0 * (double)np * np, (double)sizeof(T) * 2.5 * (double)np * np);
    hipLaunchKernelGGL(loo::sym_scale_kernel<T>, dim3(nt, nt), dim3(256), 0, s, C, ldc, sw, B, np);
    hipLaunchKernelGGL((loo::row_chunk_kernel<T, false>), dim3(nb, nb), dim3(loo::CH), 0, s, (const T*)B, np, np, r,
                       part);
    hipLaunchKernelGGL(loo::chunk_sum_kernel<T>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s,
                       (const double*)part, np, (int)nb, a);
    GPRX_HIP(hipGetLastError());
}

#define GPRX_INST(T)                                                                                              \
    template void launch_loo_diag<T>(const T*, int64_t, double*, hipStream_t);                                    \
    template void launch_loo_vectors<T>(const T*, const T*, int64_t, int64_t, int, const double*, const T*, int64_t, \
                                        T*, T*, T*, T*, T*, double*, double*, hipStream_t);                       \
    template void launch_loo_weights<T>(const T*, int64_t, int64_t, const T*, const T*, T*, double*, T*, hipStream_t);
GPRX_INST(double)
GPRX_INST(float)
#undef GPRX_INST

}  // namespace gprx
