// k_sample.hip — what posterior sampling (gprx_model_sample, gprx_query.cpp) needs beside the
// launchers it shares with the fit and the variance call: a counter-based normal generator and
// the element-wise kernels around the sample transform
//     out[i, p, c] = mean[p, c] + sum_{r <= p} Lq[p, r] Z[(i m + c), r],
// whose product is launch_gemm_nt (k_gemm.hip) on GT multiples.  No product and no solve here.
//
// The generator is specified so that a numpy restatement reproduces it (tests/sample_ref.py):
// Philox4x32-10 (Salmon et al., SC'11; Random123's constants and round order) keyed by the seed's
// two halves, counter block c = (c low, c high, 0, 0) for the normals e = 2c and 2c + 1; with the
// output words w0..w3, u1 = (((w0 | w1 << 32) >> 11) + 0.5) 2^-53, u2 likewise from w2, w3,
// r = sqrt(-2 ln u1), normal 2c = r cos(2 pi u2), normal 2c + 1 = r sin(2 pi u2) (Box-Muller),
// always in fp64 and rounded once to T.  A normal depends on (seed, e) alone.
#include "gprx_internal.h"

namespace gprx {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t* w) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;  // (the key is bumped between rounds: the tenth bump is never used)
        k1 += 0xBB67AE85u;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}

__device__ __forceinline__ double unit_open(uint32_t lo, uint32_t hi) {  // in (0, 1): 53 bits, centred
    return ((double)((((uint64_t)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// One thread per counter block: the normals e = 2c and 2c + 1 as one 2-element store (out is
// count long, e-linear: consecutive lanes store consecutive pairs).
template <typename T>
__global__ __launch_bounds__(256) void normals_kernel(uint64_t seed, int64_t count, T* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x, e = 2 * c;
    if (e >= count) return;
    uint32_t w[4];
    philox4x32_10((uint32_t)c, (uint32_t)((uint64_t)c >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const double r = sqrt(-2.0 * log(unit_open(w[0], w[1])));
    double sn, cs;
    sincos(6.283185307179586 * unit_open(w[2], w[3]), &sn, &cs);
    const T z0 = (T)(r * cs), z1 = (T)(r * sn);
    if (e + 1 < count) {
        typedef T t2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<t2*>(out + e) = t2{z0, z1};  // (e even, out from hipMalloc: aligned)
    } else {
        out[e] = z0;
    }
}

// The normals z (ncols x q, row-major: z[col q + r], the order of the generator and of a caller's
// z) into the product's operand Zp[col + r ldz] (ldz x qp, both GT multiples), zero in the padding
// (Lq's padding columns are zeros, which a non-finite leftover would still turn into NaN).  32 x 32
// tiles transposed through LDS, so the reads run along r and the stores along col.
template <typename T>
__global__ __launch_bounds__(256) void stage_normals_kernel(const T* __restrict__ z, int64_t ncols, int64_t q,
                                                            T* __restrict__ Zp, int64_t ldz) {
    __shared__ T sh[32][33];
    const int64_t col0 = (int64_t)blockIdx.x * 32, r0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int64_t col = col0 + ty + 8 * k, r = r0 + tx;
        sh[ty + 8 * k][tx] = (col < ncols && r < q) ? z[col * q + r] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) Zp[col0 + tx + (r0 + ty + 8 * k) * ldz] = sh[tx][ty + 8 * k];
}

// The strict upper part of the n x n block L (column-major, ld) to zero: the tile factorisation
// leaves what it found there.  Column j's rows [0, j) are one run.
template <typename T>
__global__ __launch_bounds__(256) void zero_upper_kernel(T* __restrict__ L, int64_t ld) {
    const int64_t j = blockIdx.x, i = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (i < j) L[i + j * ld] = T(0);
}

// out[i, p, c] (nsamp x q x m, row-major) = mean[p, c] + C[p + (i m + c) ldc]: one thread per
// output element, so the stores are one run; for m = 1 the reads are too.
template <typename T>
__global__ __launch_bounds__(256) void sample_out_kernel(const T* __restrict__ C, int64_t ldc,
                                                         const T* __restrict__ mean, int64_t total, int64_t q, int m,
                                                         T* __restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int64_t t = o / m, c = o - t * m, i = t / q, p = t - i * q;
    out[o] = mean[p * m + c] + C[p + (i * m + c) * ldc];
}

template <typename T>
void launch_normals(uint64_t seed, int64_t count, T* out, hipStream_t s) {
    if (count <= 0) return;
    const int64_t nblk = (count + 1) / 2;
    hipLaunchKernelGGL(normals_kernel<T>, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, seed, count, out);
}

template <typename T>
void launch_stage_normals(const T* z, int64_t ncols, int64_t q, T* Zp, int64_t ldz, int64_t qp, hipStream_t s) {
    if (ldz <= 0 || qp <= 0) return;
    hipLaunchKernelGGL(stage_normals_kernel<T>, dim3((unsigned)(ldz / 32), (unsigned)(qp / 32)), dim3(256), 0, s, z,
                       ncols, q, Zp, ldz);
}

template <typename T>
void launch_zero_upper(T* L, int64_t ld, int64_t n, hipStream_t s) {
    if (n <= 1) return;
    hipLaunchKernelGGL(zero_upper_kernel<T>, dim3((unsigned)n, (unsigned)((n + 255) / 256)), dim3(256), 0, s, L, ld);
}

template <typename T>
void launch_sample_out(const T* C, int64_t ldc, const T* mean, int64_t nsamp, int64_t q, int m, T* out,
                       hipStream_t s) {
    const int64_t total = nsamp * q * m;
    if (total <= 0) return;
    hipLaunchKernelGGL(sample_out_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, C, ldc, mean,
                       total, q, m, out);
}

#define GPRX_INST(T)                                                                                     \
    template void launch_normals<T>(uint64_t, int64_t, T*, hipStream_t);                                 \
    template void launch_stage_normals<T>(const T*, int64_t, int64_t, T*, int64_t, int64_t, hipStream_t); \
    template void launch_zero_upper<T>(T*, int64_t, int64_t, hipStream_t);                               \
    template void launch_sample_out<T>(const T*, int64_t, const T*, int64_t, int64_t, int, T*, hipStream_t);
GPRX_INST(double)
GPRX_INST(float)
#undef GPRX_INST

}  // namespace gprx
