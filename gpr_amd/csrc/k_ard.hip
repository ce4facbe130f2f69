// k_ard.hip — per-dimension length scales (automatic relevance determination) on gfx950: the
// scaling of point sets and the gradient of the log marginal likelihood in the d length scales.
// Not in the reference, whose kernels are isotropic.
//
// A model with scales ell evaluates k_tree on z = x / ell.  Every r2 leaf sees a pair only through
// r2 = sum_j (z_aj - z_bj)^2, so with G_ab = dk_tree/dr2 at the pair and the likelihood's weights
// w_ab = alpha_a alpha_b - C_ab
//   dK_ab/d ell_j  = -(2 / ell_j) G_ab (z_aj - z_bj)^2
//   dLML/d ell_j   = 1/2 sum_ab w_ab dK_ab/d ell_j = -(1 / ell_j) g_j,
//   g_j            = sum_{a != b} H_ab (z_aj - z_bj)^2,   H = w o G.
// Per lower 128 x 128 tile (rows I, columns J; Ht = 2 H on the strict lower triangle, 0 elsewhere):
//   g_j += sum_a [ z_aj^2 R_a - 2 z_aj P_aj + Q_aj ],  R = Ht 1,  P = Ht Z_J,  Q = Ht (Z_J o Z_J)
// i.e. after the r2 statistic (the pair kernels' MFMA tile on the existing features) one more
// 128 x 128 x (2 d + 1) MFMA product with Ht as an operand, then row dots with Z_I.  The bracket is
// sum_b Ht_ab (z_aj - z_bj)^2 expanded: it cancels (its terms are 15 to 4000 times the result on the
// tested inputs), so it is combined and summed in double whatever T.
// z is read from the U features (k_pairs.hip: x~ = x - x_0 of the model's scaled points, columns
// padded with zeros to a multiple of 16): the identity holds for any common shift of z.
#include "k_pairs.h"

namespace gprx {
namespace ard {

using namespace mm;

constexpr int LDH = GT + PAD;  // Ht in LDS: column b at b LDH, rows contiguous
constexpr int NW = NT / 64;    // waves per workgroup = 16-row blocks of the second product

template <typename T>
__global__ void scale_points_kernel(const T* in, const T* __restrict__ ell, int64_t total, int d, T* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) out[i] = in[i] / ell[i % d];
}

template <typename T>
__global__ void unscale_deriv_kernel(T* __restrict__ der, const T* __restrict__ ell, int64_t total, int d, int m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) der[i] = der[i] / ell[(i / m) % d];
}

// value k and derivative g = dk/dr2 of one r2 leaf at E pairs (finite at r2 = 0 in every form)
template <typename T, int E, bool MAT>
__device__ __forceinline__ void leaf_kg(const KLeaf<T>* __restrict__ L, const T (&r2)[E], T (&k)[E], T (&g)[E]) {
    const int ty = L->type;
    const T c0 = L->c0, c1 = L->c1, c2 = L->c2;
    if (ty == L_RQ) {  // c0 (1 + c1 r2)^-c2
        const T m = -(c1 * c2);
#pragma unroll
        for (int e = 0; e < E; e++) {
            const T b = fma(c1, r2[e], T(1));
            k[e] = c0 * exp(-c2 * log(b));
            g[e] = m * k[e] / b;
        }
    } else if (MAT && ty == L_MATERN32) {  // c0 (1 + a) e^-a, a = sqrt(c1 r2)
        const T m = T(-0.5) * c0 * c1;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const T a = matern_arg(c1, r2[e]), ex = exp(-a);
            k[e] = fma(c0, a, c0) * ex;
            g[e] = m * ex;
        }
    } else if (MAT && ty == L_MATERN52) {  // c0 (1 + a + a^2 / 3) e^-a, c2 = c0 / 3
        const T m = T(-0.5) * c2 * c1;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const T a = matern_arg(c1, r2[e]), ex = exp(-a);
            k[e] = fma(a, fma(a, c2, c0), c0) * ex;
            g[e] = m * (T(1) + a) * ex;
        }
    } else if (ty == L_WHITE) {
#pragma unroll
        for (int e = 0; e < E; e++) {
            k[e] = r2[e] == T(0) ? c0 : T(0);
            g[e] = T(0);
        }
    } else {  // L_GAUSS, L_GAUSS_EXP: c0 e^(c1 r2)
#pragma unroll
        for (int e = 0; e < E; e++) {
            k[e] = c0 * exp(c1 * r2[e]);
            g[e] = c1 * k[e];
        }
    }
}

// One workgroup per lower tile; part[(tile NW + w) Kr + j] = wave w's share of the tile's g_j (its
// 16 rows), j < Kr (the columns d .. Kr - 1 are zero features: they give 0).
template <typename T, bool MAT>
__device__ __forceinline__ void ard_grad_body(const KCanon<T>* __restrict__ Kd, const T* __restrict__ FU,
                                              const T* __restrict__ FV, int64_t nf, int Kr,
                                              const T* __restrict__ alpha, const T* __restrict__ beta,
                                              const T* __restrict__ C, int64_t ldc, int64_t n,
                                              double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* smem = reinterpret_cast<T*>(smem_raw);
    static_assert(sizeof(T) * GT * LDH <= gemm_lds<T>(), "Ht takes the staging ring's place");
    typedef Mfma<T> Tr;
    int64_t ti, tj;
    {
        const int64_t b = blockIdx.x;
        int64_t i = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
        while ((i + 1) * (i + 2) / 2 <= b) i++;
        while (i * (i + 1) / 2 > b) i--;
        ti = i;
        tj = b - i * (i + 1) / 2;
    }
    const int64_t i0 = ti * GT, j0 = tj * GT;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = w & 1, wc = w >> 1, lr = lane & 15, lk = lane >> 4;
    const int nl = Kd->nleaf, nterm = Kd->nterm;
    auto each = [&](auto fn) {
        fn(std::integral_constant<int, 0>{});
        fn(std::integral_constant<int, 1>{});
        fn(std::integral_constant<int, 2>{});
        fn(std::integral_constant<int, 3>{});
        fn(std::integral_constant<int, 4>{});
        fn(std::integral_constant<int, 5>{});
        fn(std::integral_constant<int, 6>{});
        fn(std::integral_constant<int, 7>{});
    };
    // ---- r2 of the tile's pairs, then Ht in the accumulators' place ----
    typename Tr::acc_t ar[2][4];
    tile_mma<T, 0, false, BKS, FEED_EARLY>(ar, FU + i0, nf, FV + j0, nf, Kr, Kr, smem, t);
    T nu[4];
#pragma unroll
    for (int y = 0; y < 4; y++) nu[y] = FU[(int64_t)Kr * nf + i0 + wr * 64 + y * 16 + lr];
    each([&](auto cc) {
        constexpr int x = decltype(cc)::value >> 2, reg = decltype(cc)::value & 3;
        const int64_t gj = j0 + wc * 32 + x * 16 + Tr::orow(lk, reg);
        const T nv = FV[(int64_t)Kr * nf + gj];
        T r2[4], G[4];
#pragma unroll
        for (int y = 0; y < 4; y++) {
            r2[y] = pr::clamp0(nu[y] + nv + ar[x][y][reg]);
            G[y] = T(0);
        }
        // the product rule over the expanded tree, term by term: (p, dp) <- (p k, dp k + p g)
#pragma unroll 1
        for (int tm = 0; tm < nterm; tm++) {
            const unsigned msk = Kd->term_mask[tm];
            T p[4], dp[4];
#pragma unroll
            for (int y = 0; y < 4; y++) {
                p[y] = T(1);
                dp[y] = T(0);
            }
#pragma unroll 1
            for (int l = 0; l < nl; l++) {
                if (!(msk & (1u << l))) continue;
                T k[4], g[4];
                leaf_kg<T, 4, MAT>(&Kd->leaf[l], r2, k, g);
#pragma unroll
                for (int y = 0; y < 4; y++) {
                    dp[y] = fma(dp[y], k[y], p[y] * g[y]);
                    p[y] *= k[y];
                }
            }
#pragma unroll
            for (int y = 0; y < 4; y++) G[y] += dp[y];
        }
        // the weights: the strict lower triangle, doubled (the diagonal's (z_a - z_a)^2 is 0)
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const int64_t gi = i0 + wr * 64 + y * 16 + lr;
            const bool in = gi < n && gj < n && gi > gj;
            const int64_t ci = in ? gi : 0, cj = in ? gj : 0;
            const T wv = T(0.5) * fma(alpha[ci], beta[cj], alpha[cj] * beta[ci]) - C[ci + cj * ldc];
            ar[x][y][reg] = in ? T(2) * wv * G[y] : T(0);
        }
    });
    // ---- Ht through LDS into operand layout: every wave is past the ring ----
    __syncthreads();
    each([&](auto cc) {
        constexpr int x = decltype(cc)::value >> 2, reg = decltype(cc)::value & 3;
        const int col = wc * 32 + x * 16 + Tr::orow(lk, reg);
#pragma unroll
        for (int y = 0; y < 4; y++) smem[col * LDH + wr * 64 + y * 16 + lr] = ar[x][y][reg];
    });
    __syncthreads();
    // ---- wave w: rows 16 w .. 16 w + 15 of R, P, Q.  MFMA D[i][j] = sum_k Aop[i][k] Bop[k][j]:
    // Aop[i = feature column][k = b] = z_b (lane i = lr, k = lk), Bop[k = b][j = a] = Ht[a][b]
    // (lane j = lr, k = lk); lane lr then holds row a = lr, feature columns orow(lk, reg) ----
    T hf[GT / 4];
#pragma unroll
    for (int kb = 0; kb < GT / 4; kb++) hf[kb] = smem[(4 * kb + lk) * LDH + 16 * w + lr];
    typename Tr::acc_t accR = {0, 0, 0, 0};
#pragma unroll
    for (int kb = 0; kb < GT / 4; kb++) accR = Tr::mma(T(1), hf[kb], accR);
    const double Ra = (double)accR[0];  // (every feature row of D holds R_a)
    const int64_t ga = i0 + 16 * w + lr;
    double* __restrict__ out = part + ((int64_t)blockIdx.x * NW + w) * Kr;
#pragma unroll 1
    for (int jc0 = 0; jc0 < Kr; jc0 += 16) {
        const T* __restrict__ zb = FU + j0 + lk + (int64_t)(jc0 + lr) * nf;
        typename Tr::acc_t accP = {0, 0, 0, 0}, accQ = {0, 0, 0, 0};
#pragma unroll
        for (int kb = 0; kb < GT / 4; kb++) {
            const T zv = zb[4 * kb];
            accP = Tr::mma(zv, hf[kb], accP);
            accQ = Tr::mma(zv * zv, hf[kb], accQ);
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int jc = jc0 + Tr::orow(lk, reg);
            const double za = (double)FU[ga + (int64_t)jc * nf];
            double v = fma(za, fma(za, Ra, -2.0 * (double)accP[reg]), (double)accQ[reg]);
            // over the 16 rows (the lanes of one lk group), in a fixed order
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lr == 0) out[jc] = v;
        }
    }
}

#define GPRX_ARD_ARGS                                                                                             \
    const KCanon<T>*__restrict__ Kd, const T *__restrict__ FU, const T *__restrict__ FV, int64_t nf, int Kr,      \
        const T *__restrict__ alpha, const T *__restrict__ beta, const T *__restrict__ C, int64_t ldc, int64_t n, \
        double *__restrict__ part
template <typename T>
__global__ __launch_bounds__(NT) void ard_grad_kernel(GPRX_ARD_ARGS) {
    ard_grad_body<T, false>(Kd, FU, FV, nf, Kr, alpha, beta, C, ldc, n, part);
}
template <typename T>
__global__ __launch_bounds__(NT) void ard_grad_kernel_m(GPRX_ARD_ARGS) {
    ard_grad_body<T, true>(Kd, FU, FV, nf, Kr, alpha, beta, C, ldc, n, part);
}
#undef GPRX_ARD_ARGS

// gout[j] = sum over the nrows (tile, wave) rows of part[row Kr + j], in row order
__global__ void ard_reduce_kernel(const double* __restrict__ part, int64_t nrows, int Kr, double* __restrict__ gout) {
    __shared__ double red[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double v = 0;
    for (int64_t b = t; b < nrows; b += 256) v += part[b * Kr + j];
    red[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) gout[j] = red[0];
}

}  // namespace ard

template <typename T>
void launch_scale_points(const T* in, const T* ell, int64_t n, int d, T* out, hipStream_t s) {
    const int64_t total = n * d;
    if (total <= 0) return;
    hipLaunchKernelGGL(ard::scale_points_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, ell,
                       total, d, out);
    GPRX_HIP(hipGetLastError());
}

template <typename T>
void launch_unscale_deriv(T* der, const T* ell, int64_t q, int d, int m, hipStream_t s) {
    const int64_t total = q * d * m;
    if (total <= 0) return;
    hipLaunchKernelGGL(ard::unscale_deriv_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, der, ell,
                       total, d, m);
    GPRX_HIP(hipGetLastError());
}

template <typename T>
bool ard_grad_supported(const KCanon<T>& K) {
    if (!K.need_r2 || K.nper > 0) return false;
    for (int l = 0; l < K.nleaf; l++)
        if (K.leaf[l].type == L_PERIODIC) return false;
    return true;
}

int64_t ard_part_elems(int64_t nf, int d) {
    const int64_t nt = nf / GT;
    return nt * (nt + 1) / 2 * ard::NW * pr::rup(d, pr::KG);
}

template <typename T>
void launch_ard_grad(const KCanon<T>& K, const KCanon<T>* Kd, const T* FU, const T* FV, int64_t nf, int64_t n, int d,
                     const T* alpha, const T* beta, const T* C, int64_t ldc, double* part, double* gout,
                     hipStream_t s) {
    GPRX_REQUIRE(nf % GT == 0 && n <= nf && ard_grad_supported<T>(K), GPRX_ERR_ARG,
                 "launch_ard_grad: feature rows must be a multiple of 128 covering the samples, the tree r2 leaves only");
    const int Kr = pr::kr_of(K, d);
    const int64_t nt = nf / GT, ntiles = nt * (nt + 1) / 2;
    bool mat = false;
    for (int l = 0; l < K.nleaf; l++) mat |= K.leaf[l].type == L_MATERN32 || K.leaf[l].type == L_MATERN52;
    ProfScope ps(KC_LML_GRAD, s, 2.0 * (double)GT * GT * (Kr + 2.0 * Kr + 1.0) * ntiles,
                 (double)sizeof(T) * ((double)n * (n + 1) / 2 + (double)n * d));
    const size_t lds = mm::gemm_lds<T>();
    auto go = [&](auto kfn) {
        GPRX_HIP(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kfn, dim3((unsigned)ntiles), dim3(mm::NT), lds, s, Kd, FU, FV, nf, Kr, alpha, beta, C, ldc,
                           n, part);
    };
    mat ? go(ard::ard_grad_kernel_m<T>) : go(ard::ard_grad_kernel<T>);
    hipLaunchKernelGGL(ard::ard_reduce_kernel, dim3((unsigned)d), dim3(256), 0, s, (const double*)part,
                       ntiles * ard::NW, Kr, gout);
    GPRX_HIP(hipGetLastError());
}

#define GPRX_ARD_INST(T)                                                                                           \
    template void launch_scale_points<T>(const T*, const T*, int64_t, int, T*, hipStream_t);                       \
    template void launch_unscale_deriv<T>(T*, const T*, int64_t, int, int, hipStream_t);                           \
    template bool ard_grad_supported<T>(const KCanon<T>&);                                                         \
    template void launch_ard_grad<T>(const KCanon<T>&, const KCanon<T>*, const T*, const T*, int64_t, int64_t, int, \
                                     const T*, const T*, const T*, int64_t, double*, double*, hipStream_t);
GPRX_ARD_INST(float)
GPRX_ARD_INST(double)
#undef GPRX_ARD_INST

}  // namespace gprx
