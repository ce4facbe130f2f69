// gprx_dev.cpp — developer timing hooks (include/gprx_dev.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gprx_dev.h"
#include "gprx_model.h"
#include "pt_sched.h"
#include "sparse_plan.h"

using namespace gprx;

template <typename T>
__global__ void dev_fill_spd(T* A, int64_t ld, int64_t n, uint64_t seed) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ld * n) return;
    int64_t i = e % ld, j = e / ld;
    uint64_t z = (uint64_t)e * 0x9E3779B97F4A7C15ull + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    T v = (T)((double)(z >> 11) * (1.0 / 9007199254740992.0)) * T(1e-3);
    if (i == j) v += T(n);  // diagonally dominant -> SPD
    A[e] = v;
}

__global__ void dev_fexp_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = fexp(x[i]);
}

template <typename T>
static gprx_status bench_impl(int what, int64_t M, int64_t N, int64_t K, int iters, double* ms, Exec& ex) {
    hipStream_t s = ex.s0;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    std::vector<void*> bufs;
    auto alloc = [&](size_t b) {
        void* p = nullptr;
        if (dev_malloc(&p, b) != hipSuccess) throw Error{GPRX_ERR_OOM, "dev bench: hipMalloc failed"};
        bufs.push_back(p);
        return p;
    };
    int* info = (int*)alloc(sizeof(int));
    float tms = 0;
    try {
        if (what == 11 || what == 12 || what == 13) {  // tile-engine diagonal factor (k_ptiles.hip), variant what - 11:
            // ms[0] = us per factor (events), ms[1..5] = per-factor phase ticks (100 MHz)
            const int reps = std::max(1, iters);
            T* A = (T*)alloc(sizeof(T) * DB * DB * (size_t)reps);
            T* L = (T*)alloc(sizeof(T) * DB * DB);
            long long* pr = (long long*)alloc(sizeof(long long) * 8);
            (void)hipMemsetAsync(pr, 0, sizeof(long long) * 8, s);
            for (int it = 0; it < reps; it++)
                hipLaunchKernelGGL(dev_fill_spd<T>, dim3((DB * DB + 255) / 256), dim3(256), 0, s, A + (size_t)it * DB * DB,
                                   (int64_t)DB, (int64_t)DB, (uint64_t)it);
            (void)hipMemsetAsync(info, 0x7f, sizeof(int), s);
            pt::launch_diag_bench<T>(what - 11, A, DB, L, info, pr, 1, s);  // warm (factors block 0 in place)
            for (int it = 0; it < 1; it++)
                hipLaunchKernelGGL(dev_fill_spd<T>, dim3((DB * DB + 255) / 256), dim3(256), 0, s, A, (int64_t)DB,
                                   (int64_t)DB, (uint64_t)0);
            (void)hipEventRecord(e0, s);
            pt::launch_diag_bench<T>(what - 11, A, DB, L, info, pr, reps, s);
            (void)hipEventRecord(e1, s);
            (void)hipEventSynchronize(e1);
            (void)hipEventElapsedTime(&tms, e0, e1);
            long long h[8];
            (void)hipMemcpy(h, pr, sizeof(h), hipMemcpyDeviceToHost);
            ms[0] = 1e3 * tms / reps;
            for (int i = 0; i < 8; i++) ms[1 + i] = (double)h[i] / reps;
        } else if (what == 1 || what == 2) {
            const int64_t ld = M;
            T* C = (T*)alloc(sizeof(T) * ld * N);
            T* A = (T*)alloc(sizeof(T) * ld * K);
            T* B = (T*)alloc(sizeof(T) * N * K);
            (void)hipMemset(C, 0, sizeof(T) * ld * N);
            (void)hipMemset(A, 0, sizeof(T) * ld * K);
            (void)hipMemset(B, 0, sizeof(T) * N * K);
            hipLaunchKernelGGL(dev_fill_spd<T>, dim3((unsigned)((ld * K + 255) / 256)), dim3(256), 0, s, A, ld, K,
                               (uint64_t)1);
            hipLaunchKernelGGL(dev_fill_spd<T>, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, s, B, N, K,
                               (uint64_t)2);
            launch_gemm_nt<T>(C, ld, A, ld, B, N, M, N, K, T(-1), T(1), what == 2, s);
            (void)hipEventRecord(e0, s);
            for (int it = 0; it < iters; it++) launch_gemm_nt<T>(C, ld, A, ld, B, N, M, N, K, T(-1), T(1), what == 2, s);
            (void)hipEventRecord(e1, s);
            (void)hipEventSynchronize(e1);
            (void)hipEventElapsedTime(&tms, e0, e1);
            *ms = tms / iters;
        } else if (what == 5 || what == 9 || what == 10) {
            // 9: the tile factorisation; 5 / 10: the per-block / chained back substitution of its
            // factor (the factorisation outside the timed region)
            const int64_t n = M;
            T* A = (T*)alloc(sizeof(T) * n * n);
            T* Li = (T*)alloc(sizeof(T) * n * DB);
            T* z = (T*)alloc(sizeof(T) * n);
            T* al = (T*)alloc(sizeof(T) * n);
            double total = 0;
            for (int it = 0; it < iters + 1; it++) {
                hipLaunchKernelGGL(dev_fill_spd<T>, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, s, A, n, n,
                                   (uint64_t)it);
                (void)hipMemsetD32Async((hipDeviceptr_t)info, INT_MAX, 1, s);
                if (what == 5 || what == 10) potrf_tiles<T>(A, n, n, n, Li, info, ex);
                (void)hipEventRecord(e0, s);
                if (what == 5) launch_backsolve<T>(A, n, n - DB, 1, Li, z, al, s);
                else if (what == 10) launch_backsolve_chain<T>(A, n, n - DB, 1, Li, al, info, ex, s);
                else potrf_tiles<T>(A, n, n, n, Li, info, ex);
                (void)hipEventRecord(e1, s);
                (void)hipEventSynchronize(e1);
                (void)hipEventElapsedTime(&tms, e0, e1);
                if (it > 0) total += tms;
            }
            *ms = total / iters;
        } else {
            throw Error{GPRX_ERR_ARG, "dev bench: unknown case"};
        }
        if (hipDeviceSynchronize() != hipSuccess) throw Error{GPRX_ERR_HIP, "dev bench: device error"};
    } catch (const Error& e) {
        for (void* p : bufs) (void)hipFree(p);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return e.st;
    }
    for (void* p : bufs) (void)hipFree(p);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return GPRX_OK;
}

// gprx_dev_forward_panel: the chained thin-panel solve (k_append.hip) or trsm_rows on a host
// factor.  The diagonal blocks' inverses are formed on the host in double (forward substitution
// of the identity).  The chained path's panel sits inside guard rows and columns of a fixed bit
// pattern, compared bitwise afterwards: the kernel must touch rows < `rows` of its columns only.
namespace gprx {
template <typename T>
void trsm_rows(const T* A, int64_t ldA, int64_t np, const T* Linv, T* R, int64_t ld, int64_t qp, hipStream_t s);

template <typename T>
static gprx_status forward_panel_impl(const void* Lh, int64_t n, void* Rh, int rows, int use_gemm, Exec& ex,
                                      hipStream_t s) {
    GPRX_REQUIRE(Lh && Rh && n > 0 && n % DB == 0 && rows >= 1 && rows <= DB, GPRX_ERR_ARG,
                 "gprx_dev_forward_panel: n must be a positive multiple of 128 and 1 <= rows <= 128");
    const T* L = static_cast<const T*>(Lh);
    T* R = static_cast<T*>(Rh);
    const int64_t nb = n / DB;
    std::vector<T> hA((size_t)n * n, T(0)), hLi((size_t)n * DB, T(0));
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = 0; j <= i; j++) hA[(size_t)i + (size_t)j * n] = L[(size_t)i * n + j];
    std::vector<double> inv((size_t)DB * DB);
    for (int64_t b = 0; b < nb; b++) {
        const int64_t o = b * DB;
        std::fill(inv.begin(), inv.end(), 0.0);
        for (int c = 0; c < DB; c++)  // column c of the inverse: L x = e_c
            for (int r = c; r < DB; r++) {
                double v = (r == c) ? 1.0 : 0.0;
                for (int q = c; q < r; q++) v -= (double)L[(size_t)(o + r) * n + o + q] * inv[(size_t)q + (size_t)c * DB];
                inv[(size_t)r + (size_t)c * DB] = v / (double)L[(size_t)(o + r) * n + o + r];
            }
        for (size_t e = 0; e < (size_t)DB * DB; e++) hLi[(size_t)b * DB * DB + e] = (T)inv[e];
    }
    // the panel: guard rows below it and DB guard columns on either side
    const int64_t gr = use_gemm ? 0 : 16, gc = use_gemm ? 0 : DB;
    const int64_t ldr = (use_gemm ? (int64_t)DB : (int64_t)((rows + 15) / 16 * 16)) + gr, ncb = n + 2 * gc;
    T guard;
    std::memset(&guard, 0x5a, sizeof(T));
    std::vector<T> hR((size_t)ldr * ncb, use_gemm ? T(0) : guard);
    for (int64_t r = 0; r < rows; r++)
        for (int64_t c = 0; c < n; c++) hR[(size_t)r + (size_t)(c + gc) * ldr] = R[(size_t)r * n + c];
    std::vector<T> before = hR;
    T *dA = nullptr, *dLi = nullptr, *dR = nullptr;
    int* dinfo = nullptr;
    gprx_status st = GPRX_OK;
    std::string msg;
    try {
        GPRX_HIP(dev_malloc(&dA, sizeof(T) * hA.size()));
        GPRX_HIP(dev_malloc(&dLi, sizeof(T) * hLi.size()));
        GPRX_HIP(dev_malloc(&dR, sizeof(T) * hR.size()));
        GPRX_HIP(dev_malloc(&dinfo, sizeof(int)));
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipMemcpy(dA, hA.data(), sizeof(T) * hA.size(), hipMemcpyHostToDevice));
        GPRX_HIP(hipMemcpy(dLi, hLi.data(), sizeof(T) * hLi.size(), hipMemcpyHostToDevice));
        GPRX_HIP(hipMemcpy(dR, hR.data(), sizeof(T) * hR.size(), hipMemcpyHostToDevice));
        const int big = INT_MAX;
        GPRX_HIP(hipMemcpy(dinfo, &big, sizeof(int), hipMemcpyHostToDevice));
        if (use_gemm) trsm_rows<T>(dA, n, n, dLi, dR, ldr, ldr, s);
        else launch_forward_panel_chain<T>(dA, n, n, dLi, dR + gc * ldr, ldr, rows, dinfo, ex, s);
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipGetLastError());
        int hinfo = 0;
        GPRX_HIP(hipMemcpy(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost));
        GPRX_HIP(hipMemcpy(hR.data(), dR, sizeof(T) * hR.size(), hipMemcpyDeviceToHost));
        GPRX_REQUIRE(hinfo >= 0, GPRX_ERR_HIP, "gprx_dev_forward_panel: a chained wait timed out");
        if (!use_gemm)
            for (int64_t c = 0; c < ncb; c++)
                for (int64_t r = 0; r < ldr; r++) {
                    if (r < rows && c >= gc && c < gc + n) continue;
                    const size_t e = (size_t)r + (size_t)c * ldr;
                    GPRX_REQUIRE(std::memcmp(&hR[e], &before[e], sizeof(T)) == 0, GPRX_ERR_HIP,
                                 "gprx_dev_forward_panel: the kernel wrote outside its panel (row " +
                                     std::to_string(r) + ", column " + std::to_string(c - gc) + ")");
                }
        for (int64_t r = 0; r < rows; r++)
            for (int64_t c = 0; c < n; c++) R[(size_t)r * n + c] = hR[(size_t)r + (size_t)(c + gc) * ldr];
    } catch (const Error& e) {
        st = e.st;
        msg = e.msg;
    }
    (void)hipFree(dA);
    (void)hipFree(dLi);
    (void)hipFree(dR);
    (void)hipFree(dinfo);
    if (st != GPRX_OK) throw Error{st, msg};
    return GPRX_OK;
}

gprx_status gprx_dev_forward_panel_impl(gprx_dtype dtype, const void* L, int64_t n, void* R, int32_t rows,
                                        int32_t use_gemm, Exec* ex, hipStream_t s) {
    return by_dtype(dtype, [&](auto t) { return forward_panel_impl<decltype(t)>(L, n, R, rows, use_gemm, *ex, s); });
}

// gprx_dev_factor_update: the rotation kernel (k_remove.hip) alone on a host factor: every block
// from 0 on, nothing shifted.  Lout is the new lower factor (row-major, zeros above the diagonal),
// LinvOut the inverse of each of its diagonal blocks (n x 128, row-major: block b in rows
// [128 b, 128 b + 128)).  The output buffers start from a fixed bit pattern, so what the kernel
// does not write shows.
template <typename T>
static gprx_status factor_update_impl(const void* Lh, int64_t n, const void* Xh, int r, void* Lout, void* LinvOut,
                                      Exec& ex, hipStream_t s) {
    GPRX_REQUIRE(Lh && Xh && Lout && LinvOut && n > 0 && n % DB == 0 && r >= 1, GPRX_ERR_ARG,
                 "gprx_dev_factor_update: n must be a positive multiple of 128 and r >= 1");
    const T* L = static_cast<const T*>(Lh);
    const T* X = static_cast<const T*>(Xh);
    const int nb = (int)(n / DB);
    T guard;
    std::memset(&guard, 0x5a, sizeof(T));
    std::vector<T> hA((size_t)n * n, guard), hX((size_t)n * r), hO((size_t)n * n, guard), hLi((size_t)n * DB, guard);
    for (int64_t i = 0; i < n; i++) {
        for (int64_t j = 0; j <= i; j++) hA[(size_t)i + (size_t)j * n] = L[(size_t)i * n + j];
        for (int64_t v = 0; v < r; v++) hX[(size_t)i + (size_t)v * n] = X[(size_t)i * r + v];
    }
    T *dA = nullptr, *dX = nullptr, *dO = nullptr, *dLi = nullptr, *dW = nullptr;
    int* dinfo = nullptr;
    gprx_status st = GPRX_OK;
    std::string msg;
    try {
        GPRX_HIP(dev_malloc(&dA, sizeof(T) * hA.size()));
        GPRX_HIP(dev_malloc(&dX, sizeof(T) * hX.size()));
        GPRX_HIP(dev_malloc(&dO, sizeof(T) * hO.size()));
        GPRX_HIP(dev_malloc(&dLi, sizeof(T) * hLi.size()));
        GPRX_HIP(dev_malloc(&dW, sizeof(T) * factor_update_ws_elems(nb, r)));
        GPRX_HIP(dev_malloc(&dinfo, sizeof(int)));
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipMemcpy(dA, hA.data(), sizeof(T) * hA.size(), hipMemcpyHostToDevice));
        GPRX_HIP(hipMemcpy(dX, hX.data(), sizeof(T) * hX.size(), hipMemcpyHostToDevice));
        GPRX_HIP(hipMemcpy(dO, hO.data(), sizeof(T) * hO.size(), hipMemcpyHostToDevice));
        GPRX_HIP(hipMemcpy(dLi, hLi.data(), sizeof(T) * hLi.size(), hipMemcpyHostToDevice));
        const int big = INT_MAX;
        GPRX_HIP(hipMemcpy(dinfo, &big, sizeof(int), hipMemcpyHostToDevice));
        launch_factor_update<T>(dA, n, dO, n, dLi, dX, n, r, 0, 0, n, 0, nb, dW, dinfo, ex, s);
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipGetLastError());
        int hinfo = 0;
        GPRX_HIP(hipMemcpy(&hinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost));
        GPRX_HIP(hipMemcpy(hO.data(), dO, sizeof(T) * hO.size(), hipMemcpyDeviceToHost));
        GPRX_HIP(hipMemcpy(hLi.data(), dLi, sizeof(T) * hLi.size(), hipMemcpyDeviceToHost));
        GPRX_REQUIRE(hinfo >= 0, GPRX_ERR_HIP, "gprx_dev_factor_update: a chained wait timed out");
        T* Lo = static_cast<T*>(Lout);
        T* Lio = static_cast<T*>(LinvOut);
        for (int64_t i = 0; i < n; i++) {
            // (tiles above the diagonal are not the kernel's to write: zero in the row-major result)
            for (int64_t j = 0; j < n; j++) Lo[(size_t)i * n + j] = j / DB <= i / DB ? hO[(size_t)i + (size_t)j * n] : T(0);
            for (int64_t c = 0; c < DB; c++) Lio[(size_t)i * DB + c] = hLi[(size_t)(i / DB) * DB * DB + i % DB + (size_t)c * DB];
        }
    } catch (const Error& e) {
        st = e.st;
        msg = e.msg;
    }
    (void)hipFree(dA);
    (void)hipFree(dX);
    (void)hipFree(dO);
    (void)hipFree(dLi);
    (void)hipFree(dW);
    (void)hipFree(dinfo);
    if (st != GPRX_OK) throw Error{st, msg};
    return GPRX_OK;
}

gprx_status gprx_dev_factor_update_impl(gprx_dtype dtype, const void* L, int64_t n, const void* X, int32_t r,
                                        void* Lout, void* LinvOut, Exec* ex, hipStream_t s) {
    return by_dtype(dtype, [&](auto t) { return factor_update_impl<decltype(t)>(L, n, X, r, Lout, LinvOut, *ex, s); });
}
}  // namespace gprx

extern "C" int64_t gprx_dev_panel_trace(int64_t* times, int64_t max_blocks) {
    try {
        return gprx::ap_trace_copy((long long*)times, max_blocks);
    } catch (const Error& e) {
        std::fprintf(stderr, "gprx_dev_panel_trace: %s\n", e.msg.c_str());
        return -1;
    }
}

namespace gprx {
int pt_debug_snapshot(int* out, int max_wg);
int64_t pt_trace_copy(int32_t* tasks, long long* times, int64_t max);
int64_t bs_trace_copy(long long* out, int64_t max_blocks);
}
extern "C" int64_t gprx_dev_bs_trace(int64_t* times, int64_t max_blocks) {
    try {
        return gprx::bs_trace_copy((long long*)times, max_blocks);
    } catch (const Error& e) {
        std::fprintf(stderr, "gprx_dev_bs_trace: %s\n", e.msg.c_str());
        return -1;
    }
}
extern "C" int64_t gprx_dev_pt_trace(int32_t* tasks, int64_t* times, int64_t max) {
    try {
        return gprx::pt_trace_copy(tasks, (long long*)times, max);
    } catch (const gprx::Error& e) {
        std::fprintf(stderr, "gprx_dev_pt_trace: %s\n", e.msg.c_str());
        return -1;
    }
}
extern "C" int32_t gprx_dev_pt_debug(int32_t* out, int32_t max_wg) { return gprx::pt_debug_snapshot(out, max_wg); }

extern "C" gprx_status gprx_dev_schedule(int32_t nc, int32_t nr, int32_t P, int32_t build, double* est_us,
                                         int64_t* ntasks) {
    try {
        // build: bit 0 = fused covariance build, bit 1 = the last nc row blocks are identity,
        // bits 8..15 = chunk rule ratio + 1 (0: the one the simulation picks), bits 16..23 =
        // paired updates' row offset + 1 (0: the simulation's choice, 1: none), bit 2 = the narrow
        // label row (row block nc, the only label block, leaves the pairs), bit 3 = the f32 schedule
        const int64_t n = potrf_tiles_schedule_stats(nc, nr, P, (build & 1) != 0, est_us, (build & 2) ? nc : 0,
                                                     ((build >> 8) & 0xff) - 1, nullptr, 0, ((build >> 16) & 0xff) - 1,
                                                     (build & 4) != 0, (build & 8) == 0);
        if (ntasks) *ntasks = n;
        return GPRX_OK;
    } catch (const Error& e) {
        std::fprintf(stderr, "gprx_dev_schedule: %s\n", e.msg.c_str());
        return e.st;
    }
}

extern "C" int64_t gprx_dev_schedule_list(int32_t nc, int32_t nr, int32_t P, int32_t build, int32_t* out,
                                          int64_t max) {
    try {
        return potrf_tiles_schedule_stats(nc, nr, P, (build & 1) != 0, nullptr, (build & 2) ? nc : 0,
                                          ((build >> 8) & 0xff) - 1, out, max, ((build >> 16) & 0xff) - 1,
                                          (build & 4) != 0, (build & 8) == 0);
    } catch (const Error& e) {
        std::fprintf(stderr, "gprx_dev_schedule_list: %s\n", e.msg.c_str());
        return -1;
    }
}

extern "C" int32_t gprx_dev_sparse_clear_plan(int64_t* state, int64_t id, int64_t ld, int64_t cols, int64_t Mp,
                                              int64_t M, int64_t nc, int64_t* rects) {
    if (!state || !rects || M <= 0 || M > Mp || Mp > ld || nc < 0 || nc > cols) return -1;
    gprx::SparseBlock st;
    st.id = state[0], st.ld = state[1], st.cols = state[2], st.Mp = state[3], st.zero = state[4], st.rows = state[5];
    gprx::ClearRect r[gprx::SPARSE_CLEAR_MAX];
    const int k = gprx::sparse_clear_plan(st, id, ld, cols, Mp, M, nc, r);
    for (int q = 0; q < k; q++) {
        rects[4 * q] = r[q].row0, rects[4 * q + 1] = r[q].nrows;
        rects[4 * q + 2] = r[q].col0, rects[4 * q + 3] = r[q].ncols;
    }
    state[0] = st.id, state[1] = st.ld, state[2] = st.cols, state[3] = st.Mp, state[4] = st.zero, state[5] = st.rows;
    return k;
}

namespace gprx {
gprx_status gprx_dev_bench_impl(gprx_dtype dtype, int32_t what, int64_t M, int64_t N, int64_t K, int32_t iters,
                                double* ms, Exec* ex) {
    return by_dtype(dtype, [&](auto t) { return bench_impl<decltype(t)>(what, M, N, K, iters, ms, *ex); });
}
}  // namespace gprx

extern "C" gprx_status gprx_dev_fexp(gprx_ctx* ctx, const double* x, int64_t n, double* y) {
    (void)ctx;
    if (n <= 0) return GPRX_OK;
    double *dx = nullptr, *dy = nullptr;
    if (dev_malloc(&dx, sizeof(double) * n) != hipSuccess || dev_malloc(&dy, sizeof(double) * n) != hipSuccess)
        return GPRX_ERR_OOM;
    (void)hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(dev_fexp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, n, dy);
    const hipError_t e = hipMemcpy(y, dy, sizeof(double) * n, hipMemcpyDeviceToHost);
    (void)hipFree(dx);
    (void)hipFree(dy);
    return e == hipSuccess ? GPRX_OK : GPRX_ERR_HIP;
}

extern "C" gprx_status gprx_dev_diag_factor(gprx_ctx* ctx, int32_t variant, const double* A, double* L, double* Linv,
                                            int32_t* info_out) {
    (void)ctx;
    if (variant < 0 || variant > 2 || !A || !L || !Linv || !info_out) return GPRX_ERR_ARG;
    double *dA = nullptr, *dLi = nullptr;
    int* di = nullptr;
    long long* pr = nullptr;
    const size_t b = sizeof(double) * DB * DB;
    gprx_status st = GPRX_OK;
    if (dev_malloc(&dA, b) != hipSuccess || dev_malloc(&dLi, b) != hipSuccess || dev_malloc(&di, sizeof(int)) != hipSuccess ||
        dev_malloc(&pr, sizeof(long long) * 8) != hipSuccess) {
        st = GPRX_ERR_OOM;
    } else {
        const int big = 0x7fffffff;
        (void)hipMemcpy(dA, A, b, hipMemcpyHostToDevice);
        (void)hipMemcpy(di, &big, sizeof(int), hipMemcpyHostToDevice);
        pt::launch_diag_bench<double>(variant, dA, DB, dLi, di, pr, 1, 0);
        if (hipMemcpy(L, dA, b, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(Linv, dLi, b, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(info_out, di, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
            st = GPRX_ERR_HIP;
    }
    (void)hipFree(dA);
    (void)hipFree(dLi);
    (void)hipFree(di);
    (void)hipFree(pr);
    return st;
}

extern "C" gprx_status gprx_dev_dist_schedule(int32_t nc, int32_t P, int32_t g, int32_t gb, int32_t ww, int32_t flags,
                                              double* est_us, int32_t* chunk_w, int64_t* ntasks) {
    if (nc < 1 || P < 1 || g < 1 || g > 32 || gb < 1 || ww < 1 || !est_us) return GPRX_ERR_ARG;
    try {
        // flags bits 8..15: the update-chunk rule's ratio + 1 (0: the fixed rule), bit 3: the f32 schedule
        const DistSched S = potrf_dist_schedule(nc, g, gb, ww, P, (flags & 1) != 0, (flags & 2) != 0,
                                                std::max(0, ((flags >> 8) & 0xff) - 1), (flags & 8) == 0);
        *est_us = S.est_us;
        if (chunk_w) *chunk_w = S.W;
        if (ntasks) {
            int64_t t = 0;
            for (const auto& l : S.lists) t += (int64_t)l.size();
            *ntasks = t;
        }
    } catch (...) {
        return GPRX_ERR_ARG;
    }
    return GPRX_OK;
}

extern "C" int64_t gprx_dev_dist_schedule_list(int32_t nc, int32_t P, int32_t g, int32_t gb, int32_t ww, int32_t flags,
                                               int32_t rank, int32_t* out, int64_t max) {
    if (nc < 1 || P < 1 || g < 1 || g > 32 || gb < 1 || ww < 1 || rank < 0 || rank >= g) return -1;
    try {
        const DistSched S = potrf_dist_schedule(nc, g, gb, ww, P, (flags & 1) != 0, (flags & 2) != 0,
                                                std::max(0, ((flags >> 8) & 0xff) - 1), (flags & 8) == 0);
        const std::vector<int4>& l = S.lists[rank];
        if (out)
            for (int64_t q = 0; q < (int64_t)l.size() && q < max; q++)
                out[4 * q] = l[q].x, out[4 * q + 1] = l[q].y, out[4 * q + 2] = l[q].z, out[4 * q + 3] = l[q].w;
        return (int64_t)l.size();
    } catch (...) {
        return -1;
    }
}
