// gprx_matrix.cpp — the standalone building blocks: kernel, derivative and cross matrices, the
// Cholesky factor and SPD inverse of a caller's matrix, the fit's covariance tiles alone.
#include "gprx_model.h"

namespace gprx {

template <typename T>
gprx_status kernel_matrix_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* X, int64_t n, int d,
                               void* Kout, bool deriv) {
    KCanon<T> K;
    std::string e = canonicalize<T>(*desc, K);
    GPRX_REQUIRE(e.empty(), GPRX_ERR_ARG, e);
    hipStream_t s = ctx->stream;
    Points<T> P;
    DevBuf dk, flag;
    stage_points<T>(P, K, X, n, d, ctx->device, s, false);
    if (deriv) {
        dk.ensure(sizeof(T) * K.nparams * n * n);
        launch_deriv_matrix<T>(K, P.x, P.tab, n, d, dk.as<T>(), s);
        download(Kout, dk.p, sizeof(T) * K.nparams * n * n, s);
        return GPRX_OK;
    }
    dk.ensure(sizeof(T) * n * n);
    flag.ensure(sizeof(int));
    GPRX_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    launch_kbuild<T>(K, P.x, P.tab, n, P.x, P.tab, n, d, dk.as<T>(), n, n, true, T(0), flag.as<int>(), s);
    std::vector<T> h((size_t)n * n);
    download(h.data(), dk.p, sizeof(T) * n * n, s);
    int hf = 0;
    download(&hf, flag.p, sizeof(int), s);
    mirror_lower<T>(h.data(), n, n, reinterpret_cast<T*>(Kout));
    check_finite(hf);
    return GPRX_OK;
}

template <typename T>
gprx_status cross_matrix_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* A, int64_t na,
                              const void* B, int64_t nb, int d, void* Kout) {
    KCanon<T> K;
    std::string e = canonicalize<T>(*desc, K);
    GPRX_REQUIRE(e.empty(), GPRX_ERR_ARG, e);
    hipStream_t s = ctx->stream;
    Points<T> Pa, Pb;
    DevBuf dk, flag;
    stage_points<T>(Pa, K, A, na, d, ctx->device, s, false);
    stage_points<T>(Pb, K, B, nb, d, ctx->device, s, false);
    dk.ensure(sizeof(T) * na * nb);
    flag.ensure(sizeof(int));
    GPRX_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    launch_kbuild<T>(K, Pa.x, Pa.tab, na, Pb.x, Pb.tab, nb, d, dk.as<T>(), na, 0, false, T(0), flag.as<int>(), s);
    std::vector<T> h((size_t)na * nb);
    download(h.data(), dk.p, sizeof(T) * na * nb, s);
    T* out = reinterpret_cast<T*>(Kout);
    for (int64_t j = 0; j < nb; j++)
        for (int64_t i = 0; i < na; i++) out[(size_t)i * nb + j] = h[(size_t)j * na + i];
    return GPRX_OK;
}

template <typename T>
gprx_status cholesky_impl(gprx_ctx* ctx, void* Ahost, int64_t n, int32_t* info, bool inverse) {
    hipStream_t s = ctx->stream;
    const int64_t np = round_up(n, DB);
    DevBuf dA, dLinv, dinfo, dV, dC;
    dA.ensure(sizeof(T) * np * np);
    dLinv.ensure(sizeof(T) * np * DB);
    dinfo.ensure(sizeof(int));
    GPRX_HIP(hipMemsetAsync(dA.p, 0, sizeof(T) * np * np, s));
    GPRX_HIP(hipStreamSynchronize(s));
    // row i of the (symmetric) host matrix = column i of the column-major device matrix
    GPRX_HIP(hipMemcpy2D(dA.p, sizeof(T) * np, Ahost, sizeof(T) * n, sizeof(T) * n, n, hipMemcpyHostToDevice));
    launch_set_identity_pad<T>(dA.as<T>(), np, n, np, s);
    GPRX_HIP(hipMemsetD32Async((hipDeviceptr_t)dinfo.p, INT_MAX, 1, s));
    potrf_tiles<T>(dA.as<T>(), np, np, np, dLinv.as<T>(), dinfo.as<int>(), ctx->ex);
    int hinfo = 0;
    download(&hinfo, dinfo.p, sizeof(int), s);
    check_sched(hinfo);
    hinfo = (hinfo == INT_MAX) ? 0 : hinfo;
    if (info) *info = hinfo;
    std::vector<T> h((size_t)n * n);
    T* out = reinterpret_cast<T*>(Ahost);
    if (!inverse) {
        GPRX_HIP(hipMemcpy2D(h.data(), sizeof(T) * n, dA.p, sizeof(T) * np, sizeof(T) * n, n, hipMemcpyDeviceToHost));
        // h[j*n + i] = L(i, j) for i >= j
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = 0; j < n; j++) out[(size_t)i * n + j] = (i >= j) ? h[(size_t)j * n + i] : T(0);
        return hinfo ? GPRX_ERR_NOT_SPD : GPRX_OK;
    }
    if (hinfo) return fail(ctx, GPRX_ERR_NOT_SPD, "gprx_spd_inverse: matrix is not positive definite");
    dV.ensure(sizeof(T) * np * np);
    dC.ensure(sizeof(T) * np * np);
    launch_spd_inverse_from_factor<T>(dA.as<T>(), np, np, dLinv.as<T>(), dV.as<T>(), dC.as<T>(), s);
    GPRX_HIP(hipStreamSynchronize(s));
    GPRX_HIP(hipGetLastError());
    GPRX_HIP(hipMemcpy2D(h.data(), sizeof(T) * n, dC.p, sizeof(T) * np, sizeof(T) * n, n, hipMemcpyDeviceToHost));
    mirror_lower<T>(h.data(), n, n, out);
    return GPRX_OK;
}

// gprx_dev_build_matrix: the fit's covariance tiles, written alone (include/gprx_dev.h)
template <typename T>
gprx_status dev_build_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* X, int64_t n, int d,
                           double sigma, int path, void* Kout, int iters, double* ms) {
    KCanon<T> K;
    std::string e = canonicalize<T>(*desc, K);
    GPRX_REQUIRE(e.empty(), GPRX_ERR_ARG, e);
    GPRX_REQUIRE(n > 0 && d > 0, GPRX_ERR_DIM, "gprx_dev_build_matrix: bad dimensions");
    GPRX_REQUIRE(pairs_mma_supported<T>(K, 1), GPRX_ERR_ARG,
                 "gprx_dev_build_matrix: the tree takes the direct (VALU) build, see gprx_kernel_matrix");
    hipStream_t s = ctx->stream;
    const int64_t np = round_up(n, GT), kf = pairs_feature_cols<T>(K, d);
    DevBuf dx, fu, fv, A, Li, info, flag;
    DevParam kd;
    upload<T>(dx, X, sizeof(T) * n * d, s);
    fu.ensure(sizeof(T) * np * kf);
    fv.ensure(sizeof(T) * np * kf);
    flag.ensure(sizeof(int));
    info.ensure(sizeof(int));
    A.ensure(sizeof(T) * np * np);
    Li.ensure(sizeof(T) * np * DB);
    GPRX_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    GPRX_HIP(hipMemsetAsync(A.p, 0, sizeof(T) * np * np, s));
    GPRX_HIP(hipMemsetD32Async((hipDeviceptr_t)info.p, INT_MAX, 1, s));
    launch_pair_features<T>(K, dx.as<T>(), n, d, dx.as<T>(), false, fu.as<T>(), np, s, flag.as<int>());
    launch_pair_features<T>(K, dx.as<T>(), n, d, dx.as<T>(), true, fv.as<T>(), np, s);
    const KCanon<T>* kdev = kd.put(K, s);
    const T sig = (T)sigma, sigma2 = sig * sig;
    TileBuild<T> tb{};
    if (path == 0) {
        tb = pairs_tile_build<T>(K, kdev, fu.as<T>(), fv.as<T>(), np, d, n, sigma2, flag.as<int>());
        GPRX_REQUIRE(tb.mode != 0, GPRX_ERR_ARG,
                     "gprx_dev_build_matrix: the fused build carries sum-of-exp-leaf trees only (path 1 for others)");
    }
    auto launch = [&] {
        if (path == 0)
            potrf_tiles<T>(A.as<T>(), np, np, np, Li.as<T>(), info.as<int>(), ctx->ex, &tb, 0, true);
        else
            launch_kbuild_mma<T>(K, kdev, fu.as<T>(), fv.as<T>(), np, d, A.as<T>(), np, n, sigma2,
                                 flag.as<int>(), s);
    };
    if (ms) {  // gprx_dev_build_time: device time of the build alone (features resident)
        launch();  // warm (schedule cached, code loaded)
        hipStream_t ls = path == 0 ? ctx->ex.s0 : s;
        GPRX_HIP(hipStreamSynchronize(s));
        hipEvent_t e0, e1;
        GPRX_HIP(hipEventCreate(&e0));
        GPRX_HIP(hipEventCreate(&e1));
        GPRX_HIP(hipEventRecord(e0, ls));
        for (int it = 0; it < iters; it++) launch();
        GPRX_HIP(hipEventRecord(e1, ls));
        GPRX_HIP(hipEventSynchronize(e1));
        float t = 0;
        GPRX_HIP(hipEventElapsedTime(&t, e0, e1));
        GPRX_HIP(hipEventDestroy(e0));
        GPRX_HIP(hipEventDestroy(e1));
        *ms = (double)t / std::max(1, iters);
        int hinfo = 0;
        download(&hinfo, info.p, sizeof(int), s);
        check_sched(hinfo);
        return GPRX_OK;
    }
    launch();
    std::vector<T> h((size_t)np * n);
    download(h.data(), A.p, sizeof(T) * np * n, s);
    int hf = 0, hinfo = 0;
    download(&hf, flag.p, sizeof(int), s);
    download(&hinfo, info.p, sizeof(int), s);
    check_sched(hinfo);
    mirror_lower<T>(h.data(), np, n, reinterpret_cast<T*>(Kout));
    check_finite(hf);
    return GPRX_OK;
}

#define GPRX_INST(T)                                                                                          \
    template gprx_status kernel_matrix_impl<T>(gprx_ctx*, const gprx_kernel_desc*, const void*, int64_t, int,  \
                                               void*, bool);                                                   \
    template gprx_status cross_matrix_impl<T>(gprx_ctx*, const gprx_kernel_desc*, const void*, int64_t,        \
                                              const void*, int64_t, int, void*);                               \
    template gprx_status cholesky_impl<T>(gprx_ctx*, void*, int64_t, int32_t*, bool);                          \
    template gprx_status dev_build_impl<T>(gprx_ctx*, const gprx_kernel_desc*, const void*, int64_t, int,      \
                                           double, int, void*, int, double*);
GPRX_INST(float)
GPRX_INST(double)
#undef GPRX_INST

}  // namespace gprx
