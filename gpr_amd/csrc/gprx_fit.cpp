// gprx_fit.cpp — what produces a model's factor: the dense fit, the sharded fit, the LU fallback,
// the fp64 refinement of fp32 fits, the explicit inverse, the append and the remove.
#include "gprx_model.h"

namespace gprx {

// device time of a fit's build, factorisation and solve (the context's events 0..3), added to out's
static void add_phase_times(gprx_ctx* ctx, gprx_fit_info* out) {
    float t[3] = {0, 0, 0};
    for (int i = 0; i < 3; i++) hipEventElapsedTime(&t[i], ctx->ev[i], ctx->ev[i + 1]);
    out->ms_build += t[0];
    out->ms_factor += t[1];
    out->ms_solve += t[2];
}

// A fit's status words: one kernel stores them into mapped pinned memory, then one synchronisation
struct FitStatus {
    int flag, info;
    double logdet, datafit;
};
static FitStatus read_fit_status(gprx_model* M, hipStream_t s) {
    M->hstat.ensure(4 * sizeof(double));
    volatile double* hs = static_cast<double*>(M->hstat.p);  // [0] flag, [1] info (ints), [2..3] log det, data fit
    launch_fit_status_gather(M->flag.as<int>(), M->info.as<int>(), M->red.as<double>(), M->hstat.dev, s);
    GPRX_HIP(hipStreamSynchronize(s));
    GPRX_HIP(hipGetLastError());
    return {reinterpret_cast<volatile int*>(hs)[0], reinterpret_cast<volatile int*>(hs + 1)[0], hs[2], hs[3]};
}

// the end of a refinement (begun at event 0): its device time, last relative correction and steps
static void refine_report(gprx_ctx* ctx, gprx_fit_info* out, double rel, int taken) {
    GPRX_HIP(hipEventRecord(ctx->ev[1], ctx->stream));
    GPRX_HIP(hipEventSynchronize(ctx->ev[1]));
    if (!out) return;
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
    out->ms_refine = ms;
    out->refine_delta = rel;
    out->refine_steps = taken;
}

// ---------------------------------------------------------------------------------------
// fp64 iterative refinement of an fp32 fit (k_refine.hip): alpha_d += (L L^T)^{-1}
// (Y - (K + s2 I) alpha_d) with K evaluated in fp64 (pair statistics of the fp64-widened
// samples, the predict path with the training set as the queries) and the correction solved
// with the fp32 factor already in A (forward solve of the residual written into the label
// rows, back substitution).  Stops when the correction is below fp32 resolution of alpha.
// ---------------------------------------------------------------------------------------
static void refine_f32(gprx_model* M, gprx_fit_info* out) {
    gprx_ctx* ctx = M->ctx;
    hipStream_t s = ctx->stream;
    const KCanon<double>& K = M->kd;
    const int64_t n = M->n, np = M->np, mp = M->mp, ld = M->ld;
    const int d = M->d, m = M->m;
    int steps = 3;
    if (const char* e = std::getenv("GPRX_REFINE_STEPS")) steps = std::max(0, std::atoi(e));
    GPRX_HIP(hipEventRecord(ctx->ev[0], s));
    M->Xd.ensure(sizeof(double) * n * d);
    M->Yd.ensure(sizeof(double) * n * m);
    M->ad.ensure(sizeof(double) * n * m);
    M->kxd.ensure(sizeof(double) * n * m);
    M->delta.ensure(sizeof(float) * np * m);
    M->nrm.ensure(2 * sizeof(unsigned long long));
    launch_convert<float, double>(M->X.as<float>(), M->Xd.as<double>(), n * d, s);
    launch_convert<float, double>(M->Y.as<float>(), M->Yd.as<double>(), n * m, s);
    launch_convert<float, double>(M->alpha.as<float>(), M->ad.as<double>(), n * m, s);
    const bool mma = pairs_mma_supported<double>(K, 1);
    const KCanon<double>* kdev = nullptr;
    if (mma) {
        const int64_t kf = pairs_feature_cols<double>(K, d);
        M->fud.ensure(sizeof(double) * np * kf);
        M->fvd.ensure(sizeof(double) * np * kf);
        launch_pair_features<double>(K, M->Xd.as<double>(), n, d, M->Xd.as<double>(), false, M->fud.as<double>(), np, s);
        launch_pair_features<double>(K, M->Xd.as<double>(), n, d, M->Xd.as<double>(), true, M->fvd.as<double>(), np, s);
        kdev = M->kfit64.put(K, s);
    } else {
        sincos_tables<double>(K, M->Xd.as<double>(), n, d, M->tabd, s);
        M->zd.ensure(sizeof(double) * n * m);
        M->outd.ensure(sizeof(double) * n * m);
    }
    const float sf = (float)M->sigma;
    const double s2 = (double)(sf * sf);  // m_Sigma * m_Sigma in T (lib/GaussianProcess.cpp:379)
    double rel = 0;
    int taken = 0;
    for (int it = 0; it < steps; it++) {
        if (mma) {
            for (int c = 0; c < m; c++)  // one label column per launch (alpha, Kx strided by m)
                launch_predict_mma<double>(K, kdev, M->fud.as<double>(), np, M->fvd.as<double>(), np, d,
                                           M->ad.as<double>() + c, n, m, n, M->kxd.as<double>() + c, s);
        } else {
            launch_predict<double>(K, M->Xd.as<double>(), M->tabd.as<double>(), n, d, m, M->ad.as<double>(),
                                   M->Xd.as<double>(), M->tabd.as<double>(), n, M->kxd.as<double>(), nullptr,
                                   M->zd.as<double>(), M->outd.as<double>(), s);
        }
        launch_residual_rows(M->Yd.as<double>(), M->kxd.as<double>(), M->ad.as<double>(), s2, n, m,
                             M->A.as<float>(), ld, np, np, (int)mp, s);
        GPRX_HIP(hipMemsetD32Async((hipDeviceptr_t)M->info.p, INT_MAX, 1, s));
        launch_forward_chain<float>(M->A.as<float>(), ld, np, m, M->Linv.as<float>(), M->info.as<int>(), ctx->ex, s);
        launch_backsolve_chain<float>(M->A.as<float>(), ld, np, m, M->Linv.as<float>(), M->delta.as<float>(),
                                      M->info.as<int>(), ctx->ex, s);
        launch_refine_accumulate(M->delta.as<float>(), M->ad.as<double>(), M->alpha.as<float>(), n * m,
                                 M->nrm.as<unsigned long long>(), s);
        unsigned long long h[2];
        int hinfo = 0;
        download(h, M->nrm.p, sizeof(h), s);
        download(&hinfo, M->info.p, sizeof(int), s);
        check_sched(hinfo);
        double dn, an;
        std::memcpy(&dn, &h[0], sizeof(double));
        std::memcpy(&an, &h[1], sizeof(double));
        rel = an > 0 ? dn / an : dn;
        taken = it + 1;
        if (!(rel > 0x1p-26)) break;  // below fp32 resolution of alpha (NaN: stop too)
    }
    refine_report(ctx, out, rel, taken);
}

// ---------------------------------------------------------------------------------------
// LU fallback (k_getrf.hip): K + sigma^2 I rebuilt in full, factored with partial pivoting in
// double, alpha = A^{-1} Y by the two triangular solves.  The reference's default inversion
// is exactly this LU (dgetrf_ on the matrix cast to double, include/LAPACKUtils.h:38-56,
// 85-97); it reaches here only when the Cholesky met a non-positive pivot.
// ---------------------------------------------------------------------------------------
template <typename T>
static void lu_build_matrix(gprx_model* M) {
    hipStream_t s = M->ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int64_t n = M->n, np = M->np;
    const T sig = (T)M->sigma;
    const T sigma2 = sig * sig;  // in T, as the reference (lib/GaussianProcess.cpp:379)
    M->lu.ensure(sizeof(double) * np * np);
    GPRX_HIP(hipMemsetAsync(M->flag.p, 0, sizeof(int), s));
    // K evaluated in T (the reference's): straight into lu for double; for float into A, then widened
    // as lu_invert<float> casts to double (LAPACKUtils.h:85-97)
    constexpr bool wide = std::is_same<T, double>::value;
    if (!wide) M->A.ensure(sizeof(T) * np * np);
    T* dst = wide ? M->lu.as<T>() : M->A.as<T>();
    if (M->host_k)  // the caller's K
        launch_kext_build<T>(M->Kext.as<T>(), n, dst, np, np, sigma2, M->flag.as<int>(), s);
    else
        launch_kbuild<T>(K, M->X.as<T>(), M->tab.as<T>(), n, M->X.as<T>(), M->tab.as<T>(), n, M->d, dst, np, np, true,
                         sigma2, M->flag.as<int>(), s);
    if constexpr (!wide) launch_convert<T, double>(dst, M->lu.as<double>(), np * np, s);
    if (!M->host_k) launch_sym_fill<double>(M->lu.as<double>(), np, np, s);
}

template <typename T>
static void lu_fit(gprx_model* M, gprx_fit_info* out) {
    gprx_ctx* ctx = M->ctx;
    hipStream_t s = ctx->stream;
    const int64_t n = M->n, np = M->np;
    const int m = M->m;
    GPRX_HIP(hipEventRecord(ctx->ev[0], s));
    lu_build_matrix<T>(M);
    M->ipiv.ensure(sizeof(int) * np);
    M->luUt.ensure(sizeof(double) * np * DB);
    M->luB.ensure(sizeof(double) * np * m);
    M->lured.ensure(sizeof(double) * 4);
    GPRX_HIP(hipMemsetD32Async((hipDeviceptr_t)M->info.p, INT_MAX, 1, s));
    GPRX_HIP(hipEventRecord(ctx->ev[1], s));
    lu_factor(M->lu.as<double>(), np, np, M->ipiv.as<int>(), M->info.as<int>(), M->luUt.as<double>(), s);
    GPRX_HIP(hipEventRecord(ctx->ev[2], s));
    lu_rhs_from_rows<T>(M->Y.as<T>(), n, m, M->luB.as<double>(), np, np, s);
    lu_solve(M->lu.as<double>(), np, np, M->ipiv.as<int>(), M->luB.as<double>(), np, m, s);
    M->alpha.ensure(sizeof(T) * np * m);
    lu_rows_from_rhs<T>(M->luB.as<double>(), np, n, m, M->alpha.as<T>(), s);
    lu_logdet(M->lu.as<double>(), np, n, M->ipiv.as<int>(), M->lured.as<double>(), s);
    GPRX_HIP(hipEventRecord(ctx->ev[3], s));
    int hflag = 0, hinfo = 0;
    double red[3];
    download(&hflag, M->flag.p, sizeof(int), s);
    download(&hinfo, M->info.p, sizeof(int), s);
    download(red, M->lured.p, sizeof(red), s);
    check_finite(hflag);
    if (hinfo != INT_MAX)
        throw Error{GPRX_ERR_SINGULAR, "gprx: kernel matrix is singular (LU pivot " + std::to_string(hinfo) +
                                           " is zero; the reference's dgetrf_ fails there too)"};
    // data fit y^T (K + s^2 I)^{-1} y from alpha (the host copies are small next to the factor)
    std::vector<T> ha((size_t)n * m), hy((size_t)n * m);
    download(ha.data(), M->alpha.p, sizeof(T) * n * m, s);
    download(hy.data(), M->Y.p, sizeof(T) * n * m, s);
    double df = 0;
    for (size_t e = 0; e < ha.size(); e++) df += (double)hy[e] * (double)ha[e];
    M->lu_sign = red[1];
    M->fit_done(1, false);
    if (out) {
        add_phase_times(ctx, out);
        out->logdet = red[0];  // log |det|; the sign is the model's lu_sign
        out->datafit = df;
        out->method = 1;
    }
}

// A^{-1} B for m right-hand sides already in M->luB-shaped column-major storage (np x m)
void lu_solve_model(gprx_model* M, double* B, int m) {
    lu_solve(M->lu.as<double>(), M->np, M->np, M->ipiv.as<int>(), B, M->np, m, M->ctx->stream);
}

// ---------------------------------------------------------------------------------------
// distributed fit (gprx_dist.cpp): row blocks dealt over the ranks, one persistent tile
// launch per rank, RCCL broadcast of each diagonal inverse and full-mesh panel exchange
// ---------------------------------------------------------------------------------------
// The LU in double on this process's full copy of the samples (np x np workspace): the
// GPRX_FIT_FORCE_LU path, and the NOT_SPD fallback of a distributed fit, where every rank
// computes the same factor from its replicated X, Y.
template <typename T>
static void lu_fit_replicated(gprx_model* M, gprx_fit_info* out) {
    const int64_t np0 = round_up(M->n, (int64_t)DB);
    M->np = np0;
    M->mp = round_up(M->m, GT);
    M->ld = np0;
    M->drop_fit();
    M->drop_dist();
    M->info.ensure(sizeof(int));
    M->flag.ensure(sizeof(int));
    M->alpha.ensure(sizeof(T) * np0 * M->m);
    if (!M->host_k) ensure_train_tables<T>(M);
    if (out) std::memset(out, 0, sizeof(*out));
    lu_fit<T>(M, out);
}

// The dense factor of a distributed fit on this process, for the calls that need the whole
// factor (the core matrix -- the reference returns all of C -- and the VALU gradient's C; the
// posterior covariance solves across the ranks instead, model_posterior_cov_dist): gathered once per
// fit from every rank's packed rows (device reads through the mappings of the mailboxes'
// storage) into A (ld np) and Linv.  The one place a sharded fit holds N^2 on a process.
template <typename T>
void ensure_dense_factor(gprx_model* M) {
    if (!M->dist_fitted || M->dist_dense) return;
    const int64_t np = M->np;
    M->ld = np;
    M->A.ensure(sizeof(T) * np * np);
    M->Linv.ensure(sizeof(T) * np * DB);
    dist_gather_factor<T>(M->dist_engine, M->A.as<T>(), np, M->Linv.as<T>(), M->ctx->stream);
    M->dense_gathered();
}

// fp64 iterative refinement of a SHARDED fp32 fit (the single-GPU refine_f32 restated over the
// ranks): each process evaluates the fp64 residual r = Y - (K + s2 I) alpha_d only at the rows
// its ranks own (pair statistics of those rows against all n samples), the correction
// (L L^T)^{-1} r runs as the sharded forward + back substitutions (k_dsolve.hip) and arrives on
// every rank, alpha_d += delta everywhere (identical: no reduction needed).
static void refine_f32_dist(gprx_model* M, gprx_fit_info* out) {
    gprx_ctx* ctx = M->ctx;
    hipStream_t s = ctx->stream;
    const KCanon<double>& K = M->kd;
    const int64_t n = M->n, np = M->np;
    const int d = M->d, m = M->m;
    int steps = 3;
    if (const char* e = std::getenv("GPRX_REFINE_STEPS")) steps = std::max(0, std::atoi(e));
    GPRX_HIP(hipEventRecord(ctx->ev[0], s));
    // the rows this process's ranks own
    std::vector<int64_t> idx;
    for (int b : dist_own_blocks(M->dist_engine))
        for (int64_t r = (int64_t)b * DB; r < std::min<int64_t>(n, (int64_t)(b + 1) * DB); r++) idx.push_back(r);
    const int64_t q = (int64_t)idx.size(), qp = round_up(std::max<int64_t>(q, 1), GT);
    DevBuf didx, Xo, fuo, kxo, rhs;
    didx.ensure(sizeof(int64_t) * std::max<int64_t>(q, 1));
    GPRX_HIP(hipStreamSynchronize(s));
    if (q) GPRX_HIP(hipMemcpy(didx.p, idx.data(), sizeof(int64_t) * q, hipMemcpyHostToDevice));
    M->Xd.ensure(sizeof(double) * n * d);
    M->Yd.ensure(sizeof(double) * n * m);
    M->ad.ensure(sizeof(double) * n * m);
    M->delta.ensure(sizeof(float) * np * m);
    M->nrm.ensure(2 * sizeof(unsigned long long));
    kxo.ensure(sizeof(double) * qp * m);
    rhs.ensure(sizeof(float) * np * m);
    launch_convert<float, double>(M->X.as<float>(), M->Xd.as<double>(), n * d, s);
    launch_convert<float, double>(M->Y.as<float>(), M->Yd.as<double>(), n * m, s);
    launch_convert<float, double>(M->alpha.as<float>(), M->ad.as<double>(), n * m, s);
    Xo.ensure(sizeof(double) * std::max<int64_t>(q, 1) * d);
    launch_gather_rows(M->Xd.as<double>(), didx.as<int64_t>(), q, d, Xo.as<double>(), s);
    const bool mma = pairs_mma_supported<double>(K, 1);
    const KCanon<double>* kdev = nullptr;
    if (mma) {
        const int64_t kf = pairs_feature_cols<double>(K, d);
        fuo.ensure(sizeof(double) * qp * kf);
        M->fvd.ensure(sizeof(double) * np * kf);
        launch_pair_features<double>(K, Xo.as<double>(), q, d, M->Xd.as<double>(), false, fuo.as<double>(), qp, s);
        launch_pair_features<double>(K, M->Xd.as<double>(), n, d, M->Xd.as<double>(), true, M->fvd.as<double>(), np, s);
        kdev = M->kfit64.put(K, s);
    } else {
        if (K.nper > 0) {
            sincos_tables<double>(K, M->Xd.as<double>(), n, d, M->tabd, s);
            fuo.ensure(sizeof(double) * 2 * K.nper * std::max<int64_t>(q, 1) * d);  // (q may be 0)
            launch_sincos_tables<double>(K, Xo.as<double>(), q, d, fuo.as<double>(), s);
        }
        M->zd.ensure(sizeof(double) * n * m);
        M->outd.ensure(sizeof(double) * std::max<int64_t>(n, qp) * m);
    }
    const float sf = (float)M->sigma;
    const double s2 = (double)(sf * sf);  // m_Sigma * m_Sigma in T (lib/GaussianProcess.cpp:379)
    double rel = 0;
    int taken = 0;
    for (int it = 0; it < steps; it++) {
        if (mma) {
            for (int c = 0; c < m; c++)
                launch_predict_mma<double>(K, kdev, fuo.as<double>(), qp, M->fvd.as<double>(), np, d,
                                           M->ad.as<double>() + c, n, m, q, kxo.as<double>() + c, s);
        } else {
            launch_predict<double>(K, M->Xd.as<double>(), M->tabd.as<double>(), n, d, m, M->ad.as<double>(),
                                   Xo.as<double>(), fuo.as<double>(), q, kxo.as<double>(), nullptr, M->zd.as<double>(),
                                   M->outd.as<double>(), s);
        }
        GPRX_HIP(hipMemsetAsync(rhs.p, 0, sizeof(float) * np * m, s));
        launch_residual_scatter(M->Yd.as<double>(), kxo.as<double>(), M->ad.as<double>(), s2, didx.as<int64_t>(), q, m,
                                rhs.as<float>(), s);
        dist_solve<float>(M->dist_engine, rhs.as<float>(), M->delta.as<float>(), s);
        launch_refine_accumulate(M->delta.as<float>(), M->ad.as<double>(), M->alpha.as<float>(), n * m,
                                 M->nrm.as<unsigned long long>(), s);
        unsigned long long h[2];
        download(h, M->nrm.p, sizeof(h), s);
        double dn, an;
        std::memcpy(&dn, &h[0], sizeof(double));
        std::memcpy(&an, &h[1], sizeof(double));
        rel = an > 0 ? dn / an : dn;
        taken = it + 1;
        if (!(rel > 0x1p-26)) break;  // below fp32 resolution of alpha (NaN: stop too)
    }
    refine_report(ctx, out, rel, taken);
}

template <typename T>
static gprx_status model_fit_dist(gprx_model* M, uint32_t flags, gprx_fit_info* out) {
    gprx_ctx* ctx = M->ctx;
    GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE, "gprx: a caller-evaluated kernel matrix needs a single-GPU fit");
    hipStream_t s = ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int64_t n = M->n, np = round_up(n, DB);
    M->np = np;
    M->mp = GT;
    M->ld = 0;
    M->drop_fit();
    M->drop_dist();
    M->alpha.ensure(sizeof(T) * np * M->m);
    M->flag.ensure(sizeof(int));
    GPRX_HIP(hipMemsetAsync(M->flag.p, 0, sizeof(int), s));
    ensure_train_tables<T>(M);  // per-sample sin/cos tables: the direct predict path reads them
    const T sig = (T)M->sigma;
    const T sigma2 = sig * sig;  // m_Sigma*m_Sigma in T (lib/GaussianProcess.cpp:379)
    TileBuild<T> tb;
    std::memset(&tb, 0, sizeof(tb));
    if (pairs_mma_supported<T>(K, 1)) {  // the fused MFMA build: features of all n samples on every rank
        const int64_t kf = pairs_feature_cols<T>(K, M->d);
        M->featU.ensure(sizeof(T) * np * kf);
        launch_pair_features<T>(K, M->X.as<T>(), n, M->d, M->X.as<T>(), false, M->featU.as<T>(), np, s,
                                M->flag.as<int>());
        train_features<T>(M, true, np);
        tb = pairs_tile_build<T>(K, M->kfit.put(K, s), M->featU.as<T>(), M->featV.as<T>(), np, M->d, n, sigma2,
                                 M->flag.as<int>());
    }
    GPRX_HIP(hipStreamSynchronize(s));  // the ranks' streams read the features
    int hflag = 0;
    GPRX_HIP(hipMemcpy(&hflag, M->flag.p, sizeof(int), hipMemcpyDeviceToHost));
    DistContext C;
    C.device = ctx->device;
    C.rank = ctx->rank;
    C.world = ctx->world;
    C.virt = ctx->virt;
    C.hc = ctx->hc;
    C.cu_slot = ctx->cu_slot;
    C.cu_slots = ctx->cu_slots;
    // LML mode: the inverse rides along in the sharded launch (identity rows + C tiles) when the
    // gradient pass can read C tile by tile; other trees take a dense C on every process
    const bool inv_tiles = M->want_inv && pairs_grad_supported<T>(K);
    DistFitIn<T> in{K, M->X.as<T>(), M->Y.as<T>(), n, M->d, M->m, sigma2, tb, inv_tiles};
    DistFitOut o;
    dist_fit<T>(M->dist_engine, C, in, o, M->alpha.as<T>());
    M->dist_stats = o;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->logdet = o.logdet;
        out->datafit = o.datafit;
        out->info = (o.info == INT_MAX || o.info < 0) ? 0 : o.info;
        out->ms_factor = o.ms_kernel;  // device time of this process's persistent launch(es)
        out->ms_solve = o.ms_solve;
        out->refine_delta = 0;
    }
    check_finite(hflag || o.flag);
    check_sched(o.info);
    if (o.info != INT_MAX) {
        // the reference's default inversion is an LU (lib/GaussianProcess.cpp:545-559) and it
        // never rejects an indefinite K: every rank refactors the same K + s^2 I with the
        // partial-pivot LU in double (X and Y are replicated, the LU is deterministic, so the
        // ranks agree bit for bit).  Replicated, like the reference's own serial getrf: an
        // indefinite K is the exception path, not the sharded fit's workload.
        if (flags & GPRX_FIT_NO_LU_FALLBACK)
            throw Error{GPRX_ERR_NOT_SPD, "gprx: kernel matrix is not positive definite (Cholesky pivot " +
                                              std::to_string(o.info) + " <= 0)"};
        lu_fit_replicated<T>(M, out);
        if (out) out->info = o.info;  // the Cholesky's failing pivot, as on one GPU
        return GPRX_OK;
    }
    M->dist_fit_done(inv_tiles);
    if (M->want_inv) {
        if (!inv_tiles) {
            // a tree off the MFMA gradient path: its VALU gradient reads a dense C, formed on
            // every process from the gathered factor (documented N^2 per process)
            ensure_dense_factor<T>(M);
            model_inverse<T>(M);
        }
        M->inverse_done();
    }
    if constexpr (std::is_same<T, float>::value) {
        // the reference inverts fp32 GPs in double (include/LAPACKUtils.h:85-97): fp64
        // refinement of alpha against the sharded fp32 factor, as on one GPU
        if (!(flags & GPRX_FIT_F32_NO_REFINE) && !M->want_inv) refine_f32_dist(M, out);
    }
    return GPRX_OK;
}



// ---------------------------------------------------------------------------------------
// fit
// ---------------------------------------------------------------------------------------
template <typename T>
gprx_status model_fit(gprx_model* M, uint32_t flags, gprx_fit_info* out) {
    gprx_ctx* ctx = M->ctx;
    GPRX_REQUIRE(M->has_data, GPRX_ERR_STATE, "GaussianProcess::Initialize: no input samples defined during initialization");
    GPRX_REQUIRE(M->has_kernel, GPRX_ERR_STATE, "gprx: no kernel set");
    GPRX_HIP(hipSetDevice(ctx->device));
    M->trim_posterior_workspace();
    M->drop_sparse_cov();  // a dense fit's posterior covariance comes from its own factor, not a sparse GP's W
    hipStream_t s = ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    // multi-GPU factorisation: an RCCL context with world > 1, a virtual-rank context, or
    // GPRX_FIT_DISTRIBUTED (the same code path on a one-rank communicator)
    GPRX_REQUIRE(!(flags & GPRX_FIT_DISTRIBUTED) || ctx->hc || ctx->virt, GPRX_ERR_STATE,
                 "gprx_model_fit: GPRX_FIT_DISTRIBUTED needs a context from gprx_ctx_create_dist / _peer");
    // the SVD inversion methods' stand-in: the LU in double directly.  On a distributed
    // context every rank runs it on its replicated X, Y (as the NOT_SPD fallback below)
    M->lu_forced = (flags & GPRX_FIT_FORCE_LU) != 0;
    if (flags & GPRX_FIT_FORCE_LU) {
        lu_fit_replicated<T>(M, out);
        return GPRX_OK;
    }
    if ((ctx->hc && ctx->world > 1) || ctx->virt || (flags & GPRX_FIT_DISTRIBUTED))
        return model_fit_dist<T>(M, flags, out);
    M->start_dense_fit();
    const int64_t n = M->n, np = round_up(n, (int64_t)DB), mp = round_up(M->m, GT);
    // the explicit inverse rides along in the tile factorisation as np identity rows
    const bool want_inv = M->want_inv;
    const int64_t ld = np + mp + (want_inv ? np : 0);
    M->np = np;
    M->mp = mp;
    M->ld = ld;
    M->A.ensure(sizeof(T) * ld * np);
    M->Linv.ensure(sizeof(T) * np * DB);
    M->z.ensure(sizeof(T) * M->m * np);
    M->alpha.ensure(sizeof(T) * np * M->m);
    M->info.ensure(sizeof(int));
    M->flag.ensure(sizeof(int));
    M->red.ensure(sizeof(double) * (2 + 2 * (np / GT + 1)));  // results, then per-block partials
    ensure_train_tables<T>(M);  // per-sample sin/cos tables: the direct build, predict, posterior and LML paths
    launch_fit_status_init(M->info.as<int>(), M->flag.as<int>(), s);
    const T sig = (T)M->sigma;
    const T sigma2 = sig * sig;  // m_Sigma*m_Sigma in T (lib/GaussianProcess.cpp:379)
    GPRX_HIP(hipEventRecord(ctx->ev[0], s));
    TileBuild<T> tb;
    std::memset(&tb, 0, sizeof(tb));
    if (M->host_k) {  // the caller's K (k_hostk.hip)
        launch_kext_build<T>(M->Kext.as<T>(), n, M->A.as<T>(), ld, np, sigma2, M->flag.as<int>(), s);
    } else if (env_kbuild() != KBUILD_DIRECT && pairs_mma_supported<T>(K, 1)) {
        // pair statistics on the MFMA units from per-sample features (k_pairs.hip)
        const int64_t kf = pairs_feature_cols<T>(K, M->d);
        M->featU.ensure(sizeof(T) * np * kf);
        M->featV.ensure(sizeof(T) * np * kf);
        launch_pair_features<T>(K, M->X.as<T>(), n, M->d, M->X.as<T>(), false, M->featU.as<T>(), np, s,
                                M->flag.as<int>());
        train_features<T>(M, true, np);
        const KCanon<T>* kdev = M->kfit.put(K, s);
        if (env_kbuild() != KBUILD_SEPARATE)
            tb = pairs_tile_build<T>(K, kdev, M->featU.as<T>(), M->featV.as<T>(), np, M->d, n, sigma2,
                                     M->flag.as<int>());
        if (!tb.mode)
            launch_kbuild_mma<T>(K, kdev, M->featU.as<T>(), M->featV.as<T>(), np, M->d, M->A.as<T>(),
                                 ld, n, sigma2, M->flag.as<int>(), s);
    } else {
        launch_kbuild<T>(K, M->X.as<T>(), M->tab.as<T>(), n, M->X.as<T>(), M->tab.as<T>(), n, M->d, M->A.as<T>(), ld,
                         np, true, sigma2, M->flag.as<int>(), s);
    }
    launch_aug_rows<T>(M->Y.as<T>(), n, M->m, M->A.as<T>(), ld, np, mp, s);
    GPRX_HIP(hipEventRecord(ctx->ev[1], s));
    if (tb.mode || want_inv) {
        // (the label block's live rows: with m <= 16 its updates skip the zero padding)
        potrf_tiles<T>(M->A.as<T>(), ld, np, ld, M->Linv.as<T>(), M->info.as<int>(), ctx->ex, tb.mode ? &tb : nullptr,
                       want_inv ? (int)(np / GT) : 0, false, mp == GT ? M->m : GT);
    } else {
        potrf_tiles<T>(M->A.as<T>(), ld, np, ld, M->Linv.as<T>(), M->info.as<int>(), ctx->ex);
    }
    GPRX_HIP(hipEventRecord(ctx->ev[2], s));
    launch_fit_reductions<T>(M->A.as<T>(), ld, n, np, M->m, M->red.as<double>(), s);
    launch_backsolve_chain<T>(M->A.as<T>(), ld, np, M->m, M->Linv.as<T>(), M->alpha.as<T>(), M->info.as<int>(), ctx->ex,
                              s);
    if (want_inv) {  // C = U U^T (lower), U = L^{-T} from the identity rows
        M->C.ensure(sizeof(T) * np * np);
        const T* U = M->A.as<T>() + np + mp;
        launch_gemm_nt_kskip<T>(M->C.as<T>(), np, U, ld, U, ld, np, np, np, s);
    }
    GPRX_HIP(hipEventRecord(ctx->ev[3], s));
    const FitStatus st = read_fit_status(M, s);
    const int hflag = st.flag, hinfo = st.info;
    M->drop_fit();
    if (out) {
        std::memset(out, 0, sizeof(*out));
        add_phase_times(ctx, out);
        out->logdet = st.logdet;
        out->datafit = st.datafit;
        out->info = (hinfo == INT_MAX) ? 0 : hinfo;
        out->method = 0;
    }
    check_finite(hflag);
    check_sched(hinfo);
    if (hinfo != INT_MAX) {
        // the reference's default inversion is an LU (lib/GaussianProcess.cpp:545-559): refactor
        // the same matrix with partial pivoting instead of rejecting it
        if (!(flags & GPRX_FIT_NO_LU_FALLBACK)) {
            lu_fit<T>(M, out);
            return GPRX_OK;
        }
        throw Error{GPRX_ERR_NOT_SPD, "gprx: kernel matrix is not positive definite (Cholesky pivot " +
                                          std::to_string(hinfo) + " <= 0)"};
    }
    M->fit_done(0, want_inv);
    if constexpr (std::is_same<T, float>::value) {
        // the reference inverts fp32 GPs in double (include/LAPACKUtils.h:85-97): refine alpha
        // in fp64 against the fp32 factor.  Not for the LML's fit (its value and gradient come
        // from the factor and its inverse).
        // (a caller-evaluated kernel has no fp64 form to refine against)
        if (!(flags & GPRX_FIT_F32_NO_REFINE) && !want_inv && !M->host_k) refine_f32(M, out);
    }
    return GPRX_OK;
}

// V = L^{-T} (upper), C = V V^T (lower, ld = np) from the stored factor
template <typename T>
void model_inverse(gprx_model* M) {
    hipStream_t s = M->ctx->stream;
    const int64_t np = M->np;
    M->V.ensure(sizeof(T) * np * np);
    M->C.ensure(sizeof(T) * np * np);
    launch_spd_inverse_from_factor<T>(M->A.as<T>(), M->ld, np, M->Linv.as<T>(), M->V.as<T>(), M->C.as<T>(), s);
}

// ---------------------------------------------------------------------------------------
// gprx_model_append: AddSample x k + Initialize (lib/GaussianProcess.cpp:36-51, 118-130) by
// extending the Cholesky factor instead of refitting.  With n0 the last full 128-block boundary
// below n, rows [0, n0) of L do not depend on later rows and are kept; the t = n - n0 rows of
// the old partial block and the k new samples (the "active" rows) are redone, so the identity
// padding stays at the end of the factor:
//   panel   P = L[n0.., 0..n0): the old tail's rows are in A, the new rows are
//           K(Xnew, X[0:n0]) L00^{-T} (one chained panel launch, k_append.hip, or trsm_rows);
//   block   S = K(act, act) + s^2 I - P P^T, identity-padded to 128, factored in place
//           (its diagonal-block inverses into Linv);
//   labels  z = L^{-1} Y for ALL rows against the whole new factor (the label rows found in A
//           are not reused: refine_f32 leaves residuals there), alpha by the chained back
//           substitution, log det and data fit by the fit's reductions over all n + k rows.
// Nothing the fitted model reads is replaced before the status words are known: a grown
// factor is built in new buffers (one O(N^2) copy per 128 appended rows), an update inside
// the existing padding stashes the 128 x 128 partial block and its inverse and restores them
// (and the zero panel rows) when the update is refused; alpha is solved into a second buffer.
// ---------------------------------------------------------------------------------------
template <typename T>
gprx_status model_append(gprx_model* M, const void* Xnew, const void* Ynew, int64_t k, uint32_t flags,
                         gprx_fit_info* out) {
    gprx_ctx* ctx = M->ctx;
    GPRX_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int d = M->d, m = M->m;
    const int64_t n = M->n, n1 = n + k;
    const uint32_t fit_flags = flags & (GPRX_FIT_NO_LU_FALLBACK | GPRX_FIT_F32_NO_REFINE);
    M->trim_posterior_workspace();
    // the new rows behind the old ones (row-major: contiguous); nothing reads them before n is
    // published.  Host or device memory, as gprx_model_set_data.
    grow_keep(M->X, sizeof(T) * n1 * d, sizeof(T) * n * d, s);
    grow_keep(M->Y, sizeof(T) * n1 * m, sizeof(T) * n * m, s);
    GPRX_HIP(hipStreamSynchronize(s));
    if (M->scaled()) {  // the new rows as uploaded behind Xraw's, scaled into X
        grow_keep(M->Xraw, sizeof(T) * n1 * d, sizeof(T) * n * d, s);
        GPRX_HIP(hipMemcpy(M->Xraw.as<T>() + n * d, Xnew, sizeof(T) * k * d, hipMemcpyDefault));
        scale_model_rows<T>(M, n, k);
        GPRX_HIP(hipStreamSynchronize(s));
    } else {
        GPRX_HIP(hipMemcpy(M->X.as<T>() + n * d, Xnew, sizeof(T) * k * d, hipMemcpyDefault));
    }
    GPRX_HIP(hipMemcpy(M->Y.as<T>() + n * m, Ynew, sizeof(T) * k * m, hipMemcpyDefault));
    // full refit of the extended data: the factor is the LU (a forced LU stays one), or the
    // trailing Cholesky below met a non-positive pivot
    auto refit = [&](uint32_t f) {
        M->n = n1;
        M->drop_fit();
        return model_fit<T>(M, f, out);
    };
    if (M->method == 1 || M->dist_fitted) return refit(fit_flags | (M->method == 1 && M->lu_forced ? GPRX_FIT_FORCE_LU : 0u));

    const int64_t np = M->np, mp = M->mp;
    const int64_t n0 = n / DB * DB, t = n - n0, na = t + k, np1 = round_up(n1, (int64_t)DB), nap = np1 - n0;
    const bool relay = np1 > np;  // the padding is used up: A, Linv re-laid (never the inverse rows of a want_inv fit)
    const int64_t ld0 = M->ld, ld1 = relay ? np1 + mp : ld0;
    const bool gemm = (flags & GPRX_APPEND_SOLVE_GEMM) != 0;
    const bool gemm_new = gemm || k > DB;  // the new rows' panel: chained kernel up to 128 rows
    DevBuf newA, newLinv;
    T *A1, *Li1;
    if (relay) {
        newA.ensure(sizeof(T) * ld1 * np1);
        newLinv.ensure(sizeof(T) * np1 * DB);
        A1 = newA.as<T>();
        Li1 = newLinv.as<T>();
        GPRX_HIP(hipMemset2DAsync(A1 + np, sizeof(T) * ld1, 0, sizeof(T) * (ld1 - np), np, s));
        GPRX_HIP(hipMemsetAsync(A1 + np * ld1, 0, sizeof(T) * ld1 * (np1 - np), s));
        GPRX_HIP(hipMemcpy2DAsync(A1, sizeof(T) * ld1, M->A.p, sizeof(T) * ld0, sizeof(T) * np, np,
                                  hipMemcpyDeviceToDevice, s));
        GPRX_HIP(hipMemcpyAsync(Li1, M->Linv.p, sizeof(T) * np * DB, hipMemcpyDeviceToDevice, s));
    } else {  // (then t > 0: the partial block is the last one, n0 = np - 128)
        A1 = M->A.as<T>();
        Li1 = M->Linv.as<T>();
        M->apStash.ensure(2 * sizeof(T) * DB * DB);
        T* st = M->apStash.as<T>();
        GPRX_HIP(hipMemcpy2DAsync(st, sizeof(T) * DB, A1 + n0 + n0 * ld1, sizeof(T) * ld1, sizeof(T) * DB, DB,
                                  hipMemcpyDeviceToDevice, s));
        GPRX_HIP(hipMemcpyAsync(st + DB * DB, Li1 + n0 * DB, sizeof(T) * DB * DB, hipMemcpyDeviceToDevice, s));
        if (n0 > 0) GPRX_HIP(hipMemset2DAsync(A1 + n, sizeof(T) * ld1, 0, sizeof(T) * (np1 - n), n0, s));
    }
    auto restore = [&]() {  // the fitted model as it was (an update inside the padding wrote into A, Linv)
        if (relay) return;
        T* st = M->apStash.as<T>();
        GPRX_HIP(hipMemcpy2DAsync(A1 + n0 + n0 * ld1, sizeof(T) * ld1, st, sizeof(T) * DB, sizeof(T) * DB, DB,
                                  hipMemcpyDeviceToDevice, s));
        GPRX_HIP(hipMemcpyAsync(Li1 + n0 * DB, st + DB * DB, sizeof(T) * DB * DB, hipMemcpyDeviceToDevice, s));
        if (n0 > 0) GPRX_HIP(hipMemset2DAsync(A1 + n, sizeof(T) * ld1, 0, sizeof(T) * (np1 - n), n0, s));
        GPRX_HIP(hipStreamSynchronize(s));
    };
    M->info.ensure(sizeof(int));
    M->flag.ensure(sizeof(int));
    M->red.ensure(sizeof(double) * (2 + 2 * (np1 / GT + 1)));
    M->apAlpha.ensure(sizeof(T) * np1 * m);
    launch_fit_status_init(M->info.as<int>(), M->flag.as<int>(), s);
    const T sig = (T)M->sigma;
    const T sigma2 = sig * sig;
    const T* Xall = M->X.as<T>();
    const T* Xact = Xall + n0 * d;
    const T* Xn = Xall + n * d;
    // the cross rows as MFMA pair statistics under solve_rows_for's conditions (fp64 only)
    const bool cross_mma = std::is_same<T, double>::value && !env_predict_direct() && pairs_mma_supported<T>(K, 1);
    GPRX_HIP(hipEventRecord(ctx->ev[0], s));
    // sin/cos tables of the sample ranges the builds read (a table's planes are n x d of ITS range)
    T *tabAct = nullptr, *tabNew = nullptr, *tabLead = nullptr;
    if (K.nper > 0) {
        const int64_t pl = 2 * K.nper * (int64_t)d;
        const bool lead = n0 > 0 && !cross_mma;
        M->apTab.ensure(sizeof(T) * pl * (na + k + (lead ? n0 : 0)));
        tabAct = M->apTab.as<T>();
        launch_sincos_tables<T>(K, Xact, na, d, tabAct, s);
        if (lead) {  // the VALU cross build's two sides
            tabNew = tabAct + pl * na;
            tabLead = tabNew + pl * k;
            launch_sincos_tables<T>(K, Xn, k, d, tabNew, s);
            launch_sincos_tables<T>(K, Xall, n0, d, tabLead, s);
        }
    }
    const int64_t ldp = round_up(k, (int64_t)GT);
    T* P = nullptr;
    if (n0 > 0) {  // K(Xnew, X[0:n0]) into the panel buffer (k x n0, zero rows up to ldp)
        M->apPanel.ensure(sizeof(T) * ldp * n0);
        P = M->apPanel.as<T>();
        GPRX_HIP(hipMemsetAsync(P, 0, sizeof(T) * ldp * n0, s));
        if (cross_mma) {
            const int64_t kf = pairs_feature_cols<T>(K, d);
            M->pvFq.ensure(sizeof(T) * ldp * kf);
            M->featV.ensure(sizeof(T) * n0 * kf);
            launch_pair_features<T>(K, Xall, n0, d, Xall, true, M->featV.as<T>(), n0, s);
            launch_pair_features<T>(K, Xn, k, d, Xall, false, M->pvFq.as<T>(), ldp, s, M->flag.as<int>());
            const KCanon<T>* kdev = M->kfit.put(K, s);
            launch_kcross_mma<T>(K, kdev, M->pvFq.as<T>(), ldp, k, M->featV.as<T>(), n0, n0, d, P, ldp,
                                 M->flag.as<int>(), s);
        } else {
            launch_kbuild<T>(K, Xn, tabNew, k, Xall, tabLead, n0, d, P, ldp, 0, false, T(0), M->flag.as<int>(), s);
        }
    }
    // K(act, act) + s^2 I, identity-padded, straight into A[n0.., n0..)
    T* S = A1 + n0 + n0 * ld1;
    launch_kbuild<T>(K, Xact, tabAct, na, Xact, tabAct, na, d, S, ld1, nap, true, sigma2, M->flag.as<int>(), s);
    GPRX_HIP(hipEventRecord(ctx->ev[1], s));
    if (n0 > 0) {
        if (gemm_new) trsm_rows<T>(A1, ld1, n0, Li1, P, ldp, ldp, s);
        else launch_forward_panel_chain<T>(A1, ld1, n0, Li1, P, ldp, (int)k, M->info.as<int>(), ctx->ex, s);
        launch_panel_rows<T>(P, ldp, k, n0, A1, ld1, n, s);
        // S -= P P^T.  A small trailing block under a long panel (the one-sample update: one
        // 128 x 128 tile, K = n0) is split over K, one 128-column slice per workgroup, and the
        // partials are summed in order (as one product the C3 one-sample update spent 1.2 ms more
        // of device time: 4.70 -> 3.52 ms, scripts/append_time.py)
        const int64_t nb0 = n0 / DB;
        if (nap <= 2 * DB && nb0 >= 8) {
            M->apPart.ensure(sizeof(T) * nb0 * nap * nap);
            GPRX_HIP(hipMemsetAsync(M->apPart.p, 0, sizeof(T) * nb0 * nap * nap, s));
            launch_gemm_nt_splitk<T>(M->apPart.as<T>(), nap, nap * nap, A1 + n0, ld1, A1 + n0, ld1, nap, nap, DB,
                                     (int)nb0, T(-1), true, s);
            launch_schur_sum<T>(S, ld1, M->apPart.as<T>(), nap, (int)nb0, s);
        } else {
            launch_gemm_nt<T>(S, ld1, A1 + n0, ld1, A1 + n0, ld1, nap, nap, n0, T(-1), T(1), true, s);
        }
    }
    potrf_tiles<T>(S, ld1, nap, nap, Li1 + n0 * DB, M->info.as<int>(), ctx->ex);
    GPRX_HIP(hipEventRecord(ctx->ev[2], s));
    launch_label_rows<T>(M->Y.as<T>(), n1, m, A1, ld1, np1, np1, mp, s);
    if (gemm) {
        trsm_rows<T>(A1, ld1, np1, Li1, A1 + np1, ld1, mp, s);
    } else {
        for (int r0 = 0; r0 < m; r0 += DB)  // slabs of 128 label rows
            launch_forward_panel_chain<T>(A1, ld1, np1, Li1, A1 + np1 + r0, ld1, std::min(DB, m - r0),
                                          M->info.as<int>(), ctx->ex, s);
    }
    launch_fit_reductions<T>(A1, ld1, n1, np1, m, M->red.as<double>(), s);
    launch_backsolve_chain<T>(A1, ld1, np1, m, Li1, M->apAlpha.as<T>(), M->info.as<int>(), ctx->ex, s);
    GPRX_HIP(hipEventRecord(ctx->ev[3], s));
    const FitStatus st = read_fit_status(M, s);
    const int hflag = st.flag, hinfo = st.info;
    if (hflag || hinfo < 0) {
        restore();
        check_finite(hflag);
        check_sched(hinfo);
    }
    if (hinfo != INT_MAX) return refit(fit_flags);  // not positive definite: the fit's LU fallback or NOT_SPD
    // publish
    if (relay) {
        swap_buf(M->A, newA);
        swap_buf(M->Linv, newLinv);
    }
    swap_buf(M->alpha, M->apAlpha);
    M->n = n1;
    M->np = np1;
    M->ld = ld1;
    M->fit_done(0, false);
    ensure_train_tables<T>(M);
    if (out) {
        std::memset(out, 0, sizeof(*out));
        add_phase_times(ctx, out);
        out->logdet = st.logdet;
        out->datafit = st.datafit;
        out->appended = (int32_t)k;
    }
    if constexpr (std::is_same<T, float>::value) {
        if (!(flags & GPRX_FIT_F32_NO_REFINE)) refine_f32(M, out);
    }
    return GPRX_OK;
}

// ---------------------------------------------------------------------------------------
// gprx_model_remove: the samples [first, first + count) taken out of a fitted model by UPDATING
// the Cholesky factor instead of refitting.  With the old factor partitioned at f = first and
// f + r, [L11 0 0; L21 L22 0; L31 L32 L33], the reduced matrix has the factor [L11 0; L31 L33']
// with L33' L33'^T = L33 L33^T + L32 L32^T: rows above f are kept, columns left of f only move
// up by r, and the trailing block takes a rank-r update by Givens rotations (k_remove.hip, one
// chained launch per 16 vectors), which also writes the identity padding and the new diagonal
// blocks' inverses.  Column blocks before b0 = f / 128 are plain copies.  The labels are redone
// exactly as the append does (label rows, chained forward panel solve over all rows, the fit's
// reductions, chained back substitution into a second alpha).
// Everything is built in second buffers (factor, Linv, X, Y, alpha: the update costs a second
// factor's memory) and swapped in once the status words are known, so a refused update leaves
// the fitted model as it was.  An LU-factored model, or more than GPRX_REMOVE_CUTOVER samples,
// reduces the data and refits in full.
// ---------------------------------------------------------------------------------------
template <typename T>
gprx_status model_remove(gprx_model* M, int64_t first, int64_t count, uint32_t flags, gprx_fit_info* out) {
    gprx_ctx* ctx = M->ctx;
    GPRX_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int d = M->d, m = M->m;
    const int64_t n = M->n, f = first, r = count, n1 = n - r;
    const uint32_t fit_flags = flags & (GPRX_FIT_NO_LU_FALLBACK | GPRX_FIT_F32_NO_REFINE);
    M->trim_posterior_workspace();
    // X and Y without rows [f, f + r) (row-major: the rows before and the rows after)
    auto compact = [&](const DevBuf& from, DevBuf& to, int w) {
        to.ensure(std::max(from.bytes, sizeof(T) * (size_t)n1 * w));
        if (f > 0) GPRX_HIP(hipMemcpyAsync(to.p, from.p, sizeof(T) * f * w, hipMemcpyDeviceToDevice, s));
        if (n1 > f)
            GPRX_HIP(hipMemcpyAsync(to.as<T>() + f * w, from.as<T>() + (f + r) * w, sizeof(T) * (n1 - f) * w,
                                    hipMemcpyDeviceToDevice, s));
    };
    compact(M->X, M->rmX, d);
    compact(M->Y, M->rmY, m);
    if (M->scaled()) compact(M->Xraw, M->rmXraw, d);  // (the points as uploaded move with the scaled ones)
    auto refit = [&](uint32_t fl) {  // full refit of the reduced data
        GPRX_HIP(hipStreamSynchronize(s));
        swap_buf(M->X, M->rmX);
        swap_buf(M->Y, M->rmY);
        if (M->scaled()) swap_buf(M->Xraw, M->rmXraw);
        M->n = n1;
        M->drop_fit();
        return model_fit<T>(M, fl, out);
    };
    if (M->method == 1 || r > GPRX_REMOVE_CUTOVER)
        return refit(fit_flags | (M->method == 1 && M->lu_forced ? GPRX_FIT_FORCE_LU : 0u));

    const int64_t mp = M->mp, np1 = round_up(n1, (int64_t)DB), ld0 = M->ld, ld1 = np1 + mp;
    const int b0 = (int)(f / DB), nb1 = (int)(np1 / DB);
    const int64_t c0 = (int64_t)b0 * DB;
    M->rmA.ensure(sizeof(T) * ld1 * np1);
    M->rmLinv.ensure(sizeof(T) * np1 * DB);
    M->info.ensure(sizeof(int));
    M->flag.ensure(sizeof(int));
    M->red.ensure(sizeof(double) * (2 + 2 * (np1 / GT + 1)));
    M->apAlpha.ensure(sizeof(T) * np1 * m);
    const T* A0 = M->A.as<T>();
    T* A1 = M->rmA.as<T>();
    T* Li1 = M->rmLinv.as<T>();
    launch_fit_status_init(M->info.as<int>(), M->flag.as<int>(), s);
    GPRX_HIP(hipEventRecord(ctx->ev[0], s));
    if (c0 > 0) {  // column blocks before b0: copied, the rows below f moved up by r, zero padding rows
        GPRX_HIP(hipMemcpy2DAsync(A1, sizeof(T) * ld1, A0, sizeof(T) * ld0, sizeof(T) * f, c0, hipMemcpyDeviceToDevice, s));
        if (n1 > f)
            GPRX_HIP(hipMemcpy2DAsync(A1 + f, sizeof(T) * ld1, A0 + f + r, sizeof(T) * ld0, sizeof(T) * (n1 - f), c0,
                                      hipMemcpyDeviceToDevice, s));
        if (np1 > n1) GPRX_HIP(hipMemset2DAsync(A1 + n1, sizeof(T) * ld1, 0, sizeof(T) * (np1 - n1), c0, s));
        GPRX_HIP(hipMemcpyAsync(Li1, M->Linv.p, sizeof(T) * c0 * DB, hipMemcpyDeviceToDevice, s));
    }
    GPRX_HIP(hipEventRecord(ctx->ev[1], s));
    if (b0 < nb1) {  // (a tail removal that ends on a block boundary leaves nothing to update)
        M->rmPairs.ensure(sizeof(T) * factor_update_ws_elems(nb1 - b0, (int)r));
        launch_factor_update<T>(A0, ld0, A1, ld1, Li1, A0 + r + f * ld0, ld0, (int)r, f, r, n1, b0, nb1,
                                M->rmPairs.as<T>(), M->info.as<int>(), ctx->ex, s);
    }
    GPRX_HIP(hipEventRecord(ctx->ev[2], s));
    launch_label_rows<T>(M->rmY.as<T>(), n1, m, A1, ld1, np1, np1, mp, s);
    for (int r0 = 0; r0 < m; r0 += DB)  // slabs of 128 label rows
        launch_forward_panel_chain<T>(A1, ld1, np1, Li1, A1 + np1 + r0, ld1, std::min(DB, m - r0), M->info.as<int>(),
                                      ctx->ex, s);
    launch_fit_reductions<T>(A1, ld1, n1, np1, m, M->red.as<double>(), s);
    launch_backsolve_chain<T>(A1, ld1, np1, m, Li1, M->apAlpha.as<T>(), M->info.as<int>(), ctx->ex, s);
    GPRX_HIP(hipEventRecord(ctx->ev[3], s));
    const FitStatus st = read_fit_status(M, s);
    check_finite(st.flag);
    check_sched(st.info);
    if (st.info != INT_MAX) return refit(fit_flags);  // (no step above reports a pivot)
    // publish
    swap_buf(M->A, M->rmA);
    swap_buf(M->Linv, M->rmLinv);
    swap_buf(M->X, M->rmX);
    swap_buf(M->Y, M->rmY);
    if (M->scaled()) swap_buf(M->Xraw, M->rmXraw);
    swap_buf(M->alpha, M->apAlpha);
    M->n = n1;
    M->np = np1;
    M->ld = ld1;
    M->fit_done(0, false);
    ensure_train_tables<T>(M);
    if (out) {
        std::memset(out, 0, sizeof(*out));
        add_phase_times(ctx, out);
        out->logdet = st.logdet;
        out->datafit = st.datafit;
        out->appended = -(int32_t)r;
    }
    if constexpr (std::is_same<T, float>::value) {
        if (!(flags & GPRX_FIT_F32_NO_REFINE)) refine_f32(M, out);
    }
    return GPRX_OK;
}

#define GPRX_INST(T)                                                                                      \
    template gprx_status model_fit<T>(gprx_model*, uint32_t, gprx_fit_info*);                              \
    template gprx_status model_remove<T>(gprx_model*, int64_t, int64_t, uint32_t, gprx_fit_info*);         \
    template gprx_status model_append<T>(gprx_model*, const void*, const void*, int64_t, uint32_t,         \
                                         gprx_fit_info*);                                                  \
    template void model_inverse<T>(gprx_model*);                                                           \
    template void ensure_dense_factor<T>(gprx_model*);
GPRX_INST(float)
GPRX_INST(double)
#undef GPRX_INST

}  // namespace gprx
