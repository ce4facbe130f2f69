// gprx_query.cpp — what reads a fitted model: predict, the posterior covariance (dense, LU, sharded,
// sparse), the core matrix, the log marginal likelihood, the leave-one-out cross-validation, the
// joint posterior with its draws and the caller-evaluated-kernel forms.
#include "gprx_model.h"

namespace gprx {

// the mean (q x m, row-major) of the staged queries Q into dmean, and with dder their derivative
// (q x d x m): what gprx_model_predict, _posterior and _sample all return as the mean
template <typename T>
static void predict_staged(gprx_model* M, const Points<T>& Q, int64_t q, T* dmean, T* dder) {
    hipStream_t s = M->ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int d = M->d, m = M->m;
    if (!dder && !env_predict_direct() && pairs_mma_supported<T>(K, m)) {
        // mean only: MFMA pair statistics, K(Xq, X) never materialised (k_pairs.hip)
        const int64_t qp = round_up(q, GT), npf = round_up(M->n, GT);
        DevBuf fq;
        train_features<T>(M, true, npf);
        query_features<T>(M, Q.x, q, qp, fq);
        launch_predict_mma<T>(K, M->kfit.put(K, s), fq.as<T>(), qp, M->featV.as<T>(), npf, d, M->alpha.as<T>(), M->n, m,
                              q, dmean, s);
        GPRX_HIP(hipStreamSynchronize(s));  // (fq is freed on return)
        return;
    }
    const int64_t ncz = (int64_t)m * (dder ? (1 + d) : 1);
    M->scratch1.ensure(sizeof(T) * M->n * ncz);
    M->scratch2.ensure(sizeof(T) * q * ncz);
    launch_predict<T>(K, M->X.as<T>(), M->tab.as<T>(), M->n, d, m, M->alpha.as<T>(), Q.x, Q.tab, q, dmean, dder,
                      M->scratch1.as<T>(), M->scratch2.as<T>(), s);
}

template <typename T>
gprx_status model_predict(gprx_model* M, const void* Xq, int64_t q, void* mean, void* deriv) {
    GPRX_REQUIRE(M->has_alpha, GPRX_ERR_STATE, "GaussianProcess::ComputeKernelVectorInternal: gaussian process is not initialized.");
    GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE, "gprx: a caller-evaluated kernel predicts through gprx_model_predict_kx");
    hipStream_t s = M->ctx->stream;
    const int d = M->d, m = M->m;
    Points<T> Q;
    DevBuf dmean, dder;
    stage_points<T>(Q, kcanon<T>(M), Xq, q, d, M->ctx->device, s, false, model_ell<T>(M));
    dmean.ensure(sizeof(T) * q * m);
    if (deriv) dder.ensure(sizeof(T) * q * d * m);
    predict_staged<T>(M, Q, q, dmean.as<T>(), deriv ? dder.as<T>() : nullptr);
    // with length scales the kernels differentiate in the scaled space: d/dx_j = (d/dz_j) / ell_j
    if (deriv && M->scaled()) launch_unscale_deriv<T>(dder.as<T>(), model_ell<T>(M), q, d, m, s);
    download(mean, dmean.p, sizeof(T) * q * m, s);
    if (deriv) download(deriv, dder.p, sizeof(T) * q * d * m, s);
    return GPRX_OK;
}

// events around the phases of a call, recorded only with the context's statistics on
struct PhaseClock {
    hipStream_t s;
    bool on;
    std::vector<hipEvent_t> ev;
    PhaseClock(gprx_ctx* ctx) : s(ctx->stream), on(ctx->prof.on) { mark(); }
    void mark() {
        if (!on) return;
        hipEvent_t e;
        GPRX_HIP(hipEventCreate(&e));
        ev.push_back(e);
        GPRX_HIP(hipEventRecord(e, s));
    }
    void read(double* ms, int n) {  // ms[k] = phase k (between marks k and k + 1)
        if (!on) return;
        GPRX_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < n && k + 1 < (int)ev.size(); k++) {
            float t = 0;
            (void)hipEventElapsedTime(&t, ev[k], ev[k + 1]);
            ms[k] = t;
        }
    }
    ~PhaseClock() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

// R = K(Xq, X) (qp x np, ld qp, zero padding), then R L^{-T} in place.  K(Xq, X) as MFMA pair
// statistics (kcross_mma_kernel: the predict path's features of the queries and of the training
// set) when the tree allows it -- 23 ms -> ~4 ms of the 300 ms variance leg at Q = 65536 against
// the VALU kernel (GPRX_PREDICT=direct keeps that one).  fp64 only: the variance k(x,x) -
// |L^{-1} k_x|^2 is a cancelling difference, and in fp32 the expanded |u|^2 + |v|^2 - 2 u.v
// statistic loses ~eps (|x - c|/l)^2 per entry, which L^{-1} amplifies; fp32 models
// keep the exact-difference VALU build.  feat_ready: the training features are already in
// featV (the second side of a pair call).
template <typename T>
static void solve_rows_for(gprx_model* M, const T* dXq, const T* dtabQ, int64_t q, int64_t qp, T* R,
                           bool feat_ready = false, PhaseClock* pc = nullptr) {
    hipStream_t s = M->ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int64_t npf = round_up(M->n, GT);
    const bool cross_mma =
        std::is_same<T, double>::value && !env_predict_direct() && pairs_mma_supported<T>(K, 1) && npf <= M->np;
    // R must be zero outside the q x n cross block (the solves run over qp x np); the MFMA cross
    // build stores every entry of that block, so with no padding there is nothing to zero (the
    // memset was 8.6 GB, 1.3 ms, per solve at Q = 65536, N = 16384)
    if (!cross_mma || q != qp || M->n != M->np) GPRX_HIP(hipMemsetAsync(R, 0, sizeof(T) * qp * M->np, s));
    if (cross_mma) {
        if (!feat_ready) train_features<T>(M, true, npf);
        query_features<T>(M, dXq, q, qp, M->pvFq);  // (model-owned: no hipMalloc + hipFree per call)
        const KCanon<T>* kdev = M->kfit.put(K, s);
        launch_kcross_mma<T>(K, kdev, M->pvFq.as<T>(), qp, q, M->featV.as<T>(), npf, M->n, M->d, R, qp,
                             M->flag.as<int>(), s);
    } else {
        launch_kbuild<T>(K, dXq, dtabQ, q, M->X.as<T>(), M->tab.as<T>(), M->n, M->d, R, qp, 0, false, T(0),
                         M->flag.as<int>(), s);
    }
    if (pc) pc->mark();  // (the cross build | the row solve)
    trsm_rows<T>(M->A.as<T>(), M->ld, M->np, M->Linv.as<T>(), R, qp, qp, s);
    if (pc) pc->mark();
}

// operator()(x, y) / GetCredibleInterval (lib/GaussianProcess.cpp:84-114) on a SHARDED fit:
// k(x, y) - (L^{-1} k_x) . (L^{-1} k_y) by the distributed forward substitution of the queries
// (dist_posterior, k_dsolve.hip dist_pvar_kernel): the ranks keep their own rows of L, the
// query columns V_k travel through the receive windows, the row sums are all-reduced.  Pairs
// (x_p, y_p) with x != y ride in the same chunk (64 + 64 columns), variances 128 per chunk.
template <typename T>
static gprx_status model_posterior_cov_dist_core(gprx_model* M, const void* Xa, const void* Xb, int64_t q, bool same,
                                                 void* out);

// FNV-1a over bytes (the processes' query agreement below)
static uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// On a multi-process context the sharded solve is a collective: every process runs the same
// sequence of launches and exchanges.  The processes first agree on their arguments (q, whether
// x == y, a hash of the queries).  Identical arguments (every process asks for the same pairs)
// take the solve as they are; different ones -- e.g. each process its own query_shard slice,
// q = 0 included -- are all-gathered, the solve runs once over every process's pairs, and each
// process keeps its own.
template <typename T>
static gprx_status model_posterior_cov_dist(gprx_model* M, const void* Xa, const void* Xb, int64_t q, void* out) {
    const int d = M->d;
    const bool same = q == 0 || (Xa == Xb) || std::memcmp(Xa, Xb, sizeof(T) * q * d) == 0;
    gprx_ctx* ctx = M->ctx;
    if (!ctx->hc || ctx->world <= 1) return model_posterior_cov_dist_core<T>(M, Xa, Xb, q, same, out);
    const int g = ctx->world;
    struct Hdr {
        int64_t q;
        int64_t same;
        uint64_t hash;
    } h{q, same ? 1 : 0, fnv1a(Xa, sizeof(T) * q * d, fnv1a(same ? Xa : Xb, sizeof(T) * q * d))};
    std::vector<Hdr> all(g);
    ctx->hc->allgather(&h, sizeof(Hdr), all.data());
    bool uniform = true;
    int64_t qmax = 0, qtot = 0;
    bool all_same = true;
    for (const Hdr& x : all) {
        uniform = uniform && x.q == h.q && x.same == h.same && x.hash == h.hash;
        qmax = std::max(qmax, x.q);
        qtot += x.q;
        all_same = all_same && x.same;
    }
    if (uniform) return q ? model_posterior_cov_dist_core<T>(M, Xa, Xb, q, same, out) : GPRX_OK;
    // every process's pairs, in rank order; this process's results from offset `off`
    std::vector<T> mine((size_t)qmax * d * 2, T(0));
    if (q) {
        std::memcpy(mine.data(), Xa, sizeof(T) * q * d);
        std::memcpy(mine.data() + (size_t)qmax * d, Xb, sizeof(T) * q * d);
    }
    std::vector<T> gath((size_t)qmax * d * 2 * g);
    ctx->hc->allgather(mine.data(), sizeof(T) * mine.size(), gath.data());
    std::vector<T> xa((size_t)std::max<int64_t>(qtot, 1) * d), xb((size_t)std::max<int64_t>(qtot, 1) * d);
    int64_t off = 0, mine_off = 0;
    for (int r = 0; r < g; r++) {
        const T* src = gath.data() + (size_t)r * qmax * d * 2;
        if (r == ctx->rank) mine_off = off;
        std::memcpy(xa.data() + off * d, src, sizeof(T) * all[r].q * d);
        std::memcpy(xb.data() + off * d, src + (size_t)qmax * d, sizeof(T) * all[r].q * d);
        off += all[r].q;
    }
    if (qtot == 0) return GPRX_OK;
    std::vector<T> res((size_t)qtot);
    model_posterior_cov_dist_core<T>(M, xa.data(), all_same ? xa.data() : xb.data(), qtot, all_same, res.data());
    if (q) std::memcpy(out, res.data() + mine_off, sizeof(T) * q);
    return GPRX_OK;
}

template <typename T>
static gprx_status model_posterior_cov_dist_core(gprx_model* M, const void* Xa, const void* Xb, int64_t q, bool same,
                                                 void* out) {
    hipStream_t s = M->ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int d = M->d;
    const int nchmax = dist_pvar_chunks(M->dist_engine);
    const int per = same ? DB : DB / 2;  // pairs per chunk
    const T* xa = static_cast<const T*>(Xa);
    const T* xb = static_cast<const T*>(Xb);
    DevBuf da, db, kab;
    Points<T> Zc;  // one chunk's query columns
    upload<T>(da, Xa, sizeof(T) * q * d, s);
    upload<T>(db, Xb, sizeof(T) * q * d, s);
    if (M->scaled()) {  // the prior pairs in the model's metric, as the staged chunks below
        launch_scale_points<T>(da.as<T>(), model_ell<T>(M), q, d, da.as<T>(), s);
        launch_scale_points<T>(db.as<T>(), model_ell<T>(M), q, d, db.as<T>(), s);
    }
    kab.ensure(sizeof(T) * q);
    launch_pair_kernel<T>(K, da.as<T>(), db.as<T>(), q, d, kab.as<T>(), s);
    std::vector<T> hk((size_t)q), res((size_t)q);
    download(hk.data(), kab.p, sizeof(T) * q, s);
    std::vector<double> sum;
    for (int64_t p0 = 0; p0 < q;) {
        const int64_t cnt = std::min<int64_t>(q - p0, (int64_t)nchmax * per);
        const int nch = (int)((cnt + per - 1) / per);
        const int64_t nq = (int64_t)nch * DB;
        std::vector<T> Z((size_t)nq * d, T(0));
        for (int64_t j = 0; j < cnt; j++) {
            const int64_t c = j / per, jj = j % per;
            std::memcpy(&Z[(size_t)(c * DB + jj) * d], xa + (p0 + j) * d, sizeof(T) * d);
            if (!same) std::memcpy(&Z[(size_t)(c * DB + DB / 2 + jj) * d], xb + (p0 + j) * d, sizeof(T) * d);
        }
        stage_points<T>(Zc, K, Z.data(), nq, d, M->ctx->device, s, false, model_ell<T>(M));
        dist_posterior<T>(M->dist_engine, K, M->X.as<T>(), K.nper > 0 ? M->tab.as<T>() : nullptr, M->n, d, Zc.x, Zc.tab,
                          nch, !same, sum, s);
        for (int64_t j = 0; j < cnt; j++) res[p0 + j] = (T)((double)hk[p0 + j] - sum[(j / per) * DB + j % per]);
        p0 += cnt;
    }
    std::memcpy(out, res.data(), sizeof(T) * q);
    return GPRX_OK;
}

template <typename T>
gprx_status model_posterior_cov(gprx_model* M, const void* Xa, const void* Xb, int64_t q, void* out) {
    GPRX_REQUIRE(M->fitted || M->sparse_cov, GPRX_ERR_STATE,
                 "GaussianProcess::ComputeKernelVectorInternal: gaussian process is not initialized.");
    GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE, "gprx: a caller-evaluated kernel uses gprx_model_posterior_cov_kx");
    // a sharded fit solves the queries across the ranks (GPRX_DIST_POSTERIOR=dense: the dense
    // factor gathered onto this process instead, as for the core matrix)
    static const bool dense_forced = std::getenv("GPRX_DIST_POSTERIOR") &&
                                     std::string(std::getenv("GPRX_DIST_POSTERIOR")) == "dense";
    if (M->dist_fitted && !M->dist_dense && M->method == 0 && !dense_forced && dist_pvar_chunks(M->dist_engine) > 0)
        return model_posterior_cov_dist<T>(M, Xa, Xb, q, out);
    ensure_dense_factor<T>(M);  // (collective on a sharded fit's first dense use)
    if (q == 0) return GPRX_OK;
    hipStream_t s = M->ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int d = M->d;
    const int64_t qp = round_up(q, GT);
    Points<T> Pa, Pb;
    DevBuf Ra, Rb, kab, res;
    stage_points<T>(Pa, K, Xa, q, d, M->ctx->device, s, false, model_ell<T>(M));
    stage_points<T>(Pb, K, Xb, q, d, M->ctx->device, s, false, model_ell<T>(M));
    if (M->sparse_cov) {  // k(x,y) - Kx^T W Ky over the inducing points, batched on the device
        const int64_t Mp = round_up(M->n, GT);
        DevBuf Z;
        Ra.ensure(sizeof(T) * qp * Mp);
        Rb.ensure(sizeof(T) * qp * Mp);
        Z.ensure(sizeof(T) * qp * Mp);
        GPRX_HIP(hipMemsetAsync(Ra.p, 0, sizeof(T) * qp * Mp, s));
        GPRX_HIP(hipMemsetAsync(Rb.p, 0, sizeof(T) * qp * Mp, s));
        launch_kbuild<T>(K, Pa.x, Pa.tab, q, M->X.as<T>(), M->tab.as<T>(), M->n, d, Ra.as<T>(), qp, 0, false,
                         T(0), M->flag.as<int>(), s);
        launch_kbuild<T>(K, Pb.x, Pb.tab, q, M->X.as<T>(), M->tab.as<T>(), M->n, d, Rb.as<T>(), qp, 0, false,
                         T(0), M->flag.as<int>(), s);
        launch_gemm_nt<T>(Z.as<T>(), qp, Rb.as<T>(), qp, M->sparseW.as<T>(), Mp, qp, Mp, Mp, T(1), T(0), false, s);
        kab.ensure(sizeof(T) * q);
        res.ensure(sizeof(T) * q);
        launch_pair_kernel<T>(K, Pa.x, Pb.x, q, d, kab.as<T>(), s);
        launch_rowdot<T>(Ra.as<T>(), Z.as<T>(), qp, q, Mp, kab.as<T>(), res.as<T>(), s);
        download(out, res.p, sizeof(T) * q, s);
        return GPRX_OK;
    }
    if (M->method == 1) {  // LU factors: k(x,y) - K(X,x)^T A^{-1} K(X,y), the reference's formula (:84-99)
        const int64_t np = M->np;
        DevBuf Kt, Wd, Kad;
        Wd.ensure(sizeof(double) * np * q);
        Kad.ensure(sizeof(double) * np * q);
        auto cross = [&](const T* Xq, const T* tq, double* dst) {  // K(X, Xq): np x q column-major
            T* buf;
            if constexpr (std::is_same<T, double>::value) {
                buf = dst;
            } else {
                Kt.ensure(sizeof(T) * np * q);
                buf = Kt.as<T>();
            }
            GPRX_HIP(hipMemsetAsync(buf, 0, sizeof(T) * np * q, s));
            launch_kbuild<T>(K, M->X.as<T>(), M->tab.as<T>(), M->n, Xq, tq, q, d, buf, np, 0, false, T(0),
                             M->flag.as<int>(), s);
            if constexpr (!std::is_same<T, double>::value) launch_convert<T, double>(buf, dst, np * q, s);
        };
        cross(Pb.x, Pb.tab, Wd.as<double>());
        lu_solve_model(M, Wd.as<double>(), (int)q);
        cross(Pa.x, Pa.tab, Kad.as<double>());
        kab.ensure(sizeof(T) * q);
        res.ensure(sizeof(T) * q);
        launch_pair_kernel<T>(K, Pa.x, Pb.x, q, d, kab.as<T>(), s);
        lu_coldot<T>(Kad.as<double>(), Wd.as<double>(), np, M->n, q, kab.as<T>(), res.as<T>(), s);
        download(out, res.p, sizeof(T) * q, s);
        return GPRX_OK;
    }
    // the variance (GetCredibleInterval, :102-114, pairs (x, x)): one solve, |L^{-1} k_x|^2
    const bool same = (Xa == Xb) || std::memcmp(Xa, Xb, sizeof(T) * q * d) == 0;
    kab.ensure(sizeof(T) * q);
    res.ensure(sizeof(T) * q);
    M->pvRa.ensure(sizeof(T) * qp * M->np);
    if (!same) M->pvRb.ensure(sizeof(T) * qp * M->np);
    {
        // device time of the whole solve (stats class "posterior"): K(x, X), the forward
        // solve (q np^2 flop) and the row dots
        ProfScope ps_(KC_POSTERIOR, s, (same ? 1.0 : 2.0) * (double)q * (double)M->np * (double)M->np);
        T* Ra_ = M->pvRa.as<T>();
        solve_rows_for<T>(M, Pa.x, Pa.tab, q, qp, Ra_);
        if (!same) solve_rows_for<T>(M, Pb.x, Pb.tab, q, qp, M->pvRb.as<T>(), true);
        launch_pair_kernel<T>(K, Pa.x, Pb.x, q, d, kab.as<T>(), s);
        launch_rowdot<T>(Ra_, same ? Ra_ : M->pvRb.as<T>(), qp, q, M->np, kab.as<T>(), res.as<T>(), s);
    }
    download(out, res.p, sizeof(T) * q, s);
    return GPRX_OK;
}

// the explicit inverse from the LU factors (A^{-1} I, double, np x np column-major in luC)
static void lu_inverse(gprx_model* M, DevBuf& luC) {
    const int64_t np = M->np;
    luC.ensure(sizeof(double) * np * np);
    GPRX_HIP(hipMemsetAsync(luC.p, 0, sizeof(double) * np * np, M->ctx->stream));
    launch_set_identity_pad<double>(luC.as<double>(), np, 0, np, M->ctx->stream);
    lu_solve_model(M, luC.as<double>(), (int)np);
}

template <typename T>
gprx_status model_core_matrix(gprx_model* M, void* Cout) {
    GPRX_REQUIRE(M->fitted, GPRX_ERR_STATE, "gprx: model is not fitted");
    ensure_dense_factor<T>(M);
    hipStream_t s = M->ctx->stream;
    if (M->method == 1) {  // dgetri_'s inverse (include/LAPACKUtils.h:49) from the LU factors
        DevBuf luC;
        lu_inverse(M, luC);
        const int64_t n = M->n, np = M->np;
        std::vector<double> h((size_t)n * n);
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipGetLastError());
        GPRX_HIP(hipMemcpy2D(h.data(), sizeof(double) * n, luC.p, sizeof(double) * np, sizeof(double) * n, n,
                             hipMemcpyDeviceToHost));
        T* C = reinterpret_cast<T*>(Cout);
        for (int64_t j = 0; j < n; j++)
            for (int64_t i = 0; i < n; i++) C[(size_t)i * n + j] = (T)h[(size_t)j * n + i];
        return GPRX_OK;
    }
    model_inverse<T>(M);
    const int64_t n = M->n, np = M->np;
    std::vector<T> h((size_t)n * n);
    // column j of C (lower part rows >= j) -> row-major; C symmetric
    GPRX_HIP(hipStreamSynchronize(s));
    GPRX_HIP(hipGetLastError());
    GPRX_HIP(hipMemcpy2D(h.data(), sizeof(T) * n, M->C.p, sizeof(T) * np, sizeof(T) * n, n, hipMemcpyDeviceToHost));
    mirror_lower<T>(h.data(), n, n, reinterpret_cast<T*>(Cout));  // h[j*n + i] = C(i, j) valid for i >= j
    return GPRX_OK;
}

// C = the LU factors' inverse in the model's T (the reference casts back), for the gradients
template <typename T>
static void lu_inverse_to_C(gprx_model* M) {
    hipStream_t s = M->ctx->stream;
    const int64_t np = M->np;
    DevBuf luC;
    lu_inverse(M, luC);
    M->C.ensure(sizeof(T) * np * np);
    if constexpr (std::is_same<T, double>::value)
        GPRX_HIP(hipMemcpyAsync(M->C.p, luC.p, sizeof(double) * np * np, hipMemcpyDeviceToDevice, s));
    else
        launch_convert<double, T>(luC.as<double>(), M->C.as<T>(), np * np, s);
    GPRX_HIP(hipStreamSynchronize(s));
}

template <typename T>
gprx_status model_lml(gprx_model* M, uint32_t flags, double* value, double* grad, int32_t* nparams,
                      double* logdet) {
    GPRX_REQUIRE(M->m == 1, GPRX_ERR_DIM,
                 "GaussianLogLikelihood: only one output dimension is supported (the reference's data-fit term is "
                 "m x m, include/Likelihood.h:175)");
    GPRX_REQUIRE(!(M->host_k && grad && (flags & GPRX_LML_GRAD)), GPRX_ERR_STATE,
                 "gprx: a caller-evaluated kernel takes its derivative matrices through gprx_model_lml_dk");
    gprx_fit_info fi;
    M->want_inv = grad && (flags & GPRX_LML_GRAD);
    gprx_status st;
    try {
        // the likelihood inverts with the GP's method too (include/Likelihood.h:77-79 ->
        // ComputeCoreMatrixWithDeterminant): a matrix the Cholesky rejects takes the LU
        // the value and gradient come from the factor (and its inverse), never from alpha:
        // an fp32 model's fp64 refinement of alpha would be thrown away (GPRX_FIT_F32_NO_REFINE)
        st = model_fit<T>(M,
                          ((flags & GPRX_LML_DISTRIBUTED) ? GPRX_FIT_DISTRIBUTED : 0u) |
                              ((flags & GPRX_LML_FORCE_LU) ? GPRX_FIT_FORCE_LU : 0u) | GPRX_FIT_F32_NO_REFINE,
                          &fi);
    } catch (...) {
        M->want_inv = false;
        throw;
    }
    M->want_inv = false;
    if (st != GPRX_OK) return st;
    const KCanon<T>& K = kcanon<T>(M);
    const double n = (double)M->n;
    const T df = (T)(-0.5 * fi.datafit);
    const T ct = (T)(-n / 2.0 * std::log(2 * M_PI));  // include/Likelihood.h:192
    double v;
    // LU fits can have det <= 0: the reference's clamp (:180-188) applies in both modes
    const double det_sign = (M->method == 1) ? M->lu_sign : 1.0;
    if ((flags & GPRX_LML_COMPAT) || det_sign <= 0) {
        // include/Likelihood.h:77-79 narrows the long-double determinant to T, :180-188 clamps
        typedef long double HP;
        const HP det_ld = (HP)det_sign * std::exp((HP)fi.logdet);
        const HP det = (HP)(T)det_ld;
        HP cp;
        if (det <= std::numeric_limits<HP>::min()) cp = -0.5L * std::log(std::numeric_limits<HP>::min());
        else if (det > std::numeric_limits<HP>::max()) cp = -0.5L * std::log(std::numeric_limits<HP>::max());
        else cp = -0.5L * std::log(det);
        v = (double)(T)(df + (T)(cp + ct));
    } else {
        v = (double)df - 0.5 * fi.logdet + (double)ct;
    }
    if (std::isinf(v))
        throw Error{GPRX_ERR_NONFINITE, "GaussianLogLikelihood::GetValueAndParameterDerivatives: likelihood is infinite."};
    if (value) *value = v;
    if (logdet) *logdet = fi.logdet;
    if (nparams) *nparams = K.nparams;
    if (grad && (flags & GPRX_LML_GRAD)) {
        hipStream_t s = M->ctx->stream;
        if (M->method == 1) {
            lu_inverse_to_C<T>(M);
        } else if (!M->inv_ready || (M->dist_fitted && !M->dist_inv_tiles && !M->dist_dense)) {
            ensure_dense_factor<T>(M);
            model_inverse<T>(M);
        }
        M->grad.ensure(sizeof(double) * MAX_LEAF * 3);
        GPRX_HIP(hipMemsetAsync(M->grad.p, 0, sizeof(double) * MAX_LEAF * 3, s));
        const int64_t np = M->np, npf = round_up(M->n, GT);
        if (!env_lml_grad_direct() && npf == np && pairs_grad_supported<T>(K)) {
            // pair statistics (and the periodic b-derivative statistic) on the MFMA units
            const int64_t kg = pairs_grad_feature_cols<T>(K, M->d);
            train_features<T>(M, false, np);
            train_features<T>(M, true, np);
            const KCanon<T>* kdev = M->kfit.put(K, s);
            M->scratch1.ensure(sizeof(T) * np * std::max<int64_t>(kg, 1));
            M->scratch2.ensure(sizeof(T) * np * std::max<int64_t>(kg, 1));
            const int64_t nt = np / GT;
            M->pack.ensure(sizeof(double) * MAX_LEAF * 3 * nt * (nt + 1) / 2);
            if (M->dist_fitted && M->dist_inv_tiles) {
                // sharded fit in LML mode: each rank sums (alpha alpha^T - C) o dK/dp over the
                // lower tiles of its own row blocks, C straight from its packed C tiles (the
                // sharded potri riding along in the factorisation); one reduction over the ranks
                dist_lml_grad<T>(M->dist_engine, K, kdev, M->X.as<T>(), M->n, M->d,
                                 M->featU.as<T>(), M->featV.as<T>(), M->scratch1.as<T>(), M->scratch2.as<T>(), np,
                                 M->alpha.as<T>(), M->pack.as<double>(), M->grad.as<double>(), s);
            } else {
                launch_lml_grad_mma<T>(K, kdev, M->X.as<T>(), M->n, M->d, M->featU.as<T>(),
                                       M->featV.as<T>(), M->scratch1.as<T>(), M->scratch2.as<T>(), np,
                                       M->alpha.as<T>(), M->C.as<T>(), M->np, M->pack.as<double>(),
                                       M->grad.as<double>(), s);
            }
        } else {
            launch_lml_grad<T>(K, M->X.as<T>(), M->tab.as<T>(), M->n, M->d, M->alpha.as<T>(), M->C.as<T>(), M->np,
                               M->grad.as<double>(), s);
        }
        double acc[MAX_LEAF * 3];
        download(acc, M->grad.p, sizeof(acc), s);
        for (int l = 0; l < K.nleaf; l++) {
            const int t = K.leaf[l].type;
            const int np = leaf_type_nparams(t);
            for (int q = 0; q < np; q++) grad[K.param_base[l] + q] = 0.5 * acc[l * 3 + q];
        }
    }
    return GPRX_OK;
}

// ---------------------------------------------------------------------------------------
// Leave-one-out cross-validation (k_loo.hip; GPML 5.4.2, not in the reference): the held-out
// means and variances of every sample, the predictive log probability and its gradient from
// what a Cholesky fit leaves resident.  A fitted model is read, never refitted; the call's own
// buffers: looVec (u, sqrt w, u / sqrt w, a), looPart (the reductions' partials), looOut (the
// results), looH (H / 2), and V, which nothing reads once C = V V^T exists, for B.
// ---------------------------------------------------------------------------------------
template <typename T>
gprx_status model_loo(gprx_model* M, uint32_t flags, double* value, void* mean, void* var, double* grad,
                      int32_t* nparams) {
    gprx_ctx* ctx = M->ctx;
    const bool want_grad = grad && (flags & GPRX_LOO_GRAD);
    GPRX_REQUIRE(!((ctx->hc && ctx->world > 1) || ctx->virt), GPRX_ERR_STATE,
                 "gprx_model_loo: sharded contexts (multi-rank or virtual-rank) are not supported");
    GPRX_REQUIRE(!M->sparse_cov, GPRX_ERR_STATE, "gprx_model_loo: a sparse-covariance model holds no factor");
    GPRX_REQUIRE(!(M->fitted && M->dist_fitted), GPRX_ERR_STATE, "gprx_model_loo: the model was fitted sharded");
    GPRX_REQUIRE(!(M->fitted && M->method == 1), GPRX_ERR_STATE,
                 "gprx_model_loo: the model's factor is an LU (leave-one-out needs the Cholesky factor)");
    GPRX_REQUIRE(!(M->host_k && want_grad), GPRX_ERR_STATE,
                 "gprx_model_loo: a caller-evaluated kernel has no device derivative (values only)");
    GPRX_REQUIRE(!(want_grad && M->m != 1), GPRX_ERR_DIM,
                 "gprx_model_loo: the gradient supports one output dimension only, as gprx_model_lml");
    if (!M->fitted) {  // data, kernel and noise but no fit: fitted here, the inverse riding along for a gradient
        M->want_inv = want_grad;
        gprx_status st;
        try {
            st = model_fit<T>(M, GPRX_FIT_NO_LU_FALLBACK, nullptr);
        } catch (...) {
            M->want_inv = false;
            throw;
        }
        M->want_inv = false;
        if (st != GPRX_OK) return st;
    }
    hipStream_t s = ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int64_t n = M->n, np = M->np;
    const int m = M->m;
    if (want_grad && !M->inv_ready) {
        model_inverse<T>(M);
        M->inverse_done();
    }
    const int64_t nvb = (np + 255) / 256;
    M->looPart.ensure(sizeof(double) * (loo_part_elems(np) + nvb + 1));
    M->looOut.ensure(sizeof(T) * (n * m + n));
    double* part = M->looPart.as<double>();
    double* vpart = part + loo_part_elems(np);
    double* dval = vpart + nvb;
    T* dmean = M->looOut.as<T>();
    T* dvar = dmean + n * m;
    T *u = nullptr, *sw = nullptr, *r = nullptr, *a = nullptr;
    if (want_grad) {
        M->looVec.ensure(sizeof(T) * 4 * np);
        u = M->looVec.as<T>();
        sw = u + np;
        r = sw + np;
        a = r + np;
    }
    const double* cpart = nullptr;
    if (!M->inv_ready) {  // diag(C) without C: the squared row norms of V = L^{-T}
        M->V.ensure(sizeof(T) * np * np);
        launch_factor_inverse_t<T>(M->A.as<T>(), M->ld, np, M->Linv.as<T>(), M->V.as<T>(), s);
        launch_loo_diag<T>(M->V.as<T>(), np, part, s);
        cpart = part;
    }
    launch_loo_vectors<T>(M->alpha.as<T>(), M->Y.as<T>(), n, np, m, cpart, M->C.as<T>(), np, dmean, dvar, u, sw, r, vpart,
                          dval, s);
    double v = 0;
    download(&v, dval, sizeof(double), s);
    if (!std::isfinite(v))
        throw Error{GPRX_ERR_NONFINITE, "gprx_model_loo: the leave-one-out log probability is not finite."};
    if (value) *value = v;
    if (nparams) *nparams = M->host_k ? 0 : K.nparams;
    if (mean) download(mean, dmean, sizeof(T) * n * m, s);
    if (var) download(var, dvar, sizeof(T) * n, s);
    if (!want_grad) return GPRX_OK;

    // B = sym(C) diag(sqrt w) into V, a = C u, H / 2 = B B^T / 2 (lower) on the tile mainloop
    M->V.ensure(sizeof(T) * np * np);
    M->looH.ensure(sizeof(T) * np * np);
    launch_loo_weights<T>(M->C.as<T>(), np, np, sw, r, M->V.as<T>(), part, a, s);
    GPRX_HIP(hipMemsetAsync(M->looH.p, 0, sizeof(T) * np * np, s));
    launch_syrk_splitk<T>(M->looH.as<T>(), np, 0, M->V.as<T>(), np, np, np, np, 1, T(0.5), s);
    // sum_kl dK_kl/dp ((a_k alpha_l + a_l alpha_k) / 2 - H_kl / 2): the LML's gradient pass in
    // its two-vector mode
    M->grad.ensure(sizeof(double) * MAX_LEAF * 3);
    GPRX_HIP(hipMemsetAsync(M->grad.p, 0, sizeof(double) * MAX_LEAF * 3, s));
    const int64_t npf = round_up(n, GT);
    if (!env_lml_grad_direct() && npf == np && pairs_grad_supported<T>(K)) {
        const int64_t kg = pairs_grad_feature_cols<T>(K, M->d);
        train_features<T>(M, false, np);
        train_features<T>(M, true, np);
        const KCanon<T>* kdev = M->kfit.put(K, s);
        M->scratch1.ensure(sizeof(T) * np * std::max<int64_t>(kg, 1));
        M->scratch2.ensure(sizeof(T) * np * std::max<int64_t>(kg, 1));
        const int64_t nt = np / GT;
        M->pack.ensure(sizeof(double) * MAX_LEAF * 3 * nt * (nt + 1) / 2);
        launch_loo_grad_mma<T>(K, kdev, M->X.as<T>(), n, M->d, M->featU.as<T>(), M->featV.as<T>(), M->scratch1.as<T>(),
                               M->scratch2.as<T>(), np, a, M->alpha.as<T>(), M->looH.as<T>(), np, M->pack.as<double>(),
                               M->grad.as<double>(), s);
    } else {
        ensure_train_tables<T>(M);
        launch_lml_grad<T>(K, M->X.as<T>(), M->tab.as<T>(), n, M->d, a, M->looH.as<T>(), np, M->grad.as<double>(), s,
                           M->alpha.as<T>());
    }
    double acc[MAX_LEAF * 3];
    download(acc, M->grad.p, sizeof(acc), s);
    for (int l = 0; l < K.nleaf; l++) {
        const int npl = leaf_type_nparams(K.leaf[l].type);
        for (int q = 0; q < npl; q++) grad[K.param_base[l] + q] = acc[l * 3 + q];
    }
    return GPRX_OK;
}

// ---------------------------------------------------------------------------------------
// d LML / d ell of a model with length scales (k_ard.hip; not in the reference): -(1 / ell_j) times
// the pair sum g_j = sum_{a != b} (alpha_a alpha_b - C_ab) dk/dr2 (z_aj - z_bj)^2 over the model's
// scaled points.  A model fitted by Cholesky is read as gprx_model_loo reads it (C formed from the
// factor when it is not resident); the call's own buffer is ardPart (the tiles' partials, then g).
// ---------------------------------------------------------------------------------------
template <typename T>
gprx_status model_lml_scale_grad(gprx_model* M, double* grad_ell) {
    gprx_ctx* ctx = M->ctx;
    GPRX_REQUIRE(M->scaled(), GPRX_ERR_STATE, "gprx_model_lml_scale_grad: no length scales are set");
    GPRX_REQUIRE(!((ctx->hc && ctx->world > 1) || ctx->virt), GPRX_ERR_STATE,
                 "gprx_model_lml_scale_grad: sharded contexts (multi-rank or virtual-rank) are not supported");
    GPRX_REQUIRE(!M->sparse_cov, GPRX_ERR_STATE, "gprx_model_lml_scale_grad: a sparse-covariance model holds no factor");
    GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE, "gprx_model_lml_scale_grad: a caller-evaluated kernel owns its own metric");
    GPRX_REQUIRE(M->fitted || (M->has_data && M->has_kernel), GPRX_ERR_STATE,
                 "gprx_model_lml_scale_grad: set the data, the kernel and the noise first");
    GPRX_REQUIRE(!(M->fitted && M->dist_fitted), GPRX_ERR_STATE, "gprx_model_lml_scale_grad: the model was fitted sharded");
    GPRX_REQUIRE(!(M->fitted && M->method == 1), GPRX_ERR_STATE,
                 "gprx_model_lml_scale_grad: the model's factor is an LU (the gradient needs the Cholesky factor)");
    const KCanon<T>& K = kcanon<T>(M);
    GPRX_REQUIRE(K.nper == 0, GPRX_ERR_STATE,
                 "gprx_model_lml_scale_grad: trees with a Periodic leaf are not supported (their values are)");
    GPRX_REQUIRE(M->m == 1, GPRX_ERR_DIM, "gprx_model_lml_scale_grad: only one output dimension is supported, as gprx_model_lml");
    const int d = M->d;
    if (!K.need_r2) {  // White leaves only: nothing depends on the metric off the diagonal
        for (int j = 0; j < d; j++) grad_ell[j] = 0.0;
        return GPRX_OK;
    }
    if (!M->fitted) {  // data, kernel and noise but no fit: fitted here, the inverse riding along
        M->want_inv = true;
        gprx_status st;
        try {
            st = model_fit<T>(M, GPRX_FIT_NO_LU_FALLBACK, nullptr);
        } catch (...) {
            M->want_inv = false;
            throw;
        }
        M->want_inv = false;
        if (st != GPRX_OK) return st;
    }
    hipStream_t s = ctx->stream;
    if (!M->inv_ready) {
        model_inverse<T>(M);
        M->inverse_done();
    }
    const int64_t n = M->n, npf = round_up(n, GT);
    train_features<T>(M, false, npf);
    train_features<T>(M, true, npf);
    const KCanon<T>* kdev = M->kfit.put(K, s);
    const int64_t pe = ard_part_elems(npf, d);
    M->ardPart.ensure(sizeof(double) * (pe + d));
    double* g = M->ardPart.as<double>() + pe;
    launch_ard_grad<T>(K, kdev, M->featU.as<T>(), M->featV.as<T>(), npf, n, d, M->alpha.as<T>(), M->alpha.as<T>(),
                       M->C.as<T>(), M->np, M->ardPart.as<double>(), g, s);
    download(grad_ell, g, sizeof(double) * d, s);
    for (int j = 0; j < d; j++) {
        if (!std::isfinite(grad_ell[j]))
            throw Error{GPRX_ERR_NONFINITE, "gprx_model_lml_scale_grad: the gradient is not finite."};
        grad_ell[j] = -grad_ell[j] / (double)(T)M->ell[j];
    }
    return GPRX_OK;
}

// ---------------------------------------------------------------------------------------
// The joint posterior over q query points and draws from it (k_sample.hip; not in the reference).
//   Sigma = K(Xq, Xq) [+ s^2 I] - R R^T,  R = K(Xq, X) L^{-T}  (solve_rows_for: the variance call's
//   rows), built lower and identity-padded to 128 exactly as gprx_model_append builds its block S;
//   a draw is mean + Lq z with Lq Lq^T = Sigma + j I (potrf_tiles on a copy, the strict upper part
//   zeroed, one launch_gemm_nt over all nsamp m columns of normals).
// The jitter j: the caller's, used once; or q eps max_p k(x_p, x_p) -- the scale of the
// factorisation's own backward error -- times 10 for every non-positive pivot met, refused with
// NOT_SPD once past 1e-2 max k.  A fitted model is read, never changed: everything lives in the
// ps* buffers, R in pvRa.
// ---------------------------------------------------------------------------------------
static void require_joint(gprx_model* M, const char* who) {
    gprx_ctx* ctx = M->ctx;
    const std::string w(who);
    GPRX_REQUIRE(!((ctx->hc && ctx->world > 1) || ctx->virt), GPRX_ERR_STATE,
                 w + ": sharded contexts (multi-rank or virtual-rank) are not supported");
    GPRX_REQUIRE(!M->sparse_cov, GPRX_ERR_STATE, w + ": a sparse-covariance model holds no factor");
    GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE, w + ": a caller-evaluated kernel has no device form to build K(Xq, Xq) with");
    GPRX_REQUIRE(M->fitted && M->has_alpha, GPRX_ERR_STATE, w + ": gaussian process is not initialized.");
    GPRX_REQUIRE(!M->dist_fitted, GPRX_ERR_STATE, w + ": the model was fitted sharded");
    GPRX_REQUIRE(M->method == 0, GPRX_ERR_STATE, w + ": the model's factor is an LU (the joint posterior needs the Cholesky factor)");
}

// Sigma + diag I (lower, identity-padded to qp, ld qp) into psS; the cross rows in pvRa
template <typename T>
static void joint_cov(gprx_model* M, const Points<T>& Q, int64_t q, int64_t qp, T diag, PhaseClock& pc) {
    hipStream_t s = M->ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    M->pvRa.ensure(sizeof(T) * qp * M->np);
    M->psS.ensure(sizeof(T) * qp * qp);
    T* R = M->pvRa.as<T>();
    T* S = M->psS.as<T>();
    solve_rows_for<T>(M, Q.x, Q.tab, q, qp, R, false, &pc);
    launch_kbuild<T>(K, Q.x, Q.tab, q, Q.x, Q.tab, q, M->d, S, qp, qp, true, diag, M->flag.as<int>(), s);
    launch_gemm_nt<T>(S, qp, R, qp, R, qp, qp, qp, M->np, T(-1), T(1), true, s);
    pc.mark();
}

template <typename T>
gprx_status model_posterior(gprx_model* M, const void* Xq, int64_t q, uint32_t flags, void* mean, void* cov) {
    require_joint(M, "gprx_model_posterior");
    hipStream_t s = M->ctx->stream;
    const int64_t qp = round_up(q, GT);
    Points<T> Q;
    stage_points<T>(Q, kcanon<T>(M), Xq, q, M->d, M->ctx->device, s, false, model_ell<T>(M));
    if (mean) {
        M->psVec.ensure(sizeof(T) * (q * M->m + q));
        predict_staged<T>(M, Q, q, M->psVec.as<T>(), (T*)nullptr);
        download(mean, M->psVec.p, sizeof(T) * q * M->m, s);
    }
    if (cov) {
        PhaseClock pc(M->ctx);
        const T sig = (T)M->sigma;
        joint_cov<T>(M, Q, q, qp, (flags & GPRX_POST_NOISE) ? sig * sig : T(0), pc);
        // the q x q block alone; with no padding it is one contiguous copy (a strided copy into
        // pageable memory goes column by column: 128 MiB at Q = 4096)
        if (qp == q) {
            launch_sym_fill<T>(M->psS.as<T>(), qp, q, s);
            download(cov, M->psS.p, sizeof(T) * q * q, s);
        } else {
            download_sym<T>(cov, M->psS, qp, q, s);
        }
    }
    return GPRX_OK;
}

template <typename T>
gprx_status model_sample(gprx_model* M, const void* Xq, int64_t q, int64_t nsamp, uint64_t seed, uint32_t flags,
                         const void* z, double* jitter, void* out) {
    require_joint(M, "gprx_model_sample");
    gprx_ctx* ctx = M->ctx;
    hipStream_t s = ctx->stream;
    const KCanon<T>& K = kcanon<T>(M);
    const int m = M->m;
    const int64_t qp = round_up(q, GT), ncols = nsamp * m, ncp = round_up(ncols, GT);
    Points<T> Q;
    stage_points<T>(Q, K, Xq, q, M->d, ctx->device, s, false, model_ell<T>(M));
    // every buffer before the first launch: a failed allocation leaves nothing half done
    M->pvRa.ensure(sizeof(T) * qp * M->np);
    M->psS.ensure(sizeof(T) * qp * qp);
    M->psL.ensure(sizeof(T) * qp * qp);
    M->psLinv.ensure(sizeof(T) * qp * DB);
    M->psVec.ensure(sizeof(T) * (q * m + q));
    M->psZ.ensure(sizeof(T) * ncols * q);
    M->psZp.ensure(sizeof(T) * ncp * qp);
    M->psOut.ensure(sizeof(T) * (qp * ncp + ncols * q));
    if (z) {  // the caller's normals in the generator's place (host or device memory)
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipMemcpy(M->psZ.p, z, sizeof(T) * ncols * q, hipMemcpyDefault));
    }
    T* dmean = M->psVec.as<T>();
    T* kqq = dmean + q * m;
    predict_staged<T>(M, Q, q, dmean, (T*)nullptr);
    // the prior diagonal's maximum: the scale of the jitter
    launch_pair_kernel<T>(K, Q.x, Q.x, q, M->d, kqq, s);
    std::vector<T> hk((size_t)q);
    download(hk.data(), kqq, sizeof(T) * q, s);
    double maxdiag = 0;
    for (T v : hk) maxdiag = std::max(maxdiag, (double)v);
    const bool automatic = !jitter || *jitter < 0;
    double j = automatic ? (double)q * (double)std::numeric_limits<T>::epsilon() * maxdiag : *jitter;
    const T sig = (T)M->sigma;
    const T noise = (flags & GPRX_POST_NOISE) ? sig * sig : T(0);

    launch_fit_status_init(M->info.as<int>(), M->flag.as<int>(), s);
    PhaseClock pc(ctx);  // marks: start, cross build, row solve, rank update, factor, normals, transform
    joint_cov<T>(M, Q, q, qp, noise + (T)j, pc);
    T* S = M->psS.as<T>();
    T* L = M->psL.as<T>();
    for (;;) {  // factor a copy; the unfactored block stays for the next, larger jitter
        GPRX_HIP(hipMemcpyAsync(L, S, sizeof(T) * qp * qp, hipMemcpyDeviceToDevice, s));
        potrf_tiles<T>(L, qp, qp, qp, M->psLinv.as<T>(), M->info.as<int>(), ctx->ex);
        int st[2];
        download(&st[0], M->flag.p, sizeof(int), s);
        download(&st[1], M->info.p, sizeof(int), s);
        check_finite(st[0]);
        check_sched(st[1]);
        if (st[1] == INT_MAX) break;
        const double jn = 10 * j;
        if (!automatic || !(jn > j) || !(jn <= 1e-2 * maxdiag))
            throw Error{GPRX_ERR_NOT_SPD, "gprx_model_sample: the joint covariance is not positive definite (jitter " +
                                              std::to_string(j) + ")"};
        launch_diag_fix<T>(S, qp, 0, q, q, (T)(jn - j), s);
        launch_fit_status_init(M->info.as<int>(), M->flag.as<int>(), s);
        j = jn;
    }
    pc.mark();
    if (jitter) *jitter = j;
    if (!z) launch_normals<T>(seed, ncols * q, M->psZ.as<T>(), s);
    launch_stage_normals<T>(M->psZ.as<T>(), ncols, q, M->psZp.as<T>(), ncp, qp, s);
    pc.mark();
    // C (qp x ncp) = Lq Zp^T, then the mean added on the way into the (nsamp, q, m) layout
    T* C = M->psOut.as<T>();
    T* dout = C + qp * ncp;
    launch_zero_upper<T>(L, qp, qp, s);
    launch_gemm_nt<T>(C, qp, L, qp, M->psZp.as<T>(), ncp, qp, ncp, qp, T(1), T(0), false, s);
    launch_sample_out<T>(C, qp, dmean, nsamp, q, m, dout, s);
    pc.mark();
    pc.read(M->psMs, 6);
    download(out, dout, sizeof(T) * ncols * q, s);
    return GPRX_OK;
}

// ---------------------------------------------------------------------------------------
// caller-evaluated kernels (k_hostk.hip): predict, posterior covariance and the LML gradient
// from the caller's kernel vectors / derivative matrices
// ---------------------------------------------------------------------------------------
template <typename T>
gprx_status model_predict_kx(gprx_model* M, const void* Kx, const void* Xq, int64_t q, void* mean, void* deriv) {
    GPRX_REQUIRE(M->has_alpha, GPRX_ERR_STATE, "GaussianProcess::ComputeKernelVectorInternal: gaussian process is not initialized.");
    GPRX_REQUIRE(!deriv || Xq, GPRX_ERR_ARG, "gprx_model_predict_kx: the derivative needs the query points");
    hipStream_t s = M->ctx->stream;
    const int d = M->d, m = M->m;
    const int64_t n = M->n;
    DevBuf dk, dq, dmean, dder;
    upload<T>(dk, Kx, sizeof(T) * q * n, s);
    if (deriv) {
        upload<T>(dq, Xq, sizeof(T) * q * d, s);
        dder.ensure(sizeof(T) * q * d * m);
    }
    dmean.ensure(sizeof(T) * q * m);
    launch_kx_predict<T>(dk.as<T>(), deriv ? dq.as<T>() : nullptr, M->X.as<T>(), q, n, d, M->alpha.as<T>(), m,
                         dmean.as<T>(), deriv ? dder.as<T>() : nullptr, s);
    download(mean, dmean.p, sizeof(T) * q * m, s);
    if (deriv) download(deriv, dder.p, sizeof(T) * q * d * m, s);
    return GPRX_OK;
}

template <typename T>
gprx_status model_posterior_cov_kx(gprx_model* M, const void* Kxa, const void* Kxb, const void* kab, int64_t q,
                                   void* out) {
    GPRX_REQUIRE(M->fitted, GPRX_ERR_STATE, "GaussianProcess::ComputeKernelVectorInternal: gaussian process is not initialized.");
    GPRX_REQUIRE(!M->dist_fitted, GPRX_ERR_STATE, "gprx: the posterior covariance needs a single-GPU fit");
    hipStream_t s = M->ctx->stream;
    const int64_t n = M->n, np = M->np, qp = round_up(q, GT);
    DevBuf dkab, res;
    upload<T>(dkab, kab, sizeof(T) * q, s);
    res.ensure(sizeof(T) * q);
    const T* ka = reinterpret_cast<const T*>(Kxa);
    const T* kb = reinterpret_cast<const T*>(Kxb);
    if (M->method == 1) {  // LU: k(x,y) - K(X,x)^T A^{-1} K(X,y) (lib/GaussianProcess.cpp:84-99)
        std::vector<double> ha((size_t)np * q, 0.0), hb((size_t)np * q, 0.0);  // np x q column-major
        for (int64_t j = 0; j < q; j++)
            for (int64_t i = 0; i < n; i++) {
                ha[(size_t)j * np + i] = (double)ka[j * n + i];
                hb[(size_t)j * np + i] = (double)kb[j * n + i];
            }
        DevBuf Wd, Kad;
        upload<double>(Wd, hb.data(), sizeof(double) * np * q, s);
        upload<double>(Kad, ha.data(), sizeof(double) * np * q, s);
        lu_solve_model(M, Wd.as<double>(), (int)q);
        lu_coldot<T>(Kad.as<double>(), Wd.as<double>(), np, n, q, dkab.as<T>(), res.as<T>(), s);
    } else {  // Cholesky: k(x,y) - (L^{-1} kx) . (L^{-1} ky), rows qp x np (ld qp)
        std::vector<T> ha((size_t)qp * np, T(0)), hb((size_t)qp * np, T(0));
        for (int64_t j = 0; j < q; j++)
            for (int64_t i = 0; i < n; i++) {
                ha[(size_t)i * qp + j] = ka[j * n + i];
                hb[(size_t)i * qp + j] = kb[j * n + i];
            }
        DevBuf Ra, Rb;
        upload<T>(Ra, ha.data(), sizeof(T) * qp * np, s);
        upload<T>(Rb, hb.data(), sizeof(T) * qp * np, s);
        trsm_rows<T>(M->A.as<T>(), M->ld, np, M->Linv.as<T>(), Ra.as<T>(), qp, qp, s);
        trsm_rows<T>(M->A.as<T>(), M->ld, np, M->Linv.as<T>(), Rb.as<T>(), qp, qp, s);
        launch_rowdot<T>(Ra.as<T>(), Rb.as<T>(), qp, q, np, dkab.as<T>(), res.as<T>(), s);
    }
    download(out, res.p, sizeof(T) * q, s);
    return GPRX_OK;
}

template <typename T>
gprx_status model_lml_dk(gprx_model* M, uint32_t flags, const void* dK, int32_t P, double* value, double* grad,
                         double* logdet) {
    GPRX_REQUIRE(P >= 0 && (P == 0 || dK), GPRX_ERR_ARG, "gprx_model_lml_dk: bad derivative matrices");
    gprx_status st = model_lml<T>(M, flags & ~GPRX_LML_GRAD, value, nullptr, nullptr, logdet);
    if (st != GPRX_OK || !grad || P == 0) return st;
    hipStream_t s = M->ctx->stream;
    const int64_t n = M->n, np = M->np;
    if (M->method == 1) lu_inverse_to_C<T>(M);
    else model_inverse<T>(M);
    DevBuf ddk, g;
    upload<T>(ddk, dK, sizeof(T) * (size_t)P * n * n, s);
    g.ensure(sizeof(double) * P);
    launch_dk_grad<T>(ddk.as<T>(), P, n, M->alpha.as<T>(), M->C.as<T>(), np, g.as<double>(), s);
    download(grad, g.p, sizeof(double) * P, s);
    return GPRX_OK;
}

#define GPRX_INST(T)                                                                                      \
    template gprx_status model_predict<T>(gprx_model*, const void*, int64_t, void*, void*);                \
    template gprx_status model_posterior_cov<T>(gprx_model*, const void*, const void*, int64_t, void*);    \
    template gprx_status model_core_matrix<T>(gprx_model*, void*);                                         \
    template gprx_status model_lml<T>(gprx_model*, uint32_t, double*, double*, int32_t*, double*);         \
    template gprx_status model_loo<T>(gprx_model*, uint32_t, double*, void*, void*, double*, int32_t*);    \
    template gprx_status model_lml_scale_grad<T>(gprx_model*, double*);                                    \
    template gprx_status model_posterior<T>(gprx_model*, const void*, int64_t, uint32_t, void*, void*);    \
    template gprx_status model_sample<T>(gprx_model*, const void*, int64_t, int64_t, uint64_t, uint32_t,   \
                                         const void*, double*, void*);                                     \
    template gprx_status model_predict_kx<T>(gprx_model*, const void*, const void*, int64_t, void*, void*); \
    template gprx_status model_posterior_cov_kx<T>(gprx_model*, const void*, const void*, const void*,     \
                                                   int64_t, void*);                                        \
    template gprx_status model_lml_dk<T>(gprx_model*, uint32_t, const void*, int32_t, double*, double*, double*);
GPRX_INST(float)
GPRX_INST(double)
#undef GPRX_INST

}  // namespace gprx
