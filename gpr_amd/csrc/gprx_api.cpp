// gprx_api.cpp — the C ABI of libgprx (include/gprx.h): argument checks, locks and dispatch to
// the host layer (gprx_fit / _query / _matrix / _sparse .cpp).  No entry point throws across the ABI.
#include "gprx_model.h"

namespace gprx {

static thread_local std::string t_last_error;
thread_local Prof* g_prof = nullptr;

gprx_status fail(gprx_ctx* ctx, gprx_status st, const std::string& msg) {
    t_last_error = msg;
    if (ctx) ctx->err = msg;
    return st;
}

// Exec is host-only state of the context that owns it: the tile factorisation's cached
// schedules and the device ints the chained launches use as counters and flags.
Exec::~Exec() {
    pt_state_free(pt);
    if (scratch) (void)hipFree(scratch);
}

int* Exec::scratch_ints(size_t n) {
    if (n > scratch_n) {
        if (scratch) GPRX_HIP(hipFree(scratch));
        scratch = nullptr;
        GPRX_HIP(dev_malloc(&scratch, sizeof(int) * n));
        scratch_n = n;
    }
    return scratch;
}

}  // namespace gprx

using namespace gprx;

// The prologue of a model entry point, in the order every one of them keeps: the NULL check
// (`args_ok` with the function's own message), `pre` (checks that run before the lock; true = there
// is nothing to do), the context's and the model's locks, the profiler binding (CALL_PROF; after
// the lock: resolved, the stream drained, before it is released), hipSetDevice (CALL_DEVICE), `body`.
// An entry point whose state checks come between the lock and the device selection selects the
// device in its body; fit and append select it in model_fit / model_append.
enum : unsigned { CALL_PROF = 1, CALL_DEVICE = 2 };

template <typename Pre, typename Body>
static gprx_status model_call(gprx_model* M, bool args_ok, const char* null_msg, unsigned opts, Pre&& pre, Body&& body) {
    gprx_ctx* ctx = M ? M->ctx : nullptr;
    API_BEGIN
    GPRX_REQUIRE(M && args_ok, GPRX_ERR_ARG, null_msg);
    if (pre()) return GPRX_OK;
    ModelLock lk(M);
    std::optional<ProfBind> pb;
    if (opts & CALL_PROF) pb.emplace(ctx);
    if (opts & CALL_DEVICE) GPRX_HIP(hipSetDevice(ctx->device));
    return body();
    API_END(ctx)
}

template <typename Body>
static gprx_status model_call(gprx_model* M, bool args_ok, const char* null_msg, unsigned opts, Body&& body) {
    return model_call(M, args_ok, null_msg, opts, [] { return false; }, body);
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int gprx_abi_version(void) { return GPRX_ABI_VERSION; }

gprx_status gprx_device_count(int* count) {
    API_BEGIN
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    if (count) *count = c;
    return GPRX_OK;
    API_END(nullptr)
}

static gprx_ctx* ctx_new(int device) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
        throw Error{GPRX_ERR_NO_DEVICE, "gprx_ctx_create: no HIP device visible (libgprx has no CPU fallback)"};
    GPRX_REQUIRE(device >= 0 && device < c, GPRX_ERR_ARG, "gprx_ctx_create: bad device index");
    GPRX_HIP(hipSetDevice(device));
    gprx_ctx* ctx = new gprx_ctx();
    ctx->device = device;
    // The context's one stream carries every launch of a call in order: the persistent tile
    // factorisation, the chained solves, the GEMMs and the reductions.  It has the highest
    // priority, so its kernels are dispatched ahead of other work on the device.
    int prio_lo = 0, prio_hi = 0;
    GPRX_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    GPRX_HIP(hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_hi));
    ctx->ex.s0 = ctx->stream;
    for (auto& e : ctx->ev) GPRX_HIP(hipEventCreate(&e));
    return ctx;
}

gprx_status gprx_ctx_create(int device, gprx_ctx** out) {
    API_BEGIN
    GPRX_REQUIRE(out, GPRX_ERR_ARG, "gprx_ctx_create: out is NULL");
    *out = ctx_new(device);
    return GPRX_OK;
    API_END(nullptr)
}

void gprx_ctx_destroy(gprx_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (auto& e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx->hc;
    // abort, not destroy: local, never waits on the peers (a communicator whose collective
    // timed out, or whose peers already left, would block ncclCommDestroy); every stream of
    // this context has drained by now
    if (ctx->comm) (void)ncclCommAbort(ctx->comm);
    delete ctx;
}

const char* gprx_last_error(const gprx_ctx* ctx) { return ctx ? ctx->err.c_str() : t_last_error.c_str(); }

gprx_status gprx_model_create(gprx_ctx* ctx, gprx_dtype dtype, gprx_model** out) {
    API_BEGIN
    GPRX_REQUIRE(ctx && out, GPRX_ERR_ARG, "gprx_model_create: NULL argument");
    GPRX_REQUIRE(dtype == GPRX_F32 || dtype == GPRX_F64, GPRX_ERR_ARG, "gprx_model_create: bad dtype");
    gprx_model* m = new gprx_model();
    m->ctx = ctx;
    m->dt = dtype;
    *out = m;
    return GPRX_OK;
    API_END(ctx)
}

void gprx_model_destroy(gprx_model* model) {
    if (!model) return;
    (void)hipSetDevice(model->ctx->device);
    delete model;
}

gprx_status gprx_model_set_data(gprx_model* M, const void* X, const void* Y, int64_t n, int32_t d, int32_t m) {
    return model_call(
        M, X && Y, "gprx_model_set_data: NULL argument", CALL_DEVICE,
        [&] {
            GPRX_REQUIRE(n > 0, GPRX_ERR_STATE, "GaussianProcess::Initialize: no input samples defined during initialization");
            GPRX_REQUIRE(d > 0 && m > 0, GPRX_ERR_DIM, "gprx_model_set_data: input and output dimensions must be positive");
            return false;
        },
        [&] {
            GPRX_REQUIRE(!M->scaled() || (int32_t)M->ell.size() == d, GPRX_ERR_DIM,
                         "gprx_model_set_data: the input dimension differs from the number of length scales set");
            const size_t es = esize(M->dt);
            M->X.ensure(es * n * d);
            M->Y.ensure(es * n * m);
            if (M->scaled()) M->Xraw.ensure(es * n * d);
            M->trim_posterior_workspace();
            // host or device memory (include/gprx.h conventions: a gprx_device_alloc pointer too)
            GPRX_HIP(hipMemcpy(M->scaled() ? M->Xraw.p : M->X.p, X, es * n * d, hipMemcpyDefault));
            GPRX_HIP(hipMemcpy(M->Y.p, Y, es * n * m, hipMemcpyDefault));
            M->n = n;
            M->d = d;
            M->m = m;
            if (M->scaled()) {  // X = the scaled points, Xraw = the points as uploaded
                by_dtype(M->dt, [&](auto t) { scale_model_rows<decltype(t)>(M, 0, n); });
                GPRX_HIP(hipStreamSynchronize(M->ctx->stream));
            }
            M->has_data = true;
            M->drop_sparse_cov();
            M->drop_fit();
            return GPRX_OK;
        });
}

gprx_status gprx_model_set_kernel(gprx_model* M, const gprx_kernel_desc* k) {
    return model_call(M, k, "gprx_model_set_kernel: NULL argument", 0, [&] {
        std::string e = by_dtype(M->dt, [&](auto t) { return canonicalize(*k, kcanon<decltype(t)>(M)); });
        GPRX_REQUIRE(e.empty(), GPRX_ERR_ARG, e);
        if (M->dt == GPRX_F32) {  // the fp64 form of the fp32 tree (its parameters rounded to float)
            gprx_kernel_desc k32 = *k;
            for (int i = 0; i < k32.n_nodes && i < GPRX_MAX_KNODES; i++)
                for (int q = 0; q < 3; q++) k32.node[i].p[q] = (double)(float)k32.node[i].p[q];
            e = canonicalize<double>(k32, M->kd);
            GPRX_REQUIRE(e.empty(), GPRX_ERR_ARG, e);
        }
        M->desc = *k;
        M->has_kernel = true;
        M->host_k = false;
        M->drop_sparse_cov();  // W belongs to the kernel it was computed with (set_sparse_cov comes after set_kernel)
        M->drop_fit();
        return GPRX_OK;
    });
}

gprx_status gprx_model_set_noise(gprx_model* M, double sigma) {
    return model_call(M, true, "gprx_model_set_noise: NULL model", 0, [&] {
        M->sigma = sigma;
        M->drop_fit();
        return GPRX_OK;
    });
}

gprx_status gprx_model_set_length_scales(gprx_model* M, const double* ell, int32_t d) {
    return model_call(M, d >= 0, "gprx_model_set_length_scales: NULL model or negative d", CALL_DEVICE, [&] {
        const bool clear = !ell || d == 0;
        if (!clear) {
            for (int j = 0; j < d; j++)
                GPRX_REQUIRE(std::isfinite(ell[j]) && ell[j] > 0 &&
                                 (M->dt == GPRX_F64 || (std::isfinite((float)ell[j]) && (float)ell[j] > 0)),
                             GPRX_ERR_ARG, "gprx_model_set_length_scales: every length scale must be finite and > 0");
            GPRX_REQUIRE(!M->has_data || d == M->d, GPRX_ERR_DIM,
                         "gprx_model_set_length_scales: the number of length scales differs from the input dimension");
            GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE,
                         "gprx_model_set_length_scales: a caller-evaluated kernel owns its own metric");
        }
        if (clear && !M->scaled()) return GPRX_OK;  // (nothing set, nothing to clear: the fit stays)
        hipStream_t s = M->ctx->stream;
        const size_t es = esize(M->dt);
        const size_t xb = M->has_data ? es * M->n * M->d : 0;
        GPRX_HIP(hipStreamSynchronize(s));
        // Xraw = the points as uploaded, whichever way the model goes
        if (!M->scaled() && xb) {
            M->Xraw.ensure(xb);
            GPRX_HIP(hipMemcpy(M->Xraw.p, M->X.p, xb, hipMemcpyDeviceToDevice));
        }
        if (clear) {
            if (xb) GPRX_HIP(hipMemcpy(M->X.p, M->Xraw.p, xb, hipMemcpyDeviceToDevice));
            M->ell.clear();
            M->Xraw.release();
            M->rmXraw.release();
        } else {
            M->ell.assign(ell, ell + d);
            M->ellT.ensure(es * d);
            if (M->dt == GPRX_F64) {
                GPRX_HIP(hipMemcpy(M->ellT.p, ell, sizeof(double) * d, hipMemcpyHostToDevice));
            } else {
                std::vector<float> ef(ell, ell + d);  // narrowed to T first
                GPRX_HIP(hipMemcpy(M->ellT.p, ef.data(), sizeof(float) * d, hipMemcpyHostToDevice));
            }
            if (xb) {
                by_dtype(M->dt, [&](auto t) { scale_model_rows<decltype(t)>(M, 0, M->n); });
                GPRX_HIP(hipStreamSynchronize(s));
            }
        }
        M->drop_sparse_cov();
        M->drop_fit();
        return GPRX_OK;
    });
}

gprx_status gprx_model_lml_scale_grad(gprx_model* M, double* grad_ell) {
    return model_call(M, grad_ell, "gprx_model_lml_scale_grad: NULL argument", CALL_PROF | CALL_DEVICE, [&] {
        return by_dtype(M->dt, [&](auto t) { return model_lml_scale_grad<decltype(t)>(M, grad_ell); });
    });
}

gprx_status gprx_model_fit(gprx_model* M, uint32_t flags, gprx_fit_info* info) {
    return model_call(M, true, "gprx_model_fit: NULL model", CALL_PROF, [&] {
        return by_dtype(M->dt, [&](auto t) { return model_fit<decltype(t)>(M, flags, info); });
    });
}

gprx_status gprx_model_append(gprx_model* M, const void* Xnew, const void* Ynew, int64_t k, uint32_t flags,
                              gprx_fit_info* info) {
    return model_call(
        M, true, "gprx_model_append: NULL model", CALL_PROF,
        [&] {
            GPRX_REQUIRE(!((M->ctx->hc && M->ctx->world > 1) || M->ctx->virt), GPRX_ERR_STATE,
                         "gprx_model_append: sharded contexts (multi-rank or virtual-rank) refit in full: use "
                         "gprx_model_set_data and gprx_model_fit");
            GPRX_REQUIRE(Xnew && Ynew, GPRX_ERR_ARG, "gprx_model_append: NULL argument");
            GPRX_REQUIRE(k > 0, GPRX_ERR_ARG, "gprx_model_append: the number of new samples must be positive");
            return false;
        },
        [&] {
            GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE,
                         "gprx_model_append: a caller-evaluated kernel has no device form to extend the factor with");
            GPRX_REQUIRE(!M->sparse_cov, GPRX_ERR_STATE, "gprx_model_append: a sparse-covariance model holds no factor");
            GPRX_REQUIRE(M->fitted && M->has_data && M->has_kernel, GPRX_ERR_STATE,
                         "GaussianProcess::AddSample: gaussian process is not initialized.");
            return by_dtype(M->dt, [&](auto t) { return model_append<decltype(t)>(M, Xnew, Ynew, k, flags, info); });
        });
}

gprx_status gprx_model_remove(gprx_model* M, int64_t first, int64_t count, uint32_t flags, gprx_fit_info* info) {
    return model_call(
        M, true, "gprx_model_remove: NULL model", CALL_PROF,
        [&] {
            GPRX_REQUIRE(!((M->ctx->hc && M->ctx->world > 1) || M->ctx->virt), GPRX_ERR_STATE,
                         "gprx_model_remove: sharded contexts (multi-rank or virtual-rank) refit in full: use "
                         "gprx_model_set_data and gprx_model_fit");
            return false;
        },
        [&] {
            GPRX_REQUIRE(!M->host_k, GPRX_ERR_STATE,
                         "gprx_model_remove: a caller-evaluated kernel matrix would have to be reduced by the caller");
            GPRX_REQUIRE(!M->sparse_cov, GPRX_ERR_STATE, "gprx_model_remove: a sparse-covariance model holds no factor");
            GPRX_REQUIRE(M->fitted && M->has_data && M->has_kernel, GPRX_ERR_STATE,
                         "gprx_model_remove: gaussian process is not initialized.");
            GPRX_REQUIRE(!M->dist_fitted, GPRX_ERR_STATE, "gprx_model_remove: the model was fitted sharded");
            GPRX_REQUIRE(first >= 0 && count >= 1 && first <= M->n - count, GPRX_ERR_DIM,
                         "gprx_model_remove: the samples [first, first + count) must lie inside the model's");
            GPRX_REQUIRE(count < M->n, GPRX_ERR_DIM, "gprx_model_remove: no sample would be left");
            return by_dtype(M->dt, [&](auto t) { return model_remove<decltype(t)>(M, first, count, flags, info); });
        });
}

gprx_status gprx_model_get_alpha(gprx_model* M, void* alpha) {
    return model_call(M, alpha, "gprx_model_get_alpha: NULL argument", 0, [&] {
        GPRX_REQUIRE(M->has_alpha, GPRX_ERR_STATE, "gprx: model is not fitted");
        GPRX_HIP(hipSetDevice(M->ctx->device));
        GPRX_HIP(hipMemcpy(alpha, M->alpha.p, esize(M->dt) * M->n * M->m, hipMemcpyDeviceToHost));
        return GPRX_OK;
    });
}

gprx_status gprx_model_set_alpha(gprx_model* M, const void* alpha) {
    return model_call(M, alpha, "gprx_model_set_alpha: NULL argument", 0, [&] {
        GPRX_REQUIRE(M->has_data && M->has_kernel, GPRX_ERR_STATE, "gprx_model_set_alpha: set data and kernel first");
        hipStream_t s = M->ctx->stream;
        GPRX_HIP(hipSetDevice(M->ctx->device));
        const size_t es = esize(M->dt);
        M->alpha.ensure(es * M->n * M->m);
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipMemcpy(M->alpha.p, alpha, es * M->n * M->m, hipMemcpyHostToDevice));
        if (by_dtype(M->dt, [&](auto t) { return ensure_train_tables<decltype(t)>(M); }))
            GPRX_HIP(hipStreamSynchronize(s));
        M->alpha_loaded();  // the factor (if any) is left as it is
        return GPRX_OK;
    });
}

gprx_status gprx_model_predict(gprx_model* M, const void* Xq, int64_t q, void* mean, void* deriv) {
    return model_call(
        M, Xq && mean, "gprx_model_predict: NULL argument", CALL_PROF | CALL_DEVICE, [&] { return q == 0; },
        [&] { return by_dtype(M->dt, [&](auto t) { return model_predict<decltype(t)>(M, Xq, q, mean, deriv); }); });
}

gprx_status gprx_model_posterior_cov(gprx_model* M, const void* Xa, const void* Xb, int64_t q, void* out) {
    return model_call(
        M, q >= 0, "gprx_model_posterior_cov: NULL model or negative q", CALL_PROF | CALL_DEVICE,
        [&] {
            // on a sharded fit of a multi-process context this is a collective call (gprx.h): a process
            // with no pairs of its own still takes part
            const bool collective = M->dist_fitted && M->ctx->hc && M->ctx->world > 1;
            if (q == 0 && !collective) return true;
            GPRX_REQUIRE(q == 0 || (Xa && Xb && out), GPRX_ERR_ARG, "gprx_model_posterior_cov: NULL argument");
            return false;
        },
        [&] { return by_dtype(M->dt, [&](auto t) { return model_posterior_cov<decltype(t)>(M, Xa, Xb, q, out); }); });
}

gprx_status gprx_model_core_matrix(gprx_model* M, void* C) {
    return model_call(M, C, "gprx_model_core_matrix: NULL argument", CALL_PROF | CALL_DEVICE, [&] {
        return by_dtype(M->dt, [&](auto t) { return model_core_matrix<decltype(t)>(M, C); });
    });
}

gprx_status gprx_model_lml(gprx_model* M, uint32_t flags, double* value, double* grad, int32_t* nparams,
                           double* logdet) {
    return model_call(M, true, "gprx_model_lml: NULL model", CALL_PROF | CALL_DEVICE, [&] {
        return by_dtype(M->dt, [&](auto t) { return model_lml<decltype(t)>(M, flags, value, grad, nparams, logdet); });
    });
}

gprx_status gprx_model_loo(gprx_model* M, uint32_t flags, double* value, void* mean, void* var, double* grad,
                           int32_t* nparams) {
    return model_call(M, true, "gprx_model_loo: NULL model", CALL_PROF | CALL_DEVICE, [&] {
        GPRX_REQUIRE(M->fitted || (M->has_data && M->has_kernel), GPRX_ERR_STATE,
                     "gprx_model_loo: set the data, the kernel and the noise first");
        return by_dtype(M->dt, [&](auto t) { return model_loo<decltype(t)>(M, flags, value, mean, var, grad, nparams); });
    });
}

gprx_status gprx_model_posterior(gprx_model* M, const void* Xq, int64_t q, uint32_t flags, void* mean, void* cov) {
    return model_call(
        M, q >= 0, "gprx_model_posterior: NULL model or negative q", CALL_PROF | CALL_DEVICE,
        [&] {
            if (q == 0) return true;
            GPRX_REQUIRE(Xq, GPRX_ERR_ARG, "gprx_model_posterior: NULL argument");
            return false;
        },
        [&] { return by_dtype(M->dt, [&](auto t) { return model_posterior<decltype(t)>(M, Xq, q, flags, mean, cov); }); });
}

gprx_status gprx_model_sample(gprx_model* M, const void* Xq, int64_t q, int64_t nsamp, uint64_t seed, uint32_t flags,
                              const void* z, double* jitter, void* out) {
    return model_call(
        M, q >= 0 && nsamp >= 0, "gprx_model_sample: NULL model or a negative count", CALL_PROF | CALL_DEVICE,
        [&] {
            if (q == 0 || nsamp == 0) return true;
            GPRX_REQUIRE(Xq && out, GPRX_ERR_ARG, "gprx_model_sample: NULL argument");
            return false;
        },
        [&] {
            return by_dtype(M->dt, [&](auto t) {
                return model_sample<decltype(t)>(M, Xq, q, nsamp, seed, flags, z, jitter, out);
            });
        });
}

gprx_status gprx_model_set_sparse_cov(gprx_model* M, const void* W) {
    return model_call(M, W, "gprx_model_set_sparse_cov: NULL argument", 0, [&] {
        GPRX_REQUIRE(M->has_data && M->has_kernel && !M->host_k, GPRX_ERR_STATE,
                     "gprx_model_set_sparse_cov: set the inducing points and the kernel first");
        hipStream_t s = M->ctx->stream;
        GPRX_HIP(hipSetDevice(M->ctx->device));
        const int64_t n = M->n, Mp = round_up(n, GT);
        const size_t es = esize(M->dt);
        std::vector<unsigned char> h(es * Mp * Mp, 0);  // padded, column-major
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = 0; j < n; j++)
                std::memcpy(&h[es * (i + j * Mp)], static_cast<const unsigned char*>(W) + es * (i * n + j), es);
        M->sparseW.ensure(h.size());
        GPRX_HIP(hipStreamSynchronize(s));
        GPRX_HIP(hipMemcpy(M->sparseW.p, h.data(), h.size(), hipMemcpyHostToDevice));
        by_dtype(M->dt, [&](auto t) { return ensure_train_tables<decltype(t)>(M); });  // the inducing points' tables
        M->flag.ensure(sizeof(int));
        GPRX_HIP(hipMemsetAsync(M->flag.p, 0, sizeof(int), s));
        GPRX_HIP(hipStreamSynchronize(s));
        M->sparse_cov_loaded();
        return GPRX_OK;
    });
}

gprx_status gprx_model_set_kernel_matrix(gprx_model* M, const void* K) {
    return model_call(M, K, "gprx_model_set_kernel_matrix: NULL argument", 0, [&] {
        GPRX_REQUIRE(M->has_data, GPRX_ERR_STATE, "gprx_model_set_kernel_matrix: set the data first");
        GPRX_REQUIRE(!M->scaled(), GPRX_ERR_STATE,
                     "gprx_model_set_kernel_matrix: the model has length scales set (a caller-evaluated kernel owns "
                     "its own metric: clear them first)");
        GPRX_HIP(hipSetDevice(M->ctx->device));
        const size_t es = esize(M->dt);
        M->Kext.ensure(es * M->n * M->n);
        GPRX_HIP(hipStreamSynchronize(M->ctx->stream));
        GPRX_HIP(hipMemcpy(M->Kext.p, K, es * M->n * M->n, hipMemcpyHostToDevice));
        std::memset(&M->kd, 0, sizeof(M->kd));  // no device form: nothing else reads the tree
        std::memset(&M->kf, 0, sizeof(M->kf));
        std::memset(&M->desc, 0, sizeof(M->desc));
        M->host_k = true;
        M->has_kernel = true;
        M->drop_sparse_cov();
        M->drop_fit();
        return GPRX_OK;
    });
}

gprx_status gprx_model_predict_kx(gprx_model* M, const void* Kx, const void* Xq, int64_t q, void* mean, void* deriv) {
    return model_call(
        M, Kx && mean, "gprx_model_predict_kx: NULL argument", CALL_DEVICE, [&] { return q == 0; },
        [&] { return by_dtype(M->dt, [&](auto t) { return model_predict_kx<decltype(t)>(M, Kx, Xq, q, mean, deriv); }); });
}

gprx_status gprx_model_posterior_cov_kx(gprx_model* M, const void* Kxa, const void* Kxb, const void* kab, int64_t q,
                                        void* out) {
    return model_call(
        M, Kxa && Kxb && kab && out, "gprx_model_posterior_cov_kx: NULL argument", CALL_DEVICE, [&] { return q == 0; },
        [&] {
            return by_dtype(M->dt, [&](auto t) { return model_posterior_cov_kx<decltype(t)>(M, Kxa, Kxb, kab, q, out); });
        });
}

gprx_status gprx_model_lml_dk(gprx_model* M, uint32_t flags, const void* dK, int32_t P, double* value, double* grad,
                              double* logdet) {
    return model_call(M, true, "gprx_model_lml_dk: NULL model", CALL_PROF | CALL_DEVICE, [&] {
        return by_dtype(M->dt, [&](auto t) { return model_lml_dk<decltype(t)>(M, flags, dK, P, value, grad, logdet); });
    });
}

gprx_status gprx_kernel_matrix(gprx_ctx* ctx, gprx_dtype dt, const gprx_kernel_desc* k, const void* X, int64_t n,
                               int32_t d, void* K) {
    API_BEGIN
    GPRX_REQUIRE(ctx && k && X && K, GPRX_ERR_ARG, "gprx_kernel_matrix: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);  // after the lock: resolved (streams drained) before it is released
    GPRX_HIP(hipSetDevice(ctx->device));
    return by_dtype(dt, [&](auto t) { return kernel_matrix_impl<decltype(t)>(ctx, k, X, n, d, K, false); });
    API_END(ctx)
}

gprx_status gprx_deriv_matrix(gprx_ctx* ctx, gprx_dtype dt, const gprx_kernel_desc* k, const void* X, int64_t n,
                              int32_t d, void* D) {
    API_BEGIN
    GPRX_REQUIRE(ctx && k && X && D, GPRX_ERR_ARG, "gprx_deriv_matrix: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);  // after the lock: resolved (streams drained) before it is released
    GPRX_HIP(hipSetDevice(ctx->device));
    return by_dtype(dt, [&](auto t) { return kernel_matrix_impl<decltype(t)>(ctx, k, X, n, d, D, true); });
    API_END(ctx)
}

gprx_status gprx_cross_matrix(gprx_ctx* ctx, gprx_dtype dt, const gprx_kernel_desc* k, const void* A, int64_t na,
                              const void* B, int64_t nb, int32_t d, void* K) {
    API_BEGIN
    GPRX_REQUIRE(ctx && k && A && B && K, GPRX_ERR_ARG, "gprx_cross_matrix: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);  // after the lock: resolved (streams drained) before it is released
    GPRX_HIP(hipSetDevice(ctx->device));
    return by_dtype(dt, [&](auto t) { return cross_matrix_impl<decltype(t)>(ctx, k, A, na, B, nb, d, K); });
    API_END(ctx)
}

gprx_status gprx_cholesky(gprx_ctx* ctx, gprx_dtype dt, void* A, int64_t n, int32_t* info) {
    API_BEGIN
    GPRX_REQUIRE(ctx && A && n > 0, GPRX_ERR_ARG, "gprx_cholesky: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);  // after the lock: resolved (streams drained) before it is released
    GPRX_HIP(hipSetDevice(ctx->device));
    gprx_status st = by_dtype(dt, [&](auto t) { return cholesky_impl<decltype(t)>(ctx, A, n, info, false); });
    if (st == GPRX_ERR_NOT_SPD) return fail(ctx, st, "gprx_cholesky: matrix is not positive definite");
    return st;
    API_END(ctx)
}

gprx_status gprx_spd_inverse(gprx_ctx* ctx, gprx_dtype dt, void* A, int64_t n, int32_t* info) {
    API_BEGIN
    GPRX_REQUIRE(ctx && A && n > 0, GPRX_ERR_ARG, "gprx_spd_inverse: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);  // after the lock: resolved (streams drained) before it is released
    GPRX_HIP(hipSetDevice(ctx->device));
    return by_dtype(dt, [&](auto t) { return cholesky_impl<decltype(t)>(ctx, A, n, info, true); });
    API_END(ctx)
}

static const char* kclass_name(int c) {
    static const char* names[KC_COUNT] = {"kbuild", "potrf_diag", "potrf_trsm", "potrf_update", "backsolve",
                                          "predict", "lml_grad", "spd_inverse", "other_gemm", "potrf_tiles",
                                          "posterior"};
    return names[c];
}

gprx_status gprx_ctx_set_stats(gprx_ctx* ctx, int32_t enable) {
    API_BEGIN
    GPRX_REQUIRE(ctx, GPRX_ERR_ARG, "gprx_ctx_set_stats: NULL ctx");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->prof.on = enable != 0;
    ctx->prof.reset();
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_device_alloc(gprx_ctx* ctx, int64_t bytes, void** out) {
    API_BEGIN
    GPRX_REQUIRE(ctx && out && bytes >= 0, GPRX_ERR_ARG, "gprx_device_alloc: NULL argument or negative size");
    *out = nullptr;
    if (bytes == 0) return GPRX_OK;
    void* p = nullptr;
    GPRX_HIP(hipSetDevice(ctx->device));
    const hipError_t e = dev_malloc(&p, (size_t)bytes);
    if (e != hipSuccess)
        throw Error{GPRX_ERR_OOM, std::string("gprx_device_alloc: hipMalloc: ") + hipGetErrorString(e)};
    *out = p;
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_device_free(gprx_ctx* ctx, void* p) {
    API_BEGIN
    GPRX_REQUIRE(ctx, GPRX_ERR_ARG, "gprx_device_free: NULL ctx");
    if (p) {
        GPRX_HIP(hipStreamSynchronize(ctx->stream));  // (no launch may still read it)
        GPRX_HIP(hipFree(p));
    }
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_device_upload(gprx_ctx* ctx, void* dst, const void* src, int64_t bytes) {
    API_BEGIN
    GPRX_REQUIRE(ctx && (bytes == 0 || (dst && src)) && bytes >= 0, GPRX_ERR_ARG, "gprx_device_upload: bad argument");
    if (bytes > 0) {
        GPRX_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
        GPRX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_device_download(gprx_ctx* ctx, void* dst, const void* src, int64_t bytes) {
    API_BEGIN
    GPRX_REQUIRE(ctx && (bytes == 0 || (dst && src)) && bytes >= 0, GPRX_ERR_ARG, "gprx_device_download: bad argument");
    if (bytes > 0) {
        GPRX_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
        GPRX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_ctx_get_stats(gprx_ctx* ctx, gprx_kstat* out, int32_t max, int32_t* count) {
    API_BEGIN
    GPRX_REQUIRE(ctx, GPRX_ERR_ARG, "gprx_ctx_get_stats: NULL ctx");
    std::lock_guard<std::mutex> lk(ctx->mu);
    int k = 0;
    for (int c = 0; c < KC_COUNT; c++) {
        const Prof::Acc& a = ctx->prof.acc[c];
        if (a.launches == 0) continue;
        if (out && k < max) {
            std::memset(&out[k], 0, sizeof(gprx_kstat));
            std::strncpy(out[k].name, kclass_name(c), sizeof(out[k].name) - 1);
            out[k].launches = a.launches;
            out[k].ms = a.ms;
            out[k].flops = a.flops;
            out[k].bytes = a.bytes;
        }
        k++;
    }
    if (count) *count = k;
    return GPRX_OK;
    API_END(ctx)
}


gprx_status gprx_dev_bench(gprx_ctx* ctx, gprx_dtype dtype, int32_t what, int64_t M, int64_t N, int64_t K,
                           int32_t iters, double* ms) {
    API_BEGIN
    GPRX_REQUIRE(ctx && ms && iters > 0, GPRX_ERR_ARG, "gprx_dev_bench: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPRX_HIP(hipSetDevice(ctx->device));
    gprx_status st = gprx_dev_bench_impl(dtype, what, M, N, K, iters, ms, &ctx->ex);
    if (st != GPRX_OK) return fail(ctx, st, "gprx_dev_bench failed");
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_dev_forward_panel(gprx_ctx* ctx, gprx_dtype dtype, const void* L, int64_t n, void* R, int32_t rows,
                                   int32_t use_gemm) {
    API_BEGIN
    GPRX_REQUIRE(ctx, GPRX_ERR_ARG, "gprx_dev_forward_panel: NULL context");
    GPRX_REQUIRE(dtype == GPRX_F32 || dtype == GPRX_F64, GPRX_ERR_ARG, "gprx_dev_forward_panel: bad dtype");
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPRX_HIP(hipSetDevice(ctx->device));
    return gprx_dev_forward_panel_impl(dtype, L, n, R, rows, use_gemm, &ctx->ex, ctx->stream);
    API_END(ctx)
}

gprx_status gprx_dev_factor_update(gprx_ctx* ctx, gprx_dtype dtype, const void* L, int64_t n, const void* X, int32_t r,
                                   void* Lout, void* LinvOut) {
    API_BEGIN
    GPRX_REQUIRE(ctx, GPRX_ERR_ARG, "gprx_dev_factor_update: NULL context");
    GPRX_REQUIRE(dtype == GPRX_F32 || dtype == GPRX_F64, GPRX_ERR_ARG, "gprx_dev_factor_update: bad dtype");
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPRX_HIP(hipSetDevice(ctx->device));
    return gprx_dev_factor_update_impl(dtype, L, n, X, r, Lout, LinvOut, &ctx->ex, ctx->stream);
    API_END(ctx)
}

int32_t gprx_dev_factor_update_width(void) { return factor_update_width(); }

gprx_status gprx_dev_normals(gprx_ctx* ctx, gprx_dtype dtype, uint64_t seed, int64_t count, void* out_host) {
    API_BEGIN
    GPRX_REQUIRE(ctx && count >= 0 && (count == 0 || out_host), GPRX_ERR_ARG, "gprx_dev_normals: bad argument");
    GPRX_REQUIRE(dtype == GPRX_F32 || dtype == GPRX_F64, GPRX_ERR_ARG, "gprx_dev_normals: bad dtype");
    if (count == 0) return GPRX_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    GPRX_HIP(hipSetDevice(ctx->device));
    DevBuf z;
    z.ensure(esize(dtype) * count);
    by_dtype(dtype, [&](auto t) { launch_normals<decltype(t)>(seed, count, z.as<decltype(t)>(), ctx->stream); });
    download(out_host, z.p, esize(dtype) * count, ctx->stream);
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_dev_sample_phases(gprx_model* M, double* ms) {
    return model_call(M, ms, "gprx_dev_sample_phases: NULL argument", 0, [&] {
        std::memcpy(ms, M->psMs, sizeof(M->psMs));
        return GPRX_OK;
    });
}

gprx_status gprx_dev_build_matrix(gprx_ctx* ctx, gprx_dtype dt, const gprx_kernel_desc* k, const void* X, int64_t n,
                                  int32_t d, double sigma, int32_t path, void* K) {
    API_BEGIN
    GPRX_REQUIRE(ctx && k && X && K, GPRX_ERR_ARG, "gprx_dev_build_matrix: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);
    GPRX_HIP(hipSetDevice(ctx->device));
    return by_dtype(dt, [&](auto t) { return dev_build_impl<decltype(t)>(ctx, k, X, n, d, sigma, path, K); });
    API_END(ctx)
}

gprx_status gprx_dev_build_time(gprx_ctx* ctx, gprx_dtype dt, const gprx_kernel_desc* k, const void* X, int64_t n,
                                int32_t d, double sigma, int32_t path, int32_t iters, double* ms) {
    API_BEGIN
    GPRX_REQUIRE(ctx && k && X && ms && iters > 0, GPRX_ERR_ARG, "gprx_dev_build_time: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);
    GPRX_HIP(hipSetDevice(ctx->device));
    return by_dtype(dt, [&](auto t) {
        return dev_build_impl<decltype(t)>(ctx, k, X, n, d, sigma, path, nullptr, iters, ms);
    });
    API_END(ctx)
}

gprx_status gprx_dev_dist_info(gprx_model* M, int64_t* out, int32_t nout) {
    API_BEGIN
    GPRX_REQUIRE(M && out, GPRX_ERR_ARG, "gprx_dev_dist_info: NULL argument");
    GPRX_REQUIRE(M->dist_fitted || M->dist_stats.bytes_rank > 0, GPRX_ERR_STATE,
                 "gprx_dev_dist_info: no distributed fit on this model");
    const DistFitOut& o = M->dist_stats;
    const int64_t v[15] = {o.bytes_rank, o.bytes_storage, o.gb, o.ww, o.chunk_w, o.P, (int64_t)o.est_us,
                           M->ctx->world, M->dist_dense ? 1 : 0,
                           M->dist_engine ? dist_pvar_chunks(M->dist_engine) : 0,
                           M->dist_engine ? dist_pvar_bytes(M->dist_engine) : 0,
                           o.push_linv, o.push_tiles, o.push_bytes, o.push_rank};
    for (int i = 0; i < std::min<int32_t>(nout, 15); i++) out[i] = v[i];
    return GPRX_OK;
    API_END(M ? M->ctx : nullptr)
}

gprx_status gprx_dev_ctx_info(gprx_ctx* ctx, int64_t* out, int32_t nout) {
    API_BEGIN
    GPRX_REQUIRE(ctx && out, GPRX_ERR_ARG, "gprx_dev_ctx_info: NULL argument");
    int count = -1, urank = -1;
    if (ctx->comm) {
        if (ncclCommCount(ctx->comm, &count) != ncclSuccess) count = -1;
        if (ncclCommUserRank(ctx->comm, &urank) != ncclSuccess) urank = -1;
    }
    int dom = -1, bus = -1, dev = -1;
    (void)hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, ctx->device);
    (void)hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, ctx->device);
    (void)hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, ctx->device);
    const int64_t transport = ctx->virt ? 3 : (ctx->comm ? 1 : (ctx->peer ? 2 : 0));
    const int64_t v[10] = {ctx->rank, ctx->world, ctx->device, transport, count, urank, dom, bus, dev, ctx->cu_slot};
    for (int i = 0; i < std::min<int32_t>(nout, 10); i++) out[i] = v[i];
    return GPRX_OK;
    API_END(ctx)
}

gprx_status gprx_dist_unique_id(void* out) {
    API_BEGIN
    GPRX_REQUIRE(out, GPRX_ERR_ARG, "gprx_dist_unique_id: out is NULL");
    static_assert(sizeof(ncclUniqueId) == GPRX_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) throw Error{GPRX_ERR_RCCL, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r)};
    std::memcpy(out, &id, sizeof(id));
    return GPRX_OK;
    API_END(nullptr)
}

gprx_status gprx_ctx_create_virtual(int device, int world, gprx_ctx** out) {
    API_BEGIN
    GPRX_REQUIRE(out, GPRX_ERR_ARG, "gprx_ctx_create_virtual: NULL argument");
    GPRX_REQUIRE(world >= 1 && world <= 8, GPRX_ERR_ARG, "gprx_ctx_create_virtual: world must be 1..8");
    gprx_ctx* ctx = ctx_new(device);
    ctx->virt = true;
    ctx->world = world;
    *out = ctx;
    return GPRX_OK;
    API_END(nullptr)
}

gprx_status gprx_ctx_create_dist(int device, int rank, int world, const void* unique_id, gprx_ctx** out) {
    API_BEGIN
    GPRX_REQUIRE(out && unique_id, GPRX_ERR_ARG, "gprx_ctx_create_dist: NULL argument");
    GPRX_REQUIRE(world >= 1 && rank >= 0 && rank < world, GPRX_ERR_ARG, "gprx_ctx_create_dist: bad rank/world");
    gprx_ctx* ctx = ctx_new(device);
    ctx->rank = rank;
    ctx->world = world;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    // GPRX_RCCL_FAIL=1 (testing): fail as an initialisation that never completes would, so the
    // caller's fallback (a peer context over its own all-gather) can be exercised
    if (const char* e = std::getenv("GPRX_RCCL_FAIL"); e && std::atoi(e) != 0) {
        gprx_ctx_destroy(ctx);
        throw Error{GPRX_ERR_RCCL, "ncclCommInitRankConfig: forced failure (GPRX_RCCL_FAIL)"};
    }
    // nonblocking initialisation, polled with a deadline (GPRX_RCCL_INIT_TIMEOUT_S, default
    // 120 s): a rank that cannot reach its peers returns GPRX_ERR_RCCL instead of blocking
    // the process for ever inside ncclCommInitRank
    double tmo = 120.0;
    if (const char* e = std::getenv("GPRX_RCCL_INIT_TIMEOUT_S"); e && std::atof(e) > 0) tmo = std::atof(e);
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    ncclComm_t comm = nullptr;
    ncclResult_t r = ncclCommInitRankConfig(&comm, world, id, rank, &cfg);
    try {
        if (r != ncclSuccess && r != ncclInProgress)
            throw Error{GPRX_ERR_RCCL, std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r)};
        rccl_settle(comm, r, "ncclCommInitRankConfig", tmo);
    } catch (...) {
        if (comm) (void)ncclCommAbort(comm);
        gprx_ctx_destroy(ctx);
        throw;
    }
    ctx->comm = comm;
    ctx->hc = make_rccl_coll(ctx->comm, world, device);
    *out = ctx;
    return GPRX_OK;
    API_END(nullptr)
}

gprx_status gprx_ctx_create_peer(int device, int rank, int world, gprx_allgather_fn fn, void* user, gprx_ctx** out) {
    API_BEGIN
    GPRX_REQUIRE(out && fn, GPRX_ERR_ARG, "gprx_ctx_create_peer: NULL argument");
    GPRX_REQUIRE(world >= 1 && world <= 32 && rank >= 0 && rank < world, GPRX_ERR_ARG,
                 "gprx_ctx_create_peer: bad rank/world");
    gprx_ctx* ctx = ctx_new(device);
    ctx->rank = rank;
    ctx->world = world;
    ctx->peer = true;
    ctx->hc = make_callback_coll(fn, user, world);
    if (const char* e = std::getenv("GPRX_DIST_SHARED_GPU"); e && std::atoi(e) != 0) {
        ctx->cu_slot = rank;
        ctx->cu_slots = world;
    }
    *out = ctx;
    return GPRX_OK;
    API_END(nullptr)
}

gprx_status gprx_sparse_fit(gprx_ctx* ctx, gprx_dtype dtype, const gprx_kernel_desc* kernel, const void* X,
                            const void* Y, int64_t n, int32_t d, int32_t m, const void* Xm, int64_t M, double sigma,
                            double jitter, void* Kinv, void* RV, void* RM) {
    API_BEGIN
    GPRX_REQUIRE(ctx && kernel && Xm && (X || n == 0) && (Y || n == 0), GPRX_ERR_ARG, "gprx_sparse_fit: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);  // after the lock: resolved (streams drained) before it is released
    return by_dtype(dtype, [&](auto t) {
        return sparse_fit_impl<decltype(t)>(ctx, kernel, X, Y, n, d, m, Xm, M, sigma, jitter, Kinv, RV, RM);
    });
    API_END(ctx)
}

gprx_status gprx_sparse_lml(gprx_ctx* ctx, gprx_dtype dtype, const gprx_kernel_desc* kernel, const void* X,
                            const void* Y, int64_t n, int32_t d, int32_t m, const void* Xm, int64_t M, double sigma,
                            double jitter, uint32_t flags, double* value, double* grad, int32_t* nparams,
                            double* logdet) {
    API_BEGIN
    GPRX_REQUIRE(M > 0, GPRX_ERR_DIM,
                 "SparseLikelihood::GetValueAndParameterDerivative: there are no inducing samples specified");
    GPRX_REQUIRE(ctx && kernel && Xm && X && Y, GPRX_ERR_ARG, "gprx_sparse_lml: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfBind pb_(ctx);
    return by_dtype(dtype, [&](auto t) {
        return sparse_lml_impl<decltype(t)>(ctx, kernel, X, Y, n, d, m, Xm, M, sigma, jitter, flags, value, grad, nparams,
                                            logdet);
    });
    API_END(ctx)
}

}  // extern "C"
