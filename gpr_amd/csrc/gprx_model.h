// gprx_model.h — the host state behind the C ABI: device buffers, gprx_ctx, gprx_model and its
// lifecycle transitions, error plumbing, transfers, staged point sets and the declarations the
// host translation units (gprx_api / _canon / _fit / _query / _matrix / _sparse .cpp) share.
// Host .cpp files only: never included by a .hip file or a k_*.h.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "gprx_dist.h"
#include "gprx_internal.h"
#include "../../include/gprx_dev.h"

// what this header declares is shared between the library's own files only (as the file-local
// functions it replaces were): kept out of the dynamic symbol table
#pragma GCC visibility push(hidden)

namespace gprx {

// ---------------------------------------------------------------------------------------
// device buffers
// ---------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    void ensure(size_t b) {
        if (b <= bytes && p) return;
        release();
        if (b == 0) return;
        GPRX_HIP(dev_malloc(&p, b));  // (GPRX_POISON: filled with finite garbage, gprx_alloc.h)
        bytes = b;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
    ~DevBuf() { release(); }
};

// Pinned host memory, mapped: the fit's status words come back by one kernel's stores into it
// and one stream synchronisation (three synchronous hipMemcpy calls were three copy launches
// and a host round trip each)
struct PinnedBuf {
    void* p = nullptr;
    double* dev = nullptr;  // the device's address of it (mapped, coherent)
    size_t bytes = 0;
    void ensure(size_t b) {
        if (b <= bytes && p) return;
        release();
        GPRX_HIP(hipHostMalloc(&p, b, hipHostMallocMapped | hipHostMallocCoherent));
        void* d = nullptr;
        GPRX_HIP(hipHostGetDevicePointer(&d, p, 0));
        dev = static_cast<double*>(d);
        bytes = b;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        dev = nullptr;
        bytes = 0;
    }
    ~PinnedBuf() { release(); }
};

// Device copy of a small parameter struct (a kernel tree), uploaded only when its bytes change (a
// pageable hipMemcpyAsync blocks the host until the stream reaches it: every fit paid that wait
// between its feature kernels and the factorisation launch).  One per tree its owner holds.
struct DevParam {
    DevBuf buf;
    std::vector<unsigned char> last;
    template <typename S>
    const S* put(const S& v, hipStream_t s) {
        const bool fresh = buf.bytes < sizeof(S) || !buf.p;
        buf.ensure(sizeof(S));
        const unsigned char* b = reinterpret_cast<const unsigned char*>(&v);
        if (fresh || last.size() != sizeof(S) || std::memcmp(last.data(), b, sizeof(S)) != 0) {
            GPRX_HIP(hipMemcpyAsync(buf.p, &v, sizeof(S), hipMemcpyHostToDevice, s));
            last.assign(b, b + sizeof(S));
        }
        return buf.as<S>();
    }
};

inline int64_t round_up(int64_t x, int64_t g) { return (x + g - 1) / g * g; }

inline size_t esize(gprx_dtype dt) { return dt == GPRX_F64 ? sizeof(double) : sizeof(float); }

// f(T{}) with T the scalar type of dt: `by_dtype(dt, [&](auto t) { using T = decltype(t); ... })`
template <typename F>
auto by_dtype(gprx_dtype dt, F&& f) {
    return dt == GPRX_F64 ? f(double{}) : f(float{});
}

// info < 0: the device scheduler of potrf_tiles timed out waiting for a dependency
inline void check_sched(int hinfo) {
    if (hinfo < 0) throw Error{GPRX_ERR_HIP, "gprx: device factorisation scheduler timed out (tile dependency wait)"};
}

// the builds' non-finite flag, reported as the reference does
inline void check_finite(int hflag) {
    if (hflag)
        throw Error{GPRX_ERR_NONFINITE,
                    "GaussianProcess::ComputeKernelMatrixInternal: kernel matrix contains entries which are not finite."};
}

// the lower triangle of a column-major matrix h (leading dimension ldh) as the full symmetric
// n x n row-major matrix out
template <typename T>
void mirror_lower(const T* h, int64_t ldh, int64_t n, T* out) {
    for (int64_t j = 0; j < n; j++)
        for (int64_t i = j; i < n; i++) out[(size_t)i * n + j] = out[(size_t)j * n + i] = h[(size_t)j * ldh + i];
}

// The environment's path switches, each read once per process.  GPRX_KBUILD: `direct` builds K
// with the VALU kernel, `separate` runs the MFMA build as its own kernel instead of BUILD tasks
// inside the tile factorisation (where the tile builds fill the factorisation's start-up ramp).
// GPRX_PREDICT=direct keeps predict and the cross rows off the MFMA pair statistics.
enum KBuildMode { KBUILD_FUSED = 0, KBUILD_DIRECT, KBUILD_SEPARATE };
inline bool env_is(const char* name, const char* value) {
    const char* e = std::getenv(name);
    return e && std::string(e) == value;
}
inline KBuildMode env_kbuild() {
    static const KBuildMode mode = env_is("GPRX_KBUILD", "direct")     ? KBUILD_DIRECT
                                   : env_is("GPRX_KBUILD", "separate") ? KBUILD_SEPARATE
                                                                       : KBUILD_FUSED;
    return mode;
}
inline bool env_predict_direct() {
    static const bool direct = env_is("GPRX_PREDICT", "direct");
    return direct;
}
// GPRX_LML_GRAD=direct keeps the LML and leave-one-out gradients on the VALU kernel
inline bool env_lml_grad_direct() {
    static const bool direct = env_is("GPRX_LML_GRAD", "direct");
    return direct;
}

}  // namespace gprx

struct gprx_ctx {
    int device = 0;
    int rank = 0, world = 1;
    bool virt = false;          // gprx_ctx_create_virtual: world virtual ranks in this process
    ncclComm_t comm = nullptr;  // RCCL communicator (gprx_ctx_create_dist), world > 1
    gprx::HostColl* hc = nullptr;  // host collectives of a multi-process context (RCCL or the caller's)
    bool peer = false;          // gprx_ctx_create_peer: the caller's collective, no RCCL
    int cu_slot = 0, cu_slots = 1;  // GPRX_DIST_SHARED_GPU: ranks of one GPU split its CUs
    hipStream_t stream = nullptr;  // the context's one stream (highest priority)
    gprx::Exec ex;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    gprx::Prof prof;
    std::shared_ptr<void> sparse_state[2];  // the sparse fit's device buffers per scalar type (sparse_state)
    std::string err;
    std::mutex mu;
};

struct gprx_model {
    gprx_ctx* ctx = nullptr;
    gprx_dtype dt = GPRX_F64;
    int64_t n = 0;
    int d = 0, m = 0;
    int64_t np = 0, mp = 0, ld = 0;
    double sigma = 0;
    bool has_data = false, has_kernel = false, fitted = false;
    bool has_alpha = false;  // regression vectors valid (fit, or gprx_model_set_alpha after Load)
    bool want_inv = false;   // the next fit also forms C = (K + s^2 I)^{-1} (identity rows in the tiles)
    bool inv_ready = false;  // C holds the inverse of the current fit
    gprx_kernel_desc desc{};
    gprx::KCanon<double> kd{};
    gprx::KCanon<float> kf{};
    gprx::DevBuf X, Y, tab, A, Linv, z, alpha, info, flag, red, V, C, scratch1, scratch2, grad, pack, featU, featV;
    // posterior covariance workspace (L^{-1} K(X, x) for a query batch: qp x np each), kept
    // across calls -- at Q = 65536, N = 16384 one buffer is 8.6 GB, whose hipMalloc + free per
    // call cost more than the solve on some boxes
    gprx::DevBuf pvRa, pvRb, pvFq;  // (+ the queries' pair features)
    // gprx_model_append workspace: the new rows' panel, the sin/cos tables of the sample ranges it
    // builds from, the old partial block (restored when the update is refused) and the new alpha
    gprx::DevBuf apPanel, apTab, apStash, apAlpha, apPart;  // (+ the Schur update's split-K partials)
    // gprx_model_remove workspace: the second factor, Linv, X and Y the reduced model is built in
    // (swapped with A, Linv, X, Y when the status words are back, so a sliding window alternates
    // between the two sets) and the rotations' (c, s) pairs (k_remove.hip)
    gprx::DevBuf rmA, rmLinv, rmX, rmY, rmPairs;
    // gprx_model_loo workspace: the gradient's vectors (u, sqrt w, u / sqrt w, a), the reductions'
    // partials, the results on their way to the host and H / 2 (np x np; the call also writes B
    // into V, which nothing reads once C exists)
    gprx::DevBuf looVec, looPart, looOut, looH;
    // gprx_model_posterior / gprx_model_sample workspace (the cross rows R are pvRa): the joint
    // covariance (qp x qp, lower, unfactored), its factored copy with the diagonal blocks'
    // inverses, the mean and the prior diagonal (q m + q), the normals (e-linear, then as the
    // product's operand) and the product with the samples behind it
    gprx::DevBuf psS, psL, psLinv, psVec, psZ, psZp, psOut;
    double psMs[6] = {0, 0, 0, 0, 0, 0};  // the last sample call's device ms per phase (stats on)
    // a fit (a refit, an append, or the fit inside an LML call) and new data free the posterior
    // workspace when it is large (one big variance call must not leave too little HBM
    // for the next fit on the device); the LML's own gradient pass does not
    void trim_posterior_workspace() {
        if (pvRa.bytes + pvRb.bytes + pvFq.bytes > (size_t(1) << 30)) {
            pvRa.release();
            pvRb.release();
            pvFq.release();
        }
        if (looH.bytes > (size_t(1) << 30)) looH.release();
        if (psS.bytes + psL.bytes + psLinv.bytes + psVec.bytes + psZ.bytes + psZp.bytes + psOut.bytes > (size_t(1) << 30))
            for (gprx::DevBuf* b : {&psS, &psL, &psLinv, &psVec, &psZ, &psZp, &psOut}) b->release();
    }
    // the kernel trees on the device (uploaded when they change): the model's T tree, and an fp32
    // model's double tree (the refinement's)
    gprx::DevParam kfit, kfit64;
    gprx::PinnedBuf hstat;   // the fit's status words: flag, info, log det, data fit
    // fp32 models: fp64 iterative refinement state (k_refine.hip).  kd then holds the tree in
    // double with the parameters rounded to float first (the reference stores them in T).
    gprx::DevBuf Xd, Yd, ad, kxd, fud, fvd, tabd, zd, outd, delta, nrm;
    // LU fallback state (k_getrf.hip), double for both scalar types: the factored matrix,
    // pivots, the 128-block inverses of L and U, and scratch
    int method = 0;  // factor of the current fit: 0 Cholesky (A, Linv), 1 LU (lu, ipiv, luL, luU)
    bool lu_forced = false;  // ... asked for by GPRX_FIT_FORCE_LU (gprx_model_append refits the same way)
    gprx::DevBuf lu, ipiv, luUt, luB, lured;
    double lu_sign = 1;  // sign of det(K + sigma^2 I) from the LU
    // distributed fit (gprx_dist.cpp): the engine (per-rank buffers, schedules) and whether
    // the current fit is one (its factor is held in tiles per rank: alpha and predict only)
    gprx::DistEngineBase* dist_engine = nullptr;
    bool dist_fitted = false;
    bool dist_dense = false;  // the tiles of a distributed fit gathered into A (ld np) and Linv
    bool dist_inv_tiles = false;  // LML-mode distributed fit: C in the ranks' tiles (dist_lml_grad)
    gprx::DistFitOut dist_stats;  // layout, window and memory of the last distributed fit
    // a kernel with no device form: the caller evaluated K (n x n, row-major, T) -- the
    // reference's virtual Kernel<T>::operator() (include/Kernel.h:52-59); see k_hostk.hip
    bool host_k = false;
    gprx::DevBuf Kext;
    // a sparse GP's variance state (gprx_model_set_sparse_cov): the model holds the inducing
    // points and W = Kmm^{-1} - RM (padded np x np, column-major) for
    // operator()(x,y) = k(x,y) - Kx^T W Ky (include/SparseGaussianProcess.h:94-106)
    bool sparse_cov = false;
    gprx::DevBuf sparseW;
    // per-dimension length scales (gprx_model_set_length_scales; empty: none).  With scales X holds
    // the SCALED points Xs = Xraw / (T)ell -- what every consumer of the model's points reads, so
    // none of them changes -- and Xraw the points as uploaded (rmXraw: gprx_model_remove's second
    // buffer of them); ellT is ell narrowed to T on the device.  Without scales X is the data as
    // uploaded and Xraw is not used.  ardPart: gprx_model_lml_scale_grad's partials and result.
    std::vector<double> ell;
    gprx::DevBuf Xraw, rmXraw, ellT, ardPart;
    bool scaled() const { return !ell.empty(); }
    std::mutex mu;
    ~gprx_model() { gprx::dist_engine_free(dist_engine); }

    // ---- lifecycle ---------------------------------------------------------------------
    // fitted, has_alpha, inv_ready, sparse_cov, method and the three dist_* flags are assigned
    // by the transitions below and nowhere else.  What each mutating call does with them:
    //
    //   call               drops                                  establishes
    //   set_data           sparse_cov, fit                        (has_data)
    //   set_kernel         sparse_cov, fit                        (has_kernel; host_k off)
    //   set_kernel_matrix  sparse_cov, fit                        (has_kernel; host_k on)
    //   set_length_scales  sparse_cov, fit                        (ell; X rescaled from Xraw)
    //   set_noise          fit                                    -
    //   set_alpha          -                                      has_alpha (the factor stays)
    //   set_sparse_cov     -                                      sparse_cov
    //   fit, one GPU       sparse_cov; dist_fitted and inv_ready  Cholesky: fit_done(0, inverse rode
    //                      at its start, fit once the status        along); LU fallback: fit_done(1, no)
    //                      words are back
    //   fit, forced LU     sparse_cov, fit, dist_fitted/_dense    fit_done(1, no)
    //   fit, sharded       sparse_cov, fit, dist_fitted/_dense    dist_fit_done(inv_tiles), then
    //                                                             inverse_done() in LML mode; its LU
    //                                                             fallback as the forced LU
    //   append             in place: nothing until the status     fit_done(0, no); a refused update
    //                      words are back; full refit: fit,         restores A, Linv and drops nothing
    //                      then as fit
    //   remove             update: nothing until the status       fit_done(0, no); a refused update
    //                      words are back (built in second          leaves every buffer as it was
    //                      buffers); full refit: fit, then as fit
    //   lml               as its fit                             as its fit, + inverse_done() on a
    //                                                             sharded fit
    //   loo               fitted by Cholesky: nothing; else as   fitted: inverse_done() once a gradient
    //                     its fit (no LU fallback)                  formed C; else as its fit
    //   posterior, sample  nothing (the model is read)            -
    //   (first dense use of a sharded fit: dense_gathered())
    //
    // "fit" = fitted, has_alpha, inv_ready.  set_data, set_kernel, set_kernel_matrix and set_noise
    // leave dist_fitted, dist_dense and dist_inv_tiles as they are; nothing clears dist_inv_tiles
    // (dist_fit_done overwrites it) and a one-GPU fit leaves dist_dense (read only with
    // dist_fitted).  Open questions about this table: DESIGN.md, "Host layer".
    void drop_fit() { fitted = has_alpha = inv_ready = false; }
    void drop_sparse_cov() { sparse_cov = false; }
    void drop_dist() { dist_fitted = dist_dense = false; }
    void start_dense_fit() {  // a one-GPU Cholesky fit begins: A is about to be overwritten
        dist_fitted = false;
        inv_ready = false;
    }
    void fit_done(int method_, bool inv_ready_) {
        method = method_;
        fitted = has_alpha = true;
        inv_ready = inv_ready_;
    }
    void dist_fit_done(bool inv_tiles) {
        method = 0;
        fitted = has_alpha = dist_fitted = true;
        dist_inv_tiles = inv_tiles;
    }
    void inverse_done() { inv_ready = true; }
    void dense_gathered() { dist_dense = true; }
    void alpha_loaded() { has_alpha = true; }
    void sparse_cov_loaded() { sparse_cov = true; }
};

namespace gprx {

// Per-call profiler binding: sets the thread's current profiler and resolves the
// recorded events (after draining the stream) when the call returns.
struct ProfBind {
    gprx_ctx* ctx;
    explicit ProfBind(gprx_ctx* c) : ctx(c) { g_prof = (c && c->prof.on) ? &c->prof : nullptr; }
    ProfBind(const ProfBind&) = delete;
    ~ProfBind() {
        if (ctx && ctx->prof.on) {
            (void)hipStreamSynchronize(ctx->stream);
            ctx->prof.resolve();
        }
        g_prof = nullptr;
    }
};

// Every model call holds its context's mutex, then the model's (always in that order): the
// device work of a model runs on the context's stream and uses the context's scratch (the
// tile factorisation's ticket and counter words, its cached schedules, the timing events),
// so two models of one context must not interleave their launches -- a second fit's memset
// of the ticket counter landing between another fit's memset and launch leaves that launch
// with a spent ticket.  Calls on one model from several threads are serialised as well.
struct ModelLock {
    std::lock_guard<std::mutex> c, m;
    explicit ModelLock(gprx_model* M) : c(M->ctx->mu), m(M->mu) {}
};

// ---------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------
gprx_status fail(gprx_ctx* ctx, gprx_status st, const std::string& msg);  // (gprx_api.cpp)

#define API_BEGIN try {
#define API_END(ctx)                                                                   \
    }                                                                                  \
    catch (const gprx::Error& e) {                                                     \
        return gprx::fail(ctx, e.st, e.msg);                                           \
    }                                                                                  \
    catch (const std::exception& e) {                                                  \
        return gprx::fail(ctx, GPRX_ERR_HIP, e.what());                                \
    }                                                                                  \
    catch (...) {                                                                      \
        return gprx::fail(ctx, GPRX_ERR_HIP, "unknown exception");                     \
    }

template <typename T>
KCanon<T>& kcanon(gprx_model* m);  // the model's tree in T
template <>
inline KCanon<double>& kcanon<double>(gprx_model* m) {
    return m->kd;
}
template <>
inline KCanon<float>& kcanon<float>(gprx_model* m) {
    return m->kf;
}

// the model's length scales in T on the device, nullptr without scales (stage_points' ell)
template <typename T>
const T* model_ell(const gprx_model* m) {
    return m->scaled() ? m->ellT.as<T>() : nullptr;
}

// ---------------------------------------------------------------------------------------
// transfers
// ---------------------------------------------------------------------------------------
// Host <-> device transfers use pageable caller memory: always synchronous, after the
// work stream has drained (no async copies from/to pageable memory).  An input may also be
// device memory (unified addressing decides the direction, hipMemcpyDefault): a caller whose
// samples already live in HBM passes them without a PCIe round trip.
template <typename T>
void upload(DevBuf& b, const void* host, size_t bytes, hipStream_t s) {
    b.ensure(bytes);
    GPRX_HIP(hipStreamSynchronize(s));
    if (bytes) GPRX_HIP(hipMemcpy(b.p, host, bytes, hipMemcpyDefault));
}

// (the destination may be device memory too -- unified addressing decides the direction -- so
// a caller that keeps results in HBM gets them without a PCIe round trip)
inline void download(void* host, const void* dev, size_t bytes, hipStream_t s) {
    GPRX_HIP(hipStreamSynchronize(s));
    GPRX_HIP(hipGetLastError());
    if (bytes) GPRX_HIP(hipMemcpy(host, dev, bytes, hipMemcpyDefault));
}

// An input the caller may pass as host or as device memory: device memory of this context's GPU
// is used where it is (no copy), anything else is copied into `b`.
template <typename T>
const T* dev_input(DevBuf& b, const void* p, size_t bytes, int device, hipStream_t s) {
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (p && hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device)
        return static_cast<const T*>(p);
    (void)hipGetLastError();  // (an unregistered host pointer reports an error: not sticky)
    upload<T>(b, p, bytes, s);
    return b.as<T>();
}

template <typename T>
void download_sym(void* out, const DevBuf& C, int64_t ldc, int64_t n, hipStream_t s) {
    // mirrored on the device, then one strided copy: the full symmetric matrix reads the same
    // row- or column-major, so it lands in the caller's buffer as is
    launch_sym_fill<T>(C.as<T>(), ldc, n, s);
    GPRX_HIP(hipGetLastError());
    GPRX_HIP(hipMemcpy2DAsync(out, sizeof(T) * n, C.p, sizeof(T) * ldc, sizeof(T) * n, n, hipMemcpyDefault, s));
    GPRX_HIP(hipStreamSynchronize(s));
}

inline void swap_buf(DevBuf& a, DevBuf& b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}

// b grown to at least `need` bytes, its first `keep` bytes kept (with head-room: a run of
// one-row appends reallocates rarely)
inline void grow_keep(DevBuf& b, size_t need, size_t keep, hipStream_t s) {
    if (need <= b.bytes && b.p) return;
    DevBuf nb;
    nb.ensure(need + need / 8 + 4096);
    GPRX_HIP(hipStreamSynchronize(s));
    if (keep && b.p) GPRX_HIP(hipMemcpy(nb.p, b.p, std::min(keep, b.bytes), hipMemcpyDeviceToDevice));
    swap_buf(b, nb);
}

// ---------------------------------------------------------------------------------------
// staged point sets
// ---------------------------------------------------------------------------------------
// the sin/cos tables of n points (2 * K.nper planes of n x d) into `tab`; nullptr, and nothing
// launched, for a tree without periodic leaves
template <typename T>
const T* sincos_tables(const KCanon<T>& K, const T* x, int64_t n, int d, DevBuf& tab, hipStream_t s) {
    if (K.nper == 0) return nullptr;
    tab.ensure(sizeof(T) * 2 * K.nper * n * d);
    launch_sincos_tables<T>(K, x, n, d, tab.as<T>(), s);
    return tab.as<T>();
}

template <typename T>
struct Points {  // a set of points on the device with what the kernels read of it
    const T* x = nullptr;
    int64_t n = 0;
    const T* tab = nullptr;  // sin/cos tables, nullptr when K.nper == 0
    DevBuf xbuf, tabbuf;     // owned only when staged here
};

// n points of the caller's (n x d, row-major) on the device, with their tables.  accept_device:
// device memory of this GPU is read where it lies (dev_input); otherwise the points are always
// copied (upload), so the staged set never aliases memory the caller may overwrite.
// ell (a model's length scales in T on the device, or nullptr): the staged copy is divided by them,
// as the model's own points are (never with accept_device: the copy is written).
template <typename T>
void stage_points(Points<T>& P, const KCanon<T>& K, const void* p, int64_t n, int d, int device, hipStream_t s,
                  bool accept_device, const T* ell = nullptr) {
    if (accept_device && !ell) {
        P.x = dev_input<T>(P.xbuf, p, sizeof(T) * n * d, device, s);
    } else {
        upload<T>(P.xbuf, p, sizeof(T) * n * d, s);
        P.x = P.xbuf.template as<T>();
        if (ell && n > 0) launch_scale_points<T>(P.x, ell, n, d, P.xbuf.template as<T>(), s);
    }
    P.n = n;
    P.tab = sincos_tables<T>(K, P.x, n, d, P.tabbuf, s);
}

// the model's own table of its samples (M->tab); false when the tree has no periodic leaf
template <typename T>
bool ensure_train_tables(gprx_model* M) {
    return sincos_tables<T>(kcanon<T>(M), M->X.as<T>(), M->n, M->d, M->tab, M->ctx->stream) != nullptr;
}

// pair features of the model's samples (k_pairs.hip), centred on its first sample, np rows
// apart: the U side into featU, the V side into featV
template <typename T>
void train_features(gprx_model* M, bool v_side, int64_t np) {
    const KCanon<T>& K = kcanon<T>(M);
    DevBuf& f = v_side ? M->featV : M->featU;
    f.ensure(sizeof(T) * np * pairs_feature_cols<T>(K, M->d));
    launch_pair_features<T>(K, M->X.as<T>(), M->n, M->d, M->X.as<T>(), v_side, f.as<T>(), np, M->ctx->stream);
}

// a model with length scales: rows [row0, row0 + rows) of X = those rows of Xraw / (T)ell
template <typename T>
void scale_model_rows(gprx_model* M, int64_t row0, int64_t rows) {
    launch_scale_points<T>(M->Xraw.as<T>() + row0 * M->d, M->ellT.as<T>(), rows, M->d, M->X.as<T>() + row0 * M->d,
                           M->ctx->stream);
}

// pair features of q query points against the model's samples (same centre), qp rows apart
template <typename T>
void query_features(gprx_model* M, const T* xq, int64_t q, int64_t qp, DevBuf& f) {
    const KCanon<T>& K = kcanon<T>(M);
    f.ensure(sizeof(T) * qp * pairs_feature_cols<T>(K, M->d));
    launch_pair_features<T>(K, xq, q, M->d, M->X.as<T>(), false, f.as<T>(), qp, M->ctx->stream);
}

// ---------------------------------------------------------------------------------------
// functions the translation units call across files (T = float, double: instantiated explicitly
// in the file that defines them)
// ---------------------------------------------------------------------------------------
// gprx_fit.cpp
template <typename T>
gprx_status model_fit(gprx_model* M, uint32_t flags, gprx_fit_info* out);
template <typename T>
gprx_status model_append(gprx_model* M, const void* Xnew, const void* Ynew, int64_t k, uint32_t flags,
                         gprx_fit_info* out);
template <typename T>
gprx_status model_remove(gprx_model* M, int64_t first, int64_t count, uint32_t flags, gprx_fit_info* out);
template <typename T>
void model_inverse(gprx_model* M);
template <typename T>
void ensure_dense_factor(gprx_model* M);
void lu_solve_model(gprx_model* M, double* B, int m);
// gprx_query.cpp
template <typename T>
gprx_status model_predict(gprx_model* M, const void* Xq, int64_t q, void* mean, void* deriv);
template <typename T>
gprx_status model_posterior_cov(gprx_model* M, const void* Xa, const void* Xb, int64_t q, void* out);
template <typename T>
gprx_status model_core_matrix(gprx_model* M, void* Cout);
template <typename T>
gprx_status model_lml(gprx_model* M, uint32_t flags, double* value, double* grad, int32_t* nparams, double* logdet);
template <typename T>
gprx_status model_loo(gprx_model* M, uint32_t flags, double* value, void* mean, void* var, double* grad,
                      int32_t* nparams);
template <typename T>
gprx_status model_lml_scale_grad(gprx_model* M, double* grad_ell);
template <typename T>
gprx_status model_posterior(gprx_model* M, const void* Xq, int64_t q, uint32_t flags, void* mean, void* cov);
template <typename T>
gprx_status model_sample(gprx_model* M, const void* Xq, int64_t q, int64_t nsamp, uint64_t seed, uint32_t flags,
                         const void* z, double* jitter, void* out);
template <typename T>
gprx_status model_predict_kx(gprx_model* M, const void* Kx, const void* Xq, int64_t q, void* mean, void* deriv);
template <typename T>
gprx_status model_posterior_cov_kx(gprx_model* M, const void* Kxa, const void* Kxb, const void* kab, int64_t q,
                                   void* out);
template <typename T>
gprx_status model_lml_dk(gprx_model* M, uint32_t flags, const void* dK, int32_t P, double* value, double* grad,
                         double* logdet);
// gprx_matrix.cpp
template <typename T>
gprx_status kernel_matrix_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* X, int64_t n, int d,
                               void* Kout, bool deriv);
template <typename T>
gprx_status cross_matrix_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* A, int64_t na, const void* B,
                              int64_t nb, int d, void* Kout);
template <typename T>
gprx_status cholesky_impl(gprx_ctx* ctx, void* Ahost, int64_t n, int32_t* info, bool inverse);
template <typename T>
gprx_status dev_build_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* X, int64_t n, int d, double sigma,
                           int path, void* Kout, int iters = 0, double* ms = nullptr);
// gprx_sparse.cpp
template <typename T>
gprx_status sparse_fit_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* Xh, const void* Yh, int64_t n,
                            int d, int m, const void* Xmh, int64_t M, double sigma, double jitter, void* Kinv, void* RV,
                            void* RM);
template <typename T>
gprx_status sparse_lml_impl(gprx_ctx* ctx, const gprx_kernel_desc* desc, const void* Xh, const void* Yh, int64_t n,
                            int d, int m, const void* Xmh, int64_t M, double sigma, double jitter, uint32_t flags,
                            double* value, double* grad, int32_t* nparams, double* logdet);

}  // namespace gprx

#pragma GCC visibility pop

namespace gprx {
// gprx_dev.cpp (as visible as before)
gprx_status gprx_dev_bench_impl(gprx_dtype dtype, int32_t what, int64_t M, int64_t N, int64_t K, int32_t iters,
                                double* ms, Exec* ex);
gprx_status gprx_dev_forward_panel_impl(gprx_dtype dtype, const void* L, int64_t n, void* R, int32_t rows,
                                        int32_t use_gemm, Exec* ex, hipStream_t s);
gprx_status gprx_dev_factor_update_impl(gprx_dtype dtype, const void* L, int64_t n, const void* X, int32_t r,
                                        void* Lout, void* LinvOut, Exec* ex, hipStream_t s);
}  // namespace gprx
