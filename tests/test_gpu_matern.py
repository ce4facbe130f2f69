"""Matern 3/2 and 5/2 as device leaf kernels, through every entry point, against numpy in fp64
from direct differences (tests/matern_ref.py; the CPU oracle does not know these kernels).

Trees without a White leaf and with one periodic leaf at most take the stand-alone MFMA build
(kbuild_mma_kernel_m), predict_mma_kernel_m, kcross_mma_kernel_m and, when they are sums of
leaves, grad_mma_kernel_m (k_pairs.hip); "m32_x_gauss" and "m52per_m32" have product terms and
take the VALU gradient, "m32_white" and "2per_m52" the VALU build and predict.  Tolerances are
those of the test of the same entry point in tests/test_gpu_trees.py / test_gpu_build.py; every
tree has cond(K + sigma^2 I) <= 2e3 on make_data(300, 3) (tests/test_matern_cpu.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import matern_ref as R
from tests.helpers import make_data, make_queries, relerr, TOL

gpu = pytest.mark.gpu
pytestmark = gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = [np.float64, np.float32]
NAMES, TREES, NODES, SIGMA = R.NAMES, R.TREES, R.NODES, R.SIGMA
ARG = 8  # GPRX_ERR_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fitted(ctx, ks, X, Y, dtype=np.float64, sigma=SIGMA, flags=0):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X.astype(dtype), Y.astype(dtype))
    M.set_kernel(ks)
    M.set_noise(sigma)
    return M, M.fit(flags)


def data_fit(name, n, d, m, sigma=SIGMA):
    X, Y = make_data(n, d, m)
    a, C, ld = R.ref_fit(name, X, Y, sigma, key=(name, n, d, m, sigma))
    return X, Y, a, C, ld


# ---------------------------------------------------------------------------------------
# 1. matrices
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [(1, 1), (129, 33), (260, 5)])
def test_kernel_matrix(ctx, name, dtype, n, d):
    X, _ = make_data(n, d, dtype=dtype)
    K = ctx.kernel_matrix(TREES[name], X, dtype)
    assert relerr(K, R.kmat(NODES[name], X)) <= (1e-12 if dtype == np.float64 else 2e-5)
    assert np.array_equal(K, K.T)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n,d", [(1, 1), (129, 33), (260, 5)])
def test_cross_matrix(ctx, name, n, d):
    A, _ = make_data(n, d)
    B = make_queries(45, d)
    assert relerr(ctx.cross_matrix(TREES[name], A, B), R.cross(NODES[name], A, B)) <= 1e-12
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    assert relerr(ctx.cross_matrix(TREES[name], A32, B32, np.float32), R.cross(NODES[name], A32, B32)) <= 2e-5


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n,d", [(1, 1), (129, 33), (260, 5)])
def test_deriv_matrix(ctx, name, n, d):
    X, _ = make_data(n, d)
    D = ctx.deriv_matrix(TREES[name], X)
    Dr = R.dmat(NODES[name], X)
    assert D.shape == Dr.shape == (NODES[name].num_params(), n, n)
    for p in range(Dr.shape[0]):
        assert relerr(D[p], Dr[p]) <= 1e-10, p


def _inputs(kind, n, d):
    X, _ = make_data(n, d)
    return {"unit": X, "offset": X + 1e3, "wide": X * 50.0}[kind]


def _rescaled(node, f):
    """The tree with every length scale multiplied by f (wide inputs: a length scale of the order
    of the data range, so the off-diagonal is not all underflow)."""
    from gpr_amd import kernels as kn
    if not node.is_leaf:
        return kn.KernelNode(node.name, k1=_rescaled(node.k1, f), k2=_rescaled(node.k2, f))
    p = list(node.params)
    i = {"GaussianKernel": 0, "Matern32Kernel": 0, "Matern52Kernel": 0, "RationalQuadraticKernel": 1}.get(node.name)
    if i is not None:
        p[i] *= f
    elif node.name == "PeriodicKernel":
        p[1] /= f  # the frequency
    return kn.KernelNode(node.name, p)


@pytest.mark.parametrize("kind", ["unit", "offset", "wide"])
@pytest.mark.parametrize("name", R.MMA)
def test_build_matrix_mfma(ctx, name, kind):
    """The stand-alone MFMA build (path 1) on inputs that exercise the cancellation in the r2
    expansion; the diagonal is r2 = 0 exactly, so it is bit-equal to k(x, x) + sigma^2."""
    n, d, sigma = 260, 5, 0.4
    X = _inputs(kind, n, d)
    node = _rescaled(NODES[name], 50.0) if kind == "wide" else NODES[name]
    K = ctx.build_matrix(node.to_string(), X, sigma, 1)
    ref = R.kmat(node, X) + sigma * sigma * np.eye(n)
    if kind == "wide":
        assert np.median(ref) > 1e-3  # (not all underflow)
    e = relerr(K, ref)
    print(f"build {name} {kind}: {e:.3e}")
    assert e <= 1e-12
    assert np.array_equal(np.diag(K), np.full(n, R.diag_value(node) + sigma * sigma))


@pytest.mark.parametrize("name", NAMES)
def test_build_matrix_fused_refused(ctx, name):
    """The fused BUILD tasks stay exp-form only: path 0 refuses every tree with a Matern leaf."""
    import gpr_amd
    X, _ = make_data(260, 5)
    with pytest.raises(gpr_amd.GprxError):
        ctx.build_matrix(TREES[name], X, 0.4, 0)


# ---------------------------------------------------------------------------------------
# 2. fit and predict
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fit_predict(ctx, name, dtype):
    n, d, m, q = 300, 3, 2, 130
    X, Y, a_ref, _, ld_ref = data_fit(name, n, d, m)
    tol = TOL[np.dtype(dtype)]
    M, info = fitted(ctx, TREES[name], X, Y, dtype)
    assert info.method == 0
    Xq = make_queries(q, d)
    mean, D = M.predict(Xq.astype(dtype), deriv=True)
    mr, Dr = R.ref_predict(name, X, a_ref, Xq, deriv=True)
    errs = relerr(M.alpha(), a_ref), relerr(mean, mr), relerr(D, Dr)
    print(f"fit {name} {np.dtype(dtype).name}: alpha {errs[0]:.3e} mean {errs[1]:.3e} deriv {errs[2]:.3e}")
    assert errs[0] <= tol and errs[1] <= tol and errs[2] <= tol
    assert relerr(M.predict(Xq.astype(dtype)), mr) <= tol  # (the mean-only call)
    assert abs(info.logdet - ld_ref) <= (1e-8 if dtype == np.float64 else 1e-3) * max(1, abs(info.logdet))
    M.close()


@pytest.mark.parametrize("name", ["m52", "m32_per"])
def test_fit_predict_one_label_column(ctx, name):
    """m = 1: the mean goes through predict_mma_kernel_m (MFMA predict carries one column)."""
    n, d = 300, 3
    X, Y, a_ref, _, _ = data_fit(name, n, d, 1)
    M, _ = fitted(ctx, TREES[name], X, Y)
    Xq = make_queries(130, d)
    assert relerr(M.alpha(), a_ref) <= 1e-6
    assert relerr(M.predict(Xq), R.ref_predict(name, X, a_ref, Xq)) <= 1e-6
    M.close()


def test_fit_three_label_columns(ctx):
    name, n, d, m = "gauss_m52", 300, 3, 3
    X, Y, a_ref, _, _ = data_fit(name, n, d, m)
    M, _ = fitted(ctx, TREES[name], X, Y)
    Xq = make_queries(70, d)
    assert M.alpha().shape == (n, m) and relerr(M.alpha(), a_ref) <= 1e-6
    assert relerr(M.predict(Xq), R.ref_predict(name, X, a_ref, Xq)) <= 1e-6
    M.close()


# ---------------------------------------------------------------------------------------
# 3. queries on training samples: the clamp of the unclamped predict statistic
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m32", "m52", "gauss_m52"])
@pytest.mark.parametrize("shift", [0.0, 1e-9])
def test_predict_on_training_samples(ctx, name, shift):
    """r2 from the norm expansion comes out at about -1e-16 for a query on a training sample; a
    square root of that is NaN unless the Matern branches clamp it."""
    n, d = 300, 3
    X, Y, a_ref, _, _ = data_fit(name, n, d, 1)
    M, _ = fitted(ctx, TREES[name], X, Y)
    Xq = X[:40].copy() + shift
    mean = M.predict(Xq)
    mr = R.ref_predict(name, X, a_ref, Xq)
    assert np.all(np.isfinite(mean))
    assert np.max(np.abs(mean - mr)) <= 1e-6
    M.close()


# ---------------------------------------------------------------------------------------
# 4. non-finite inputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("name", ["m32", "gauss_m52", "m32_white"])
def test_fit_rejects_nonfinite_inputs(ctx, name, bad):
    import gpr_amd
    X, Y = make_data(200, 4)
    X = X.copy()
    X[77, 2] = bad
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X, Y)
    M.set_kernel(TREES[name])
    M.set_noise(0.5)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.fit()
    assert "not finite" in str(e.value)
    M.close()


@pytest.mark.parametrize("name", ["m32", "m52", "m32_white"])
def test_nan_query_gives_nan_in_its_row_only(ctx, name):
    X, Y, _, _, _ = data_fit(name, 300, 3, 1)
    M, _ = fitted(ctx, TREES[name], X, Y)
    Xq = make_queries(10, 3)
    Xq[3, 1] = np.nan
    mean = M.predict(Xq)
    assert np.isnan(mean[3, 0])
    assert np.all(np.isfinite(np.delete(mean, 3, axis=0)))
    M.close()


# ---------------------------------------------------------------------------------------
# 5. posterior
# ---------------------------------------------------------------------------------------
def _ref_cov(name, X, C, Xa, Xb):
    Ka, Kb = R.cross(NODES[name], Xa, X), R.cross(NODES[name], Xb, X)
    kab = np.array([R.cross(NODES[name], Xa[i:i + 1], Xb[i:i + 1])[0, 0] for i in range(Xa.shape[0])])
    return kab - np.sum((Ka @ C) * Kb, axis=1), kab


@pytest.mark.parametrize("name", NAMES)
def test_posterior(ctx, name):
    n, d, sigma = 300, 3, 0.3
    X, Y, _, C_ref, _ = data_fit(name, n, d, 1, sigma)
    M, _ = fitted(ctx, TREES[name], X, Y, sigma=sigma)
    Xa = make_queries(40, d)
    for Xb in (Xa, Xa[::-1].copy()):
        c_ref, kab = _ref_cov(name, X, C_ref, Xa, Xb)
        assert np.max(np.abs(M.posterior_cov(Xa, Xb) - c_ref)) <= 1e-6 * max(1.0, np.max(np.abs(kab)))
    ci_ref = 2 * np.sqrt(np.maximum(_ref_cov(name, X, C_ref, Xa, Xa)[0], 0))
    assert np.max(np.abs(M.credible_interval(Xa) - ci_ref)) <= 1e-6 * max(1.0, np.max(ci_ref))
    assert relerr(M.core_matrix(), C_ref) <= 1e-6
    M.close()


@pytest.mark.parametrize("name", ["m32", "gauss_m52", "m52per_m32", "m32_white"])
def test_posterior_f32(ctx, name):
    """fp32, queries within 1e-3 of training samples, at the fp32 bar on the scale of k(x, x); the
    reference is numpy's fp64 solve of the fp32 inputs' system."""
    n, d, sigma = 300, 3, 0.3
    X, Y = make_data(n, d)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    M, _ = fitted(ctx, TREES[name], X32, Y32, np.float32, sigma)
    _, C_ref, _ = R.ref_fit(name, X32.astype(np.float64), Y32.astype(np.float64), sigma)
    rng = np.random.default_rng(7)
    Xa = (X32[rng.choice(n, 64, replace=False)] + 1e-3 * rng.standard_normal((64, d))).astype(np.float32)
    kaa = R.diag_value(NODES[name])
    for Xb in (Xa, Xa[::-1].copy()):
        c_ref, _ = _ref_cov(name, X32.astype(np.float64), C_ref, Xa.astype(np.float64), Xb.astype(np.float64))
        assert np.max(np.abs(M.posterior_cov(Xa, Xb) - c_ref)) <= TOL[F32] * max(1.0, kaa)
    assert relerr(M.core_matrix(), C_ref) <= TOL[F32]
    M.close()


# ---------------------------------------------------------------------------------------
# 6. LML value and gradient
# ---------------------------------------------------------------------------------------
_lml = {}


def lml_ref(name, n, d, sigma):
    key = (name, n, d, sigma)
    if key not in _lml:
        X, Y = make_data(n, d)
        X.setflags(write=False)
        Y.setflags(write=False)
        _lml[key] = (X, Y) + R.ref_lml(name, X, Y[:, 0], sigma)
    return _lml[key]


@pytest.mark.parametrize("name", NAMES)
def test_lml(ctx, name):
    """n = 300: three row tiles, the last one partial.  Single m32 / m52: the tree's last (only)
    leaf has two parameters; rq_m32 has the Matern leaf last among three-parameter leaves, m32_per
    has it first.  The gradient is written into a buffer with sentinels behind its nparams slots."""
    from gpr_amd import gprx
    n, d, sigma = 300, 5, 0.7
    X, Y, vr, gr, ldr = lml_ref(name, n, d, sigma)
    M, _ = fitted(ctx, TREES[name], X, Y, sigma=sigma)
    v, g, logdet = M.lml(grad=True)
    e = relerr(g, gr)
    print(f"lml {name}: value {abs(v - vr) / max(1.0, abs(vr)):.3e} grad {e:.3e}")
    assert abs(v - vr) <= 1e-6 * max(1.0, abs(vr))
    assert abs(logdet - ldr) <= 1e-8 * max(1.0, abs(ldr))
    assert g.shape == (NODES[name].num_params(),) and g.shape == gr.shape
    assert e <= 1e-6
    buf = np.full(gprx.MAX_KPARAMS, 777.0)
    vv, npar, ld = ctypes.c_double(), ctypes.c_int32(), ctypes.c_double()
    M._c(gprx.lib().gprx_model_lml(M.h, gprx.LML_GRAD, ctypes.byref(vv), gprx._ptr(buf), ctypes.byref(npar),
                                   ctypes.byref(ld)))
    assert npar.value == NODES[name].num_params()
    assert relerr(buf[:npar.value], g) <= 1e-10  # (the VALU gradient sums with atomics: not bit-stable)
    assert np.all(buf[npar.value:] == 777.0)  # nothing written past the last leaf's slots
    M.close()


@pytest.mark.parametrize("name", ["m52", "rq_m32"])
def test_lml_f32(ctx, name):
    n, d, sigma = 300, 5, 0.7
    X, Y, vr, gr, _ = lml_ref(name, n, d, sigma)
    M, _ = fitted(ctx, TREES[name], X, Y, np.float32, sigma)
    v, g, _ = M.lml(grad=True)
    assert abs(v - vr) <= 1e-3 * max(1.0, abs(vr))
    assert g.shape == gr.shape and relerr(g, gr) <= 1e-3
    M.close()


# ---------------------------------------------------------------------------------------
# 7. the device leaf against the same kernel through the host-kernel route
# ---------------------------------------------------------------------------------------
class _HostMatern32:
    def __init__(self, node):
        self.node = node

    def __call__(self, A, B):
        return R.cross(self.node, A, B)

    def gradient(self, A, B):
        assert A is B or np.array_equal(A, B)
        return R.dmat(self.node, A)


def test_device_leaf_matches_host_kernel_route(ctx):
    n, d, sigma = 300, 3, 0.3
    X, Y = make_data(n, d, 1)
    Md, _ = fitted(ctx, TREES["m32"], X, Y, sigma=sigma)
    Mh, _ = fitted(ctx, _HostMatern32(NODES["m32"]), X, Y, sigma=sigma)
    Xq = make_queries(40, d)
    assert relerr(Md.alpha(), Mh.alpha()) <= 1e-9
    assert relerr(Md.predict(Xq), Mh.predict(Xq)) <= 1e-9
    vd, gd, _ = Md.lml(grad=True)
    vh, gh, _ = Mh.lml(grad=True)
    assert abs(vd - vh) <= 1e-9 * abs(vh)
    assert relerr(gd, gh) <= 1e-9
    Md.close()
    Mh.close()


# ---------------------------------------------------------------------------------------
# 8. append   9. forced LU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SUMS)
@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("dtype", DTYPES)
def test_append(ctx, dtype, k, name):
    n, d, m = 300, 3, 2
    X, Y, a_ref, _, ld_ref = data_fit(name, n + k, d, m)
    tol = TOL[np.dtype(dtype)]
    M, _ = fitted(ctx, TREES[name], X[:n], Y[:n], dtype)
    info = M.append(X[n:].astype(dtype), Y[n:].astype(dtype))
    assert info.appended == k and info.method == 0
    assert M.n == n + k and M.alpha().shape == (n + k, m)
    assert relerr(M.alpha(), a_ref) <= tol
    Xq = make_queries(64, d)
    mean, D = M.predict(Xq.astype(dtype), deriv=True)
    mr, Dr = R.ref_predict(name, X, a_ref, Xq, deriv=True)
    assert relerr(mean, mr) <= tol and relerr(D, Dr) <= tol
    assert abs(info.logdet - ld_ref) <= (1e-8 if dtype == np.float64 else 1e-3) * max(1, abs(info.logdet))
    M.close()


def test_forced_lu(ctx):
    from gpr_amd import gprx
    name, n, d, m = "gauss_m52", 300, 3, 2
    X, Y, a_ref, C_ref, ld_ref = data_fit(name, n, d, m)
    M, info = fitted(ctx, TREES[name], X, Y, flags=gprx.FIT_FORCE_LU)
    assert info.method == 1
    assert relerr(M.alpha(), a_ref) <= 1e-6
    Xq = make_queries(64, d)
    assert relerr(M.predict(Xq), R.ref_predict(name, X, a_ref, Xq)) <= 1e-6
    assert abs(info.logdet - ld_ref) <= 1e-8 * max(1.0, abs(ld_ref))
    cov_ref, _ = _ref_cov(name, X, C_ref, Xq, Xq[::-1].copy())
    assert np.max(np.abs(M.posterior_cov(Xq, Xq[::-1].copy()) - cov_ref)) <= 1e-6 * max(1.0, np.max(np.abs(cov_ref)))
    M.close()


# ---------------------------------------------------------------------------------------
# 10. sparse GP: numpy restatements of the returned quantities (oracle/gpr_oracle.cpp
# orc_sparse_fit, sparse_core / sparse_lml)
# ---------------------------------------------------------------------------------------
def _sparse_inputs(n, d, M, m):
    X, Y = make_data(n, d, m)
    return X, Y, X[:: n // M][:M].copy()


def _np_sparse_fit(node, X, Y, Xm, sigma, jitter):
    """K = Kmm + jitter I, S = K + Kmn Knm / sigma^2, Sigma = S^-1:
    Kinv = K^-1, RV = Kinv (K Sigma Kmn Y / sigma^2), RM = Kinv (K Sigma K) Kinv."""
    K = R.kmat(node, Xm) + jitter * np.eye(Xm.shape[0])
    Knm = R.cross(node, X, Xm)
    is2 = 1.0 / (sigma * sigma)
    Ki = np.linalg.inv(K)
    Sig = np.linalg.inv(K + is2 * Knm.T @ Knm)
    A = K @ Sig
    return Ki, Ki @ (is2 * (A @ (Knm.T @ Y))), Ki @ (A @ K) @ Ki


def _np_sparse_lml(node, X, y, Xm, sigma, jitter):
    """-y^T Cinv y / 2 - log det / 2 - n log(2 pi) / 2 with Cinv = I / s2 - Knm inner^-1 Kmn / s2^2,
    inner = K + Kmn Knm / s2, log det = -log|K| + n log s2 + log|inner|."""
    n = X.shape[0]
    s2 = sigma * sigma
    K = R.kmat(node, Xm) + jitter * np.eye(Xm.shape[0])
    Knm = R.cross(node, X, Xm)
    inner = K + Knm.T @ Knm / s2
    t = Knm.T @ y
    df = -0.5 * (y @ y / s2 - t @ np.linalg.solve(inner, t) / (s2 * s2))
    ld = -np.linalg.slogdet(K)[1] + n * np.log(s2) + np.linalg.slogdet(inner)[1]
    return df - 0.5 * ld - 0.5 * n * np.log(2 * np.pi), ld


@pytest.mark.parametrize("name,chunk", [("gauss_m52", None), ("gauss_m52", 64), ("m32_per", None), ("m32_white", None)])
def test_sparse_fit(ctx, monkeypatch, name, chunk):
    if chunk:
        monkeypatch.setenv("GPRX_SPARSE_CHUNK", str(chunk))
    sigma, jitter = 0.5, 1e-4
    X, Y, Xm = _sparse_inputs(700, 3, 40, 2)
    Kinv, RV, RM = ctx.sparse_fit(TREES[name], X, Y, Xm, sigma, jitter)
    Ki_r, RV_r, RM_r = _np_sparse_fit(NODES[name], X, Y, Xm, sigma, jitter)
    assert relerr(Kinv, Ki_r) <= TOL[F64]
    assert relerr(RV, RV_r) <= TOL[F64]
    assert relerr(RM, RM_r) <= TOL[F64]


@pytest.mark.parametrize("name,chunk", [("gauss_m52", None), ("gauss_m52", 64), ("m32_per", None), ("m32_white", None)])
def test_sparse_lml(ctx, monkeypatch, name, chunk):
    """The value against the same formula in numpy; the gradient against Richardson-extrapolated
    central differences (O(h^4) truncation) of that numpy value."""
    if chunk:
        monkeypatch.setenv("GPRX_SPARSE_CHUNK", str(chunk))
    sigma, jitter = 0.5, 1e-3
    X, Y, Xm = _sparse_inputs(600, 3, 40, 1)
    y = Y[:, 0]
    node = NODES[name]
    v, g, ld = ctx.sparse_lml(TREES[name], X, y, Xm, sigma, jitter)
    vr, ld_r = _np_sparse_lml(node, X, y, Xm, sigma, jitter)
    assert abs(v - vr) <= TOL[F64] * max(1.0, abs(vr)), (v, vr)
    assert abs(ld - ld_r) <= TOL[F64] * max(1.0, abs(ld_r)), (ld, ld_r)
    p0 = node.parameters()
    assert g.shape == (len(p0),)
    fd = np.empty(len(p0))
    for i in range(len(p0)):
        def cd(h):
            pp, pm = list(p0), list(p0)
            pp[i] += h
            pm[i] -= h
            return (_np_sparse_lml(R.with_params(node, pp), X, y, Xm, sigma, jitter)[0] -
                    _np_sparse_lml(R.with_params(node, pm), X, y, Xm, sigma, jitter)[0]) / (2 * h)
        h = 1e-2 * abs(p0[i])
        fd[i] = (4 * cd(h / 2) - cd(h)) / 3
    print(f"sparse lml {name}: grad {relerr(g, fd):.3e}")
    assert relerr(g, fd) <= 1e-6, (g, fd)


# ---------------------------------------------------------------------------------------
# 11. sharded fit (two virtual ranks) and the distributed LML gradient
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gauss_m52", "m32_white"])
def test_sharded_fit(name):
    import gpr_amd
    n, d, m = 700, 5, 1
    X, Y, a_ref, _, ld_ref = data_fit(name, n, d, m)
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        M, info = fitted(vctx, TREES[name], X, Y)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        Xq = make_queries(50, d)
        assert relerr(M.predict(Xq), R.ref_predict(name, X, a_ref, Xq)) <= 1e-6
        assert abs(info.logdet - ld_ref) <= 1e-9 * max(1.0, abs(info.logdet))
        df_ref = float(np.sum(Y * a_ref))
        assert abs(info.datafit - df_ref) <= 1e-8 * abs(df_ref)
        if name == "gauss_m52":
            _, g, ld = M.lml(grad=True, distributed=True)
            _, gr, ldr = R.ref_lml(name, X, Y[:, 0], SIGMA)
            assert abs(ld - ldr) <= 1e-9 * abs(ldr)
            assert g.shape == gr.shape and relerr(g, gr) <= 1e-6
        M.close()
    finally:
        vctx.close()


# ---------------------------------------------------------------------------------------
# 12. the C++ host API
# ---------------------------------------------------------------------------------------
def test_cpp_host_api():
    """GaussianProcess<double> with Sum(Matern52, Gaussian): Initialize, Predict and
    GetCredibleInterval against a host solve, a Save / Load round trip, GaussianLogLikelihood's
    gradient against its own central differences (tests/cpp/gp_matern_test.cpp)."""
    path = os.path.join(ROOT, "gpr_amd", "lib", "gp_matern_test")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0, out
    assert len(lines) == 3 and all(l.startswith("PASS") for l in lines), out
