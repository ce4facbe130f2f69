"""Kernel trees at the limits of the device form, against the CPU oracle in fp64.

canonicalize (gprx_canon.cpp) lowers a tree to at most MAX_LEAF = 8 leaves, MAX_TERM = 16 product
terms and MAX_PER = 2 periodic leaves, each periodic leaf with a sin/cos table slot of its own.
A tree with two periodic leaves is off the MFMA pair-statistics paths (pairs_mma_supported), so
every entry point runs the direct kernels' NPER = 2 instantiations: sincos_tables_kernel's second
plane pair, tile_stats<T, 2, R2>, predict_kernel<T, 2, R2>, the direct launch_kbuild,
pair_kernel_kernel, leaf_value / leaf_grad with pslot == 1, the direct LML gradient, the direct
branch of refine_f32 and model_append's tabNew / tabLead tables.  The trees below reach each of
them, the limits themselves (eight leaves, sixteen terms) and the three refusals beyond them.

Tolerances are those of the existing tests of the same entry point (tests/test_gpu_parity.py,
test_gpu_append.py, test_gpu_sparse.py, test_gpu_sparse_lml.py, test_gpu_dist.py).  Every tree has
cond(K + sigma^2 I) <= 2e3 at sigma = 0.5 on make_data(300, 3) (test_fixture_trees, CPU)."""
import numpy as np
import pytest

from gpr_amd import kernels as kn
from oracle import oracle as O
from tests.helpers import make_data, make_queries, relerr, TOL

gpu = pytest.mark.gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = [np.float64, np.float32]


def _sum(*ks):
    """Left-nested SumKernel of the given nodes."""
    node = ks[0]
    for k in ks[1:]:
        node = kn.Sum(node, k)
    return node


_P1, _P2 = kn.Periodic(0.9, 2.5, 0.8), kn.Periodic(0.5, 1.3, 1.1)
NODES = {
    # NPER = 2, R2 = false
    "2per_sum": kn.Sum(_P1, _P2),
    # NPER = 2, R2 = true
    "2per_sum_gauss": kn.Sum(kn.Sum(kn.Gaussian(0.7, 1.3), _P1), _P2),
    "2per_prod": kn.Product(_P1, _P2),
    "2per_prod_gauss": kn.Product(kn.Gaussian(1.5, 1), kn.Product(kn.Periodic(1, 1.3, 0.9),
                                                                  kn.Periodic(0.8, 2.1, 1.2))),
    "2per_white": kn.Sum(kn.Sum(_P1, _P2), kn.White(0.3)),
    # every leaf type, two periodic leaves (the second one is the fifth leaf), one White, and both
    # branches of the rational quadratic leaf (alpha = 1 and alpha != 1)
    "8leaf_sum": _sum(kn.Gaussian(0.7, 0.5), kn.Periodic(0.4, 2.5, 0.8), kn.RationalQuadratic(0.5, 0.6, 1.5),
                      kn.GaussianExp(-0.3, -0.8), kn.Periodic(0.3, 1.3, 1.1), kn.Gaussian(1.6, 0.4),
                      kn.RationalQuadratic(0.4, 1.2, 1.0), kn.White(0.3)),
    # eight leaves and 2 * 2 * 2 * 2 = 16 product terms: both limits at once
    "16term": kn.Product(
        kn.Product(kn.Sum(kn.Gaussian(0.9, 0.8), kn.RationalQuadratic(0.6, 0.7, 1.5)),
                   kn.Sum(kn.Gaussian(1.4, 0.7), kn.Periodic(0.8, 2.5, 0.8))),
        kn.Product(kn.Sum(kn.GaussianExp(-0.2, -0.3), kn.Gaussian(2.0, 0.6)),
                   kn.Sum(kn.Periodic(0.7, 1.3, 1.1), kn.Gaussian(1.1, 0.9)))),
}
TREES = {name: node.to_string() for name, node in NODES.items()}
NAMES = list(TREES)
SUMS = ["2per_sum", "2per_sum_gauss", "2per_white"]  # the trees that also go through append, LU, sparse, sharded

# beyond the device form (canonicalize's three refusals)
_G = kn.Gaussian(0.7, 1.3)
_S3 = _sum(kn.Gaussian(0.7, 1.0), kn.Gaussian(1.1, 0.8), kn.RationalQuadratic(0.5, 0.6, 1.5))
REFUSED = {
    "3per": (_sum(_P1, _P2, kn.Periodic(0.7, 1.9, 1.0)), "at most 2 periodic leaves on the device"),
    "9leaf": (_sum(*[kn.Gaussian(0.5 + 0.1 * i, 0.4) for i in range(9)]), "too many leaf kernels for the device form"),
    # eight leaves, 3 * 3 * 2 = 18 terms
    "18term": (kn.Product(kn.Product(_S3, _S3), kn.Sum(_G, kn.Gaussian(1.7, 0.5))),
               "too many product terms for the device form"),
}
ARG = 8  # GPRX_ERR_ARG

SIGMA = 0.5
_refs = {}


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def oracle_fit(name, n, d, m, sigma=SIGMA):
    """(X, Y, alpha, C, log det) of the oracle on make_data(n, d, m), computed once and read-only."""
    key = ("fit", name, n, d, m, sigma)
    if key not in _refs:
        X, Y = make_data(n, d, m)
        a, C = O.fit(TREES[name], X, Y, sigma)
        ld = np.linalg.slogdet(O.kernel_matrix(TREES[name], X) + sigma * sigma * np.eye(n))[1]
        _refs[key] = _ro(X, Y, a, C, ld)
    return _refs[key]


def oracle_lml(name, n, d, sigma, dtype=np.float64):
    key = ("lml", name, n, d, sigma, np.dtype(dtype))
    if key not in _refs:
        X, Y = make_data(n, d)
        X, Y = X.astype(dtype), Y.astype(dtype)
        v, g, _, ld = O.lml(TREES[name], X, Y, sigma, dtype)
        _refs[key] = _ro(X, Y, float(v), np.asarray(g, np.float64), ld)
    return _refs[key]


def fitted(ctx, ks, X, Y, dtype=np.float64, sigma=SIGMA, flags=0):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X.astype(dtype), Y.astype(dtype))
    M.set_kernel(ks)
    M.set_noise(sigma)
    return M, M.fit(flags)


# ---------------------------------------------------------------------------------------
# the fixtures themselves (CPU)
# ---------------------------------------------------------------------------------------
def _leaf(node, x, y):
    r2 = float(np.sum((x - y) ** 2))
    p = node.params
    if node.name == "GaussianKernel":
        return p[1] ** 2 * np.exp(-0.5 * r2 / p[0] ** 2)
    if node.name == "GaussianExpKernel":
        return np.exp(p[1]) ** 2 * np.exp(-0.5 * r2 / np.exp(p[0]) ** 2)
    if node.name == "WhiteKernel":
        return p[0] ** 2 if r2 == 0 else 0.0
    if node.name == "RationalQuadraticKernel":
        return p[0] ** 2 * (1 + 0.5 * r2 / (p[1] ** 2 * p[2])) ** (-p[2])
    s = float(np.sum(np.sin(p[1] * (x - y)) ** 2))
    return p[0] ** 2 * np.exp(-0.5 * s / p[2] ** 2)


def _eval(node, x, y):
    if node.is_leaf:
        return _leaf(node, x, y)
    a, b = _eval(node.k1, x, y), _eval(node.k2, x, y)
    return a + b if node.name == "SumKernel" else a * b


def _shape(node):
    """(leaves, product terms, periodic leaves) of a tree."""
    if node.is_leaf:
        return 1, 1, int(node.name == "PeriodicKernel")
    (l1, t1, p1), (l2, t2, p2) = _shape(node.k1), _shape(node.k2)
    return l1 + l2, (t1 + t2 if node.name == "SumKernel" else t1 * t2), p1 + p2


def test_fixture_trees():
    """The strings mean the trees they were built from (the oracle parses them on its own: its
    value at a few pairs against a numpy evaluation of the node tree), the trees sit where the
    module says they do (leaf, term and periodic-leaf counts), and K + sigma^2 I is well inside
    1 / tolerance for every fit below."""
    X, _ = make_data(12, 3)
    for name, node in NODES.items():
        assert kn.parse_kernel(TREES[name]).to_string() == TREES[name]
        assert O.kernel_nparams(TREES[name]) == node.num_params()
        for i, j in [(0, 0), (0, 1), (3, 7), (11, 2)]:
            v = O.kernel_eval(TREES[name], X[i], X[j], with_grad=False)
            assert abs(v - _eval(node, X[i], X[j])) <= 1e-14 * max(1.0, abs(v)), (name, i, j)
        assert _shape(node)[2] == 2, name
    assert _shape(NODES["8leaf_sum"]) == (8, 8, 2)
    assert _shape(NODES["16term"]) == (8, 16, 2)
    assert _shape(REFUSED["3per"][0])[2] == 3
    assert _shape(REFUSED["9leaf"][0])[0] == 9
    assert _shape(REFUSED["18term"][0]) == (8, 18, 0)
    for n, d in [(300, 3), (300, 5)]:
        X, _ = make_data(n, d)
        for name in NAMES:
            K = O.kernel_matrix(TREES[name], X) + SIGMA * SIGMA * np.eye(n)
            assert np.linalg.cond(K) <= 2e3, (name, n, d)


# ---------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [(1, 1), (77, 3), (200, 33)])
def test_kernel_matrix(ctx, name, dtype, n, d):
    X, _ = make_data(n, d, dtype=dtype)
    K = ctx.kernel_matrix(TREES[name], X, dtype)
    R = O.kernel_matrix(TREES[name], X, dtype)
    assert relerr(K, R) <= (1e-12 if dtype == np.float64 else 2e-5)
    assert np.array_equal(K, K.T)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_deriv_matrix(ctx, name):
    """Per parameter: a leaf that read the other periodic leaf's statistics (pslot, f0 / f1) is
    wrong in its own three slabs only."""
    X, _ = make_data(50, 4)
    D = ctx.deriv_matrix(TREES[name], X)
    R = O.deriv_matrix(TREES[name], X)
    assert D.shape == R.shape
    for p in range(R.shape[0]):
        e = relerr(D[p], R[p])
        print(f"deriv_matrix {name} p={p}: {e:.3e}")
        assert e <= 1e-10, p


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_cross_matrix(ctx, name):
    A, _ = make_data(70, 5)
    B = make_queries(45, 5)
    assert relerr(ctx.cross_matrix(TREES[name], A, B), O.cross_matrix(TREES[name], A, B)) <= 1e-12


@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("path", [0, 1])
def test_build_matrix_refused(ctx, name, path):
    """The MFMA pair-statistics build carries one periodic leaf at most: both of its paths refuse
    these trees with GPRX_ERR_ARG and point at the direct build."""
    import gpr_amd
    X, _ = make_data(260, 5)
    with pytest.raises(gpr_amd.GprxError) as e:
        ctx.build_matrix(TREES[name], X, 0.4, path)
    assert e.value.status == ARG and "the tree takes the direct (VALU) build" in str(e.value)


# ---------------------------------------------------------------------------------------
# fit, predict, posterior, LML
# ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fit_predict(ctx, name, dtype):
    """Three 128-blocks, three ragged query blocks, derivatives; the fp32 fit is refined through
    refine_f32's direct branch."""
    n, d, m, q = 300, 3, 2, 130
    ks = TREES[name]
    X, Y, a_ref, _, ld_ref = oracle_fit(name, n, d, m)
    tol = TOL[np.dtype(dtype)]
    M, info = fitted(ctx, ks, X, Y, dtype)
    assert info.method == 0
    Xq = make_queries(q, d)
    mean, D = M.predict(Xq.astype(dtype), deriv=True)
    mr, Dr = O.predict(ks, X, a_ref, Xq, np.float64, with_deriv=True)
    errs = relerr(M.alpha(), a_ref), relerr(mean, mr), relerr(D, Dr)
    print(f"fit {name} {np.dtype(dtype).name}: alpha {errs[0]:.3e} mean {errs[1]:.3e} deriv {errs[2]:.3e}")
    assert errs[0] <= tol and errs[1] <= tol and errs[2] <= tol
    assert relerr(M.predict(Xq.astype(dtype)), mr) <= tol  # (the mean-only call)
    assert abs(info.logdet - ld_ref) <= (1e-8 if dtype == np.float64 else 1e-3) * max(1, abs(info.logdet))
    M.close()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_posterior_cov(ctx, name):
    n, d, sigma = 300, 3, 0.3
    ks = TREES[name]
    X, Y, _, C_ref, _ = oracle_fit(name, n, d, 1, sigma)
    M, _ = fitted(ctx, ks, X, Y, sigma=sigma)
    Xa = make_queries(40, d)
    for Xb in (Xa, Xa[::-1].copy()):
        c = M.posterior_cov(Xa, Xb)
        c_ref = O.posterior_cov(ks, X, C_ref, Xa, Xb)
        kab = np.array([O.kernel_eval(ks, a, b, with_grad=False) for a, b in zip(Xa, Xb)])
        # the covariance is a difference of O(1) terms: compare on the scale of k(x,y)
        assert np.max(np.abs(c - c_ref)) <= 1e-6 * max(1.0, np.max(np.abs(kab)))
    assert relerr(M.core_matrix(), C_ref) <= 1e-6
    M.close()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_posterior_cov_f32(ctx, name):
    """fp32 variances at queries within 1e-3 of training samples, and pairs x != y, against the
    oracle's fp32 path at the fp32 bar on the scale of k(x,x)
    (tests/test_gpu_parity.py test_posterior_variance_f32_near_training_points)."""
    n, d, sigma = 300, 3, 0.3
    ks = TREES[name]
    X, Y = make_data(n, d)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    M, _ = fitted(ctx, ks, X32, Y32, np.float32, sigma)
    _, C_ref = O.fit(ks, X32, Y32, sigma, np.float32)
    rng = np.random.default_rng(7)
    Xa = (X32[rng.choice(n, 64, replace=False)] + 1e-3 * rng.standard_normal((64, d))).astype(np.float32)
    kaa = max(abs(O.kernel_eval(ks, a, a, with_grad=False)) for a in Xa.astype(np.float64))
    for Xb in (Xa, Xa[::-1].copy()):
        c = M.posterior_cov(Xa, Xb)
        c_ref = O.posterior_cov(ks, X32, C_ref, Xa, Xb, np.float32)
        assert np.max(np.abs(c - c_ref)) <= TOL[F32] * max(1.0, kaa)
    M.close()


@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n,d,sigma", [(150, 2, 0.4), (300, 5, 0.7)])
def test_lml(ctx, name, n, d, sigma):
    """The direct LML gradient (k_lml.hip) on one tile pair and on several ragged ones."""
    X, Y, vr, gr, ldr = oracle_lml(name, n, d, sigma)
    M, _ = fitted(ctx, TREES[name], X, Y, sigma=sigma)
    v, g, logdet = M.lml(grad=True)
    e = relerr(g, gr)
    print(f"lml {name} n={n}: value {abs(v - vr) / max(1.0, abs(vr)):.3e} grad {e:.3e}")
    assert abs(v - vr) <= 1e-6 * max(1.0, abs(vr))
    assert abs(logdet - ldr) <= 1e-8 * max(1.0, abs(ldr))
    assert g.shape == gr.shape and e <= 1e-6
    vc, _, _ = M.lml(grad=False, compat=True)
    assert abs(vc - vr) <= 1e-6 * max(1.0, abs(vr))
    M.close()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_lml_f32(ctx, name):
    n, d, sigma = 300, 4, 0.7
    X, Y, vr, gr, _ = oracle_lml(name, n, d, sigma)
    M, _ = fitted(ctx, TREES[name], X, Y, np.float32, sigma)
    v, g, _ = M.lml(grad=True)
    assert abs(v - vr) <= 1e-3 * max(1.0, abs(vr))
    assert relerr(g, gr) <= 1e-3
    M.close()


# ---------------------------------------------------------------------------------------
# the sums of two periodic leaves through the other entry points
# ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", SUMS)
@pytest.mark.parametrize("n,k", [(300, 1), (300, 100)])
@pytest.mark.parametrize("gemm", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_append(ctx, dtype, gemm, n, k, name):
    """model_append's tables of the three sample ranges (tabAct, tabNew, tabLead: 2 * nper planes
    each), inside the padding and with the re-layout."""
    from gpr_amd import gprx
    d, m = 3, 2
    ks = TREES[name]
    X, Y, a_ref, _, ld_ref = oracle_fit(name, n + k, d, m)
    tol = TOL[np.dtype(dtype)]
    M, _ = fitted(ctx, ks, X[:n], Y[:n], dtype)
    info = M.append(X[n:].astype(dtype), Y[n:].astype(dtype), gprx.APPEND_SOLVE_GEMM if gemm else 0)
    assert info.appended == k and info.method == 0
    assert M.n == n + k and M.alpha().shape == (n + k, m)
    assert relerr(M.alpha(), a_ref) <= tol
    Xq = make_queries(64, d)
    mean, D = M.predict(Xq.astype(dtype), deriv=True)  # (the direct predict reads the model's new tables)
    mr, Dr = O.predict(ks, X, a_ref, Xq, with_deriv=True)
    assert relerr(mean, mr) <= tol and relerr(D, Dr) <= tol
    assert abs(info.logdet - ld_ref) <= (1e-8 if dtype == np.float64 else 1e-3) * max(1, abs(info.logdet))
    M.close()


@gpu
@pytest.mark.parametrize("name", SUMS)
def test_forced_lu(ctx, name):
    from gpr_amd import gprx
    n, d, m = 300, 3, 2
    ks = TREES[name]
    X, Y, a_ref, C_ref, ld_ref = oracle_fit(name, n, d, m)
    M, info = fitted(ctx, ks, X, Y, flags=gprx.FIT_FORCE_LU)
    assert info.method == 1
    assert relerr(M.alpha(), a_ref) <= 1e-6
    Xq = make_queries(64, d)
    assert relerr(M.predict(Xq), O.predict(ks, X, a_ref, Xq)) <= 1e-6
    assert abs(info.logdet - ld_ref) <= 1e-8 * max(1.0, abs(ld_ref))
    cov = M.posterior_cov(Xq, Xq[::-1].copy())
    cov_ref = O.posterior_cov(ks, X, C_ref, Xq, Xq[::-1].copy())
    assert np.max(np.abs(cov - cov_ref)) <= 1e-6 * max(1.0, np.max(np.abs(cov_ref)))
    M.close()


def _sparse_inputs(n, d, M, m):
    X, Y = make_data(n, d, m)
    return X, Y, X[:: n // M][:M].copy()


@gpu
@pytest.mark.parametrize("name", SUMS)
@pytest.mark.parametrize("chunk", [None, 64])
def test_sparse_fit(ctx, monkeypatch, name, chunk):
    if chunk:
        monkeypatch.setenv("GPRX_SPARSE_CHUNK", str(chunk))
    ks, sigma, jitter = TREES[name], 0.5, 1e-4
    X, Y, Xm = _sparse_inputs(700, 3, 40, 2)
    Kinv, RV, RM = ctx.sparse_fit(ks, X, Y, Xm, sigma, jitter)
    Ki_r, RV_r, RM_r = O.sparse_fit(ks, X, Y, Xm, sigma, jitter)
    assert relerr(Kinv, Ki_r) <= TOL[F64]
    assert relerr(RV, RV_r) <= TOL[F64]
    assert relerr(RM, RM_r) <= TOL[F64]


@gpu
@pytest.mark.parametrize("name", SUMS)
@pytest.mark.parametrize("chunk", [None, 128])
def test_sparse_lml(ctx, monkeypatch, name, chunk):
    if chunk:
        monkeypatch.setenv("GPRX_SPARSE_CHUNK", str(chunk))
    ks, sigma, jitter = TREES[name], 0.5, 1e-3
    X, Y, Xm = _sparse_inputs(600, 3, 40, 1)
    v, g, ld = ctx.sparse_lml(ks, X, Y[:, 0], Xm, sigma, jitter)
    vr, gr, _, ld_r = O.sparse_lml(ks, X, Y[:, 0], Xm, sigma, jitter)
    assert abs(v - vr) <= TOL[F64] * max(1.0, abs(vr)), (v, vr)
    assert abs(ld - ld_r) <= TOL[F64] * max(1.0, abs(ld_r)), (ld, ld_r)
    assert g.shape == gr.shape
    assert relerr(g, gr) <= TOL[F64], (g, gr)


@gpu
@pytest.mark.parametrize("name", SUMS)
def test_sharded_fit(name):
    """Two virtual ranks: the sharded engine builds its tiles with the direct kernel."""
    import gpr_amd
    n, d, m = 700, 5, 1
    ks = TREES[name]
    X, Y, a_ref, _, ld_ref = oracle_fit(name, n, d, m)
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        M, info = fitted(vctx, ks, X, Y)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        Xq = make_queries(50, d)
        assert relerr(M.predict(Xq), O.predict(ks, X, a_ref, Xq)) <= 1e-6
        assert abs(info.logdet - ld_ref) <= 1e-9 * max(1.0, abs(info.logdet))
        df_ref = float(np.sum(Y * a_ref))
        assert abs(info.datafit - df_ref) <= 1e-8 * abs(df_ref)
        M.close()
    finally:
        vctx.close()


# ---------------------------------------------------------------------------------------
# beyond the limits
# ---------------------------------------------------------------------------------------
@gpu
def test_refusals(ctx):
    """A third periodic leaf, a ninth leaf, eighteen product terms: GPRX_ERR_ARG with
    canonicalize's message from set_kernel and from kernel_matrix, and the context and the model
    go on working."""
    import gpr_amd
    n, d = 100, 3
    X, Y, a_ref, _, _ = oracle_fit("2per_sum_gauss", n, d, 1)
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X, Y)
    M.set_noise(SIGMA)
    for key, (node, msg) in REFUSED.items():
        ks = node.to_string()
        with pytest.raises(gpr_amd.GprxError) as e:
            M.set_kernel(ks)
        assert e.value.status == ARG and msg in str(e.value), key
        with pytest.raises(gpr_amd.GprxError) as e:
            ctx.kernel_matrix(ks, X)
        assert e.value.status == ARG and msg in str(e.value), key
    M.set_kernel(TREES["2per_sum_gauss"])
    M.fit()
    assert relerr(M.alpha(), a_ref) <= 1e-6
    M.close()
