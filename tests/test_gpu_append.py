"""gprx_model_append (Model.append): samples added to a fitted model by extending its Cholesky
factor, against the CPU oracle's fit of the concatenated data.

make_data(n + k, d, m)[:n] equals make_data(n, d, m), so every test fits a prefix and appends
the rest.  Tolerances are the fit's own (tests/helpers.TOL, tests/test_gpu_parity.py)."""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import make_data, make_queries, relerr, TOL
from tests.test_gpu_parity import KERNELS

pytestmark = pytest.mark.gpu

SIGMA = 0.5
INDEF = "RationalQuadraticKernel(1.2,2,-1,)"  # tests/test_gpu_lu.py: K + sigma^2 I indefinite
SHAPES = [
    (300, 1, 3, 2),    # fits in the padding
    (300, 100, 3, 2),  # np grows 384 -> 512: re-layout
    (256, 1, 3, 1),    # t = 0: a new block
    (100, 5, 2, 1),    # n0 = 0: no panel solve
    (128, 128, 4, 1),
    (200, 700, 5, 1),  # k > 128: several new blocks
    (640, 17, 3, 3),   # five chained blocks, rows padded 17 -> 32
    (1100, 3, 2, 1),   # eight leading blocks: the Schur update of the one trailing block is split over K
]
_refs = {}


def oracle_fit(ks, n, d, m, sigma=SIGMA):
    """(X, Y, alpha, C, log det) of the oracle on make_data(n, d, m), computed once."""
    key = (ks, n, d, m, sigma)
    if key not in _refs:
        X, Y = make_data(n, d, m)
        a, C = O.fit(ks, X, Y, sigma)
        ld = np.linalg.slogdet(O.kernel_matrix(ks, X) + sigma * sigma * np.eye(n))[1]
        for v in (X, Y, a, C):
            v.setflags(write=False)
        _refs[key] = (X, Y, a, C, ld)
    return _refs[key]


def fitted(ctx, ks, X, Y, dtype=np.float64, sigma=SIGMA, flags=0):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X.astype(dtype), Y.astype(dtype))
    M.set_kernel(ks)
    M.set_noise(sigma)
    return M, M.fit(flags)


@pytest.mark.parametrize("ks", [KERNELS[0], KERNELS[4], KERNELS[6], KERNELS[2]])
@pytest.mark.parametrize("n,k,d,m", SHAPES)
@pytest.mark.parametrize("gemm", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_append_parity(ctx, dtype, gemm, n, k, d, m, ks):
    from gpr_amd import gprx
    X, Y, a_ref, _, ld_ref = oracle_fit(ks, n + k, d, m)
    tol = TOL[np.dtype(dtype)]
    M, _ = fitted(ctx, ks, X[:n], Y[:n], dtype)
    info = M.append(X[n:].astype(dtype), Y[n:].astype(dtype), gprx.APPEND_SOLVE_GEMM if gemm else 0)
    assert info.appended == k and info.method == 0
    assert M.n == n + k and M.alpha().shape == (n + k, m)
    assert relerr(M.alpha(), a_ref) <= tol
    Xq = make_queries(64, d)
    assert relerr(M.predict(Xq.astype(dtype)), O.predict(ks, X, a_ref, Xq)) <= tol
    assert abs(info.logdet - ld_ref) <= (1e-8 if dtype == np.float64 else 1e-3) * max(1, abs(info.logdet))
    M.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_repeated_appends_cross_a_block_boundary(ctx, dtype):
    ks, d, m = KERNELS[4], 3, 2
    X, Y, a_ref, _, _ = oracle_fit(ks, 260, d, m)
    M, _ = fitted(ctx, ks, X[:250], Y[:250], dtype)
    for i in range(250, 260):
        info = M.append(X[i:i + 1].astype(dtype), Y[i:i + 1].astype(dtype))
        assert info.appended == 1
        assert M.alpha().shape[0] == i + 1
    assert relerr(M.alpha(), a_ref) <= TOL[np.dtype(dtype)]
    M.close()


@pytest.mark.parametrize("ks", [KERNELS[0], KERNELS[4]])
def test_posterior_after_append(ctx, ks):
    n, k, d, sigma = 300, 20, 3, 0.3
    X, Y, _, C_ref, _ = oracle_fit(ks, n + k, d, 1, sigma)
    M, _ = fitted(ctx, ks, X[:n], Y[:n], sigma=sigma)
    assert M.append(X[n:], Y[n:]).appended == k
    Xa = make_queries(40, d)
    for Xb in (Xa, Xa[::-1].copy()):
        c = M.posterior_cov(Xa, Xb)
        c_ref = O.posterior_cov(ks, X, C_ref, Xa, Xb)
        kab = np.array([O.kernel_eval(ks, a, b, with_grad=False) for a, b in zip(Xa, Xb)])
        assert np.max(np.abs(c - c_ref)) <= 1e-6 * max(1.0, np.max(np.abs(kab)))
    assert relerr(M.core_matrix(), C_ref) <= 1e-6
    M.close()


@pytest.mark.parametrize("ks", [KERNELS[0], KERNELS[4]])
def test_lml_after_append(ctx, ks):
    n, k, d, sigma = 150, 30, 2, 0.4
    X, Y = make_data(n + k, d)
    M, _ = fitted(ctx, ks, X[:n], Y[:n], sigma=sigma)
    assert M.append(X[n:], Y[n:]).appended == k
    v, g, logdet = M.lml(grad=True)
    vr, gr, _, ldr = O.lml(ks, X, Y, sigma)
    assert abs(v - vr) <= 1e-6 * max(1.0, abs(vr))
    assert abs(logdet - ldr) <= 1e-8 * max(1.0, abs(ldr))
    assert relerr(g, gr) <= 1e-6
    M.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_refit_equivalence(ctx, dtype):
    ks, n, k, d, m = KERNELS[4], 300, 100, 3, 2
    X, Y, a_ref, _, _ = oracle_fit(ks, n + k, d, m)
    tol = TOL[np.dtype(dtype)]
    M, _ = fitted(ctx, ks, X[:n], Y[:n], dtype)
    assert M.append(X[n:].astype(dtype), Y[n:].astype(dtype)).appended == k
    a_app = M.alpha()
    info = M.fit()
    assert info.appended == 0 and M.n == n + k
    a_fit = M.alpha()
    assert relerr(a_app, a_ref) <= tol and relerr(a_fit, a_ref) <= tol
    assert relerr(a_fit, a_app) <= 2 * tol
    M.close()


def test_append_to_forced_lu_model_refits(ctx):
    from gpr_amd import gprx
    ks, n, k, d, m = KERNELS[0], 300, 7, 3, 2
    X, Y, a_ref, _, _ = oracle_fit(ks, n + k, d, m)
    M, info = fitted(ctx, ks, X[:n], Y[:n], flags=gprx.FIT_FORCE_LU)
    assert info.method == 1
    info = M.append(X[n:], Y[n:])
    assert info.appended == 0 and info.method == 1
    assert M.n == n + k and relerr(M.alpha(), a_ref) <= TOL[np.dtype(np.float64)]
    M.close()


def test_append_that_loses_definiteness_falls_back_to_lu(ctx):
    """tests/test_gpu_lu.py's indefinite fixture (n = 260) with its last 10 rows withheld: the
    250-row prefix is positive definite (min eigenvalue 1.9e-3), all 260 rows are not (-3.6e-3).
    The trailing Cholesky of the update meets a non-positive pivot: a documented error path on
    valid input, answered by the full refit and its LU fallback."""
    import gpr_amd
    from gpr_amd import gprx
    n, k, d, sigma = 250, 10, 3, 0.3
    X, Y = make_data(n + k, d, 1)
    K = O.kernel_matrix(INDEF, X) + sigma * sigma * np.eye(n + k)
    assert np.linalg.eigvalsh(K[:n, :n])[0] > 0 > np.linalg.eigvalsh(K)[0]
    M, info = fitted(ctx, INDEF, X[:n], Y[:n], sigma=sigma)
    assert info.method == 0
    info = M.append(X[n:], Y[n:])
    assert info.appended == 0 and info.method == 1 and info.info > 0
    a_ref, C_ref = O.fit(INDEF, X, Y, sigma)
    assert relerr(M.alpha(), a_ref) <= 1e-6
    Xq = make_queries(64, d)
    assert relerr(M.predict(Xq), O.predict(INDEF, X, a_ref, Xq)) <= 1e-6
    assert abs(info.logdet - np.linalg.slogdet(K)[1]) <= 1e-9 * max(1.0, abs(info.logdet))
    assert relerr(M.core_matrix(), C_ref) <= 1e-6
    M.close()
    M, _ = fitted(ctx, INDEF, X[:n], Y[:n], sigma=sigma)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.append(X[n:], Y[n:], gprx.FIT_NO_LU_FALLBACK)
    assert e.value.status == 2  # NOT_SPD
    M.close()


def test_refusals(ctx):
    import gpr_amd
    ks, n, d, m = KERNELS[0], 200, 3, 1
    X, Y = make_data(n + 4, d, m)
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X[:n], Y[:n])
    M.set_kernel(ks)
    M.set_noise(SIGMA)
    with pytest.raises(gpr_amd.GprxError) as e:  # before any fit
        M.append(X[n:], Y[n:])
    assert e.value.status == 9 and "not initialized" in str(e.value)
    M.fit()
    with pytest.raises(gpr_amd.GprxError) as e:
        M.append(X[n:n], Y[n:n])  # k = 0
    assert e.value.status == 8
    with pytest.raises(gpr_amd.GprxError) as e:
        M.append(np.zeros((2, d + 1)), np.zeros((2, m)))
    assert e.value.status in (4, 8)
    a0 = M.alpha()
    M.set_kernel(lambda A, B: O.cross_matrix(ks, A, B))  # a caller-evaluated kernel (set_kernel_matrix)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.append(X[n:], Y[n:])
    assert e.value.status == 9
    assert M.n == n
    M.set_kernel(ks)
    M.fit()
    assert np.array_equal(M.alpha(), a0)
    M.close()


def test_refused_on_a_sharded_context():
    """No distributed kernel runs: the model is not even fitted."""
    import gpr_amd
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        X, Y = make_data(204, 3, 1)
        M = gpr_amd.Model(vctx, np.float64)
        M.set_data(X[:200], Y[:200])
        M.set_kernel(KERNELS[0])
        M.set_noise(SIGMA)
        with pytest.raises(gpr_amd.GprxError) as e:
            M.append(X[200:], Y[200:])
        assert e.value.status == 9 and "sharded" in str(e.value)
        M.close()
    finally:
        vctx.close()


@pytest.mark.parametrize("n", [300, 380])
def test_nonfinite_new_sample_leaves_the_model_as_it_was(ctx, n):
    """n = 300: the update would fit in the padding (the factor's partial block is restored);
    n = 380: it would re-lay the factor (the new buffers are dropped)."""
    import gpr_amd
    ks, k, d, m = KERNELS[0], 10, 3, 2
    X, Y, a_ref, _, _ = oracle_fit(ks, n, d, m)
    Xn, Yn = make_data(n + k, d, m)
    Xn, Yn = Xn[n:].copy(), Yn[n:].copy()
    Xn[k // 2, 1] = np.nan
    M, _ = fitted(ctx, ks, X, Y)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.append(Xn, Yn)
    assert e.value.status == 1 and "not finite" in str(e.value)
    assert M.n == n and M.alpha().shape == (n, m)
    assert relerr(M.alpha(), a_ref) <= 1e-6
    Xq = make_queries(64, d)
    assert relerr(M.predict(Xq), O.predict(ks, X, a_ref, Xq)) <= 1e-6
    # the factor too: the variance, and a later valid append
    _, C_ref = O.fit(ks, X, Y, SIGMA)
    c = M.posterior_cov(Xq, Xq)
    assert np.max(np.abs(c - O.posterior_cov(ks, X, C_ref, Xq, Xq))) <= 1e-6
    X2, Y2, a2, _, _ = oracle_fit(ks, n + k, d, m)
    assert M.append(X2[n:], Y2[n:]).appended == k
    assert relerr(M.alpha(), a2) <= 1e-6
    M.close()


@pytest.mark.parametrize("n,k", [(300, 5), (380, 10)])
def test_device_inputs_give_the_same_bits(ctx, n, k):
    ks, d, m = KERNELS[4], 3, 2
    X, Y = make_data(n + k, d, m)
    Mh, _ = fitted(ctx, ks, X[:n], Y[:n])
    Md, _ = fitted(ctx, ks, X[:n], Y[:n])
    Mh.append(X[n:], Y[n:])
    Md.append(ctx.device_array(X[n:]), ctx.device_array(Y[n:]))
    assert np.array_equal(Mh.alpha(), Md.alpha())
    Mh.close()
    Md.close()


def test_predict_from_four_threads_during_an_append(ctx):
    """tests/cpp/gp_host_test.cpp's PosteriorProcessTest scenario at n = 300: four threads predict
    while one appends; every mean is the pre-append or the post-append model's."""
    ks, n, k, d, m = KERNELS[0], 300, 40, 3, 2
    X, Y, a1, _, _ = oracle_fit(ks, n + k, d, m)
    _, _, a0, _, _ = oracle_fit(ks, n, d, m)
    Xq = make_queries(16, d)
    before, after = O.predict(ks, X[:n], a0, Xq), O.predict(ks, X, a1, Xq)
    M, _ = fitted(ctx, ks, X[:n], Y[:n])
    tol = TOL[np.dtype(np.float64)]
    bad, done = [], threading.Event()

    def reader():
        try:
            for it in range(200):
                mean = M.predict(Xq)
                if relerr(mean, before) > tol and relerr(mean, after) > tol:
                    bad.append((it, relerr(mean, before), relerr(mean, after)))
                if done.is_set() and it >= 8:
                    break
        except Exception as ex:  # noqa: BLE001
            bad.append(repr(ex))

    th = [threading.Thread(target=reader) for _ in range(4)]
    for t in th:
        t.start()
    info = M.append(X[n:], Y[n:])
    done.set()
    for t in th:
        t.join(120)
    assert info.appended == k and not bad, bad
    assert relerr(M.predict(Xq), after) <= tol
    M.close()
