"""gprx_model_posterior / gprx_model_sample / gprx_dev_normals (Model.posterior, Model.sample,
Context.normals; k_sample.hip) against the numpy restatement (tests/sample_ref.py).  Tolerances
are the project's (tests/helpers.TOL, normwise relative: 1e-6 in f64, 1e-3 in f32); the generator's
own bound is worked out at its test.  Inputs are make_data / make_queries; sigma >= 0.5 keeps
cond(K + sigma^2 I) far inside 1 / tol, and at these shapes the joint covariance is 7-27 % of the
prior's magnitude, so its comparison is not dominated by cancellation."""
import numpy as np
import pytest

from tests import loo_ref as L
from tests import sample_ref as S
from tests.helpers import make_data, make_queries, relerr, TOL

pytestmark = pytest.mark.gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
SHAPES = [(100, 1, 3), (128, 128, 3), (129, 129, 3), (777, 300, 5), (777, 127, 5)]  # (n, q, d)
TREES = ["c3", "matern32", "rq_gaussexp", "product"]  # (the product tree: the VALU cross build)
_refs = {}


def reference(ks, n, q, d, m, sigma):
    """(X, Y, Xq, mean, Sigma, max prior diagonal) of the restatement, computed once."""
    key = (ks, n, q, d, m, sigma)
    if key not in _refs:
        X, Y = make_data(n, d, m)
        Xq = make_queries(q, d)
        mean, Sigma = S.posterior(ks, X, Y, Xq, sigma)
        Kqq, _ = L.matrices(ks, Xq)
        out = (X, Y, Xq, mean, Sigma, float(np.max(np.diag(Kqq))))
        for a in out[:5]:
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def model(ctx, ks, X, Y, sigma, dtype=np.float64, fit=True, flags=0):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(np.asarray(X, dtype), np.asarray(Y, dtype))
    M.set_kernel(ks)
    M.set_noise(sigma)
    if fit:
        M.fit(flags)
    return M


# ---- the generator ------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 257, 65537])
def test_normals(ctx, count):
    """fp64 within 1e-12 absolute of the restatement: the device's log, sin and cos are a few ulp
    from the C library's and |z| < 9, so the difference is ~1e-15; a wrong bit anywhere in the
    integer part gives an unrelated number.  fp32 is that number rounded once: within one float
    spacing of float32(ref)."""
    ref = S.normals(20240607, count)
    z = ctx.normals(20240607, count)
    assert z.dtype == np.float64 and z.shape == (count,)
    print(f"normals count={count}: f64 max abs diff {np.max(np.abs(z - ref)):.2e}")
    assert np.max(np.abs(z - ref)) <= 1e-12
    z32 = ctx.normals(20240607, count, np.float32)
    r32 = ref.astype(np.float32)
    assert z32.dtype == np.float32 and z32.shape == (count,)
    assert np.all(np.abs(z32.astype(np.float64) - r32.astype(np.float64)) <= np.spacing(np.abs(r32)).astype(np.float64))
    assert not np.array_equal(ctx.normals(20240608, count), z)


# ---- the joint posterior ------------------------------------------------------------------
def check_posterior(M, ks, sigma, Xq, mean_ref, Sigma_ref, tol, what):
    mean, cov = M.posterior(Xq)
    q = Xq.shape[0]
    var = M.posterior_cov(Xq, Xq)
    _, noisy = M.posterior(Xq, noise=True)
    s2 = np.asarray(sigma, M.dtype) ** 2
    print(f"posterior {what}: cov {relerr(cov, Sigma_ref):.2e}, mean {relerr(mean, mean_ref):.2e}, "
          f"diag vs posterior_cov {relerr(np.diag(cov), var):.2e}, "
          f"noise {relerr(noisy, cov + s2 * np.eye(q)):.2e}")
    assert mean.shape == mean_ref.shape and cov.shape == (q, q) and mean.dtype == M.dtype and cov.dtype == M.dtype
    assert relerr(cov, Sigma_ref) <= tol
    assert np.array_equal(cov, cov.T)
    assert np.array_equal(mean, M.predict(Xq))
    assert relerr(mean, mean_ref) <= tol
    assert relerr(np.diag(cov), var) <= tol
    assert relerr(noisy, cov + s2 * np.eye(q)) <= tol
    return mean, cov


@pytest.mark.parametrize("n,q,d", SHAPES)
def test_posterior_shapes_f64(ctx, n, q, d):
    """One query; exact tiles; a one-row second tile on both sides; ragged tiles, q above and below
    one tile."""
    X, Y, Xq, mean_ref, Sigma_ref, _ = reference(L.GAUSS, n, q, d, 1, 0.5)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    check_posterior(M, L.GAUSS, 0.5, Xq, mean_ref, Sigma_ref, TOL[F64], f"n={n} q={q}")
    M.close()


@pytest.mark.parametrize("name", TREES)
def test_posterior_trees(ctx, name):
    ks = L.GRAD_TREES[name]
    X, Y, Xq, mean_ref, Sigma_ref, _ = reference(ks, 777, 300, 5, 1, 0.7)
    M = model(ctx, ks, X, Y, 0.7)
    check_posterior(M, ks, 0.7, Xq, mean_ref, Sigma_ref, TOL[F64], name)
    M.close()


def test_posterior_three_label_columns(ctx):
    X, Y, Xq, mean_ref, Sigma_ref, _ = reference(L.GAUSS, 300, 70, 3, 3, 0.5)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    mean, cov = check_posterior(M, L.GAUSS, 0.5, Xq, mean_ref, Sigma_ref, TOL[F64], "m=3")
    assert mean.shape == (70, 3)
    M1 = model(ctx, L.GAUSS, X, Y[:, :1], 0.5)
    assert np.array_equal(M1.posterior(Xq)[1], cov)  # (one covariance for every label column)
    M1.close()
    M.close()


# ---- the factor, through the draws of z = I ------------------------------------------------
def check_factor(M, Xq, Sigma_ref, tol):
    """D[i, p] = Lq[p, i]: zero left of the diagonal exactly, and D^T D = Sigma + j I."""
    q = Xq.shape[0]
    mean = M.predict(Xq)
    out, j = M.sample(Xq, n=q, z=np.eye(q, dtype=M.dtype))
    assert out.shape == (q, q, 1) and out.dtype == M.dtype
    D = out[:, :, 0].astype(np.float64) - mean.T.astype(np.float64)
    assert np.all(np.tril(D, -1) == 0)
    err = float(np.max(np.abs(D.T @ D - (Sigma_ref + j * np.eye(q)))) / np.max(np.abs(Sigma_ref)))
    print(f"factor q={q} {M.dtype}: jitter {j:.3e}, reconstruction {err:.2e}")
    assert err <= tol
    return j


@pytest.mark.parametrize("n,q,d", SHAPES)
def test_factor_f64(ctx, n, q, d):
    X, Y, Xq, _, Sigma_ref, maxdiag = reference(L.GAUSS, n, q, d, 1, 0.5)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    j = check_factor(M, Xq, Sigma_ref, TOL[F64])
    j0 = q * 2.0 ** -52 * maxdiag
    assert abs(j - j0) <= TOL[F64] * j0  # (no escalation: numpy factors Sigma + j0 I here to 1e-15)
    M.close()


# ---- seeded draws -------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2])
def test_seeded_draws(ctx, m):
    """noise=True, jitter=0: cond(Sigma + s^2 I) <= (|K| + s^2) / s^2, so the draws follow the
    restatement's at the project's tolerance."""
    n, q, d, sigma = 129, 129, 3, 0.5
    X, Y, Xq, mean_ref, Sigma_ref, _ = reference(L.GAUSS, n, q, d, m, sigma)
    M = model(ctx, L.GAUSS, X, Y, sigma)
    got, j = M.sample(Xq, n=5, seed=7, noise=True, jitter=0)
    ref = S.sample(mean_ref, Sigma_ref + sigma ** 2 * np.eye(q), 0.0, S.normals(7, 5 * m * q).reshape(5, m, q))
    print(f"seeded draws m={m}: {relerr(got, ref):.2e}")
    assert j == 0.0 and got.shape == (5, q, m)
    assert relerr(got, ref) <= TOL[F64]
    two, _ = M.sample(Xq, n=2, seed=7, noise=True, jitter=0)
    assert np.array_equal(two, got[:2])  # (draw i does not depend on n)
    again, _ = M.sample(Xq, n=5, seed=7, noise=True, jitter=0)
    assert np.array_equal(again, got)
    other, _ = M.sample(Xq, n=5, seed=8, noise=True, jitter=0)
    assert not np.array_equal(other, got)
    # (the generator's stream in the caller's hands gives the same draws)
    mine, _ = M.sample(Xq, n=5, noise=True, jitter=0, z=ctx.normals(7, 5 * m * q).reshape(5, m, q))
    assert np.array_equal(mine, got)
    M.close()


# ---- fp32 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gauss", "c3"])
def test_f32(ctx, name):
    """(600, 200), d = 4: a float32 numpy restatement itself sits at 1.7e-5 (gauss) and 4.3e-6 (c3)
    of the float64 one.  float32 Sigma of the Gaussian tree has an eigenvalue of -4.9e-6, below the
    automatic jitter 4.0e-5: escalation is allowed, not expected."""
    ks = L.GRAD_TREES[name]
    X, Y, Xq, mean_ref, Sigma_ref, _ = reference(ks, 600, 200, 4, 1, 0.7)
    M = model(ctx, ks, X, Y, 0.7, np.float32)
    Xq32 = Xq.astype(np.float32)
    mean, cov = M.posterior(Xq32)
    print(f"f32 {name}: cov {relerr(cov, Sigma_ref):.2e}")
    assert mean.dtype == np.float32 and cov.dtype == np.float32
    assert relerr(cov, Sigma_ref) <= TOL[F32] and np.array_equal(cov, cov.T)
    assert np.array_equal(mean, M.predict(Xq32))
    check_factor(M, Xq32, Sigma_ref, TOL[F32])
    out, _ = M.sample(Xq32, n=3, seed=1)
    assert out.dtype == np.float32 and out.shape == (3, 200, 1) and np.all(np.isfinite(out))
    M.close()


# ---- state and lifecycle ------------------------------------------------------------------
def test_the_model_is_read_not_changed(ctx):
    X, Y, Xq, *_ = reference(L.C3, 300, 70, 3, 1, 0.5)
    M = model(ctx, L.C3, X, Y, 0.5)
    before = [M.alpha(), M.predict(Xq), M.posterior_cov(Xq, Xq)]
    M.posterior(Xq)
    M.sample(Xq, n=4, seed=3)
    M.sample(Xq, n=2, seed=3, noise=True)
    after = [M.alpha(), M.predict(Xq), M.posterior_cov(Xq, Xq)]
    for k, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(a, b), k
    M.close()


def test_after_append_and_remove(ctx):
    """The factor append and remove keep current serves the calls as it stands."""
    n, d = 300, 3
    X, Y = make_data(n, d, 1)
    Xq = make_queries(70, d)
    M = model(ctx, L.GAUSS, X[:n - 3], Y[:n - 3], 0.5)
    assert M.append(X[n - 3:], Y[n - 3:]).appended == 3
    fresh = model(ctx, L.GAUSS, X, Y, 0.5)
    for a, b in zip(M.posterior(Xq), fresh.posterior(Xq)):
        assert relerr(a, b) <= TOL[F64]
    fresh.close()
    assert M.remove(0, 2).appended == -2
    fresh = model(ctx, L.GAUSS, X[2:], Y[2:], 0.5)
    for a, b in zip(M.posterior(Xq), fresh.posterior(Xq)):
        assert relerr(a, b) <= TOL[F64]
    mean_ref, Sigma_ref = S.posterior(L.GAUSS, X[2:], Y[2:], Xq, 0.5)
    assert relerr(M.posterior(Xq)[1], Sigma_ref) <= TOL[F64]
    fresh.close()
    M.close()


class HostGauss:
    """The Gaussian tree with no device form (tests/test_gpu_hostk.py)."""

    def __call__(self, A, B):
        r2 = np.sum((A[:, None, :] - B[None, :, :]) ** 2, axis=-1)
        return 1.3 ** 2 * np.exp(-0.5 * r2 / 0.7 ** 2)


def refused(M, Xq):
    import gpr_amd
    for call in (lambda: M.posterior(Xq), lambda: M.sample(Xq, n=2)):
        with pytest.raises(gpr_amd.GprxError) as e:
            call()
        assert e.value.status == 9  # STATE


def test_refused_states(ctx):
    import gpr_amd
    from gpr_amd import gprx
    X, Y = make_data(200, 3, 1)
    Xq = make_queries(10, 3)
    U = model(ctx, L.GAUSS, X, Y, 0.5, fit=False)  # unfitted
    refused(U, Xq)
    U.close()
    M = model(ctx, L.GAUSS, X, Y, 0.5, flags=gprx.FIT_FORCE_LU)  # an LU factor
    alpha = M.alpha()
    refused(M, Xq)
    assert np.array_equal(M.alpha(), alpha)
    M.close()
    Sp = model(ctx, L.GAUSS, X, Y, 0.5, fit=False)  # a sparse-covariance model
    Sp.set_sparse_cov(0.01 * np.eye(200) + 1e-4 * np.ones((200, 200)))
    refused(Sp, Xq)
    Sp.close()
    H = model(ctx, HostGauss(), X, Y, 0.5)  # a caller-evaluated kernel
    refused(H, Xq)
    H.close()
    vctx = gpr_amd.Context(0, virtual=2)  # a sharded context (no distributed kernel runs: not even fitted)
    try:
        V = model(vctx, L.GAUSS, X, Y, 0.5, fit=False)
        refused(V, Xq)
        V.close()
    finally:
        vctx.close()


def test_not_spd_leaves_the_model_usable(ctx):
    """Every query twice, no noise, no jitter: the joint covariance is singular."""
    import gpr_amd
    X, Y, Xq, mean_ref, Sigma_ref, _ = reference(L.GAUSS, 300, 70, 3, 1, 0.5)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    before = M.predict(Xq)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.sample(np.concatenate([Xq, Xq]), n=2, jitter=0, noise=False)
    assert e.value.status == 2  # NOT_SPD
    assert np.array_equal(M.predict(Xq), before)
    assert relerr(M.posterior(Xq)[1], Sigma_ref) <= TOL[F64]
    out, j = M.sample(np.concatenate([Xq, Xq]), n=2, seed=5)  # (the automatic jitter serves the same request)
    assert j > 0 and np.all(np.isfinite(out))
    M.close()


def test_empty_requests(ctx):
    X, Y, Xq, *_ = reference(L.GAUSS, 300, 70, 3, 3, 0.5)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    mean, cov = M.posterior(np.empty((0, 3)))
    assert mean.shape == (0, 3) and cov.shape == (0, 0)
    out, j = M.sample(np.empty((0, 3)), n=4)
    assert out.shape == (4, 0, 3)
    out, j = M.sample(Xq, n=0)
    assert out.shape == (0, 70, 3)
    M.close()
