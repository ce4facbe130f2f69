"""gprx_model_remove (Model.remove): samples taken out of a fitted model by updating its Cholesky
factor with Givens rotations (k_remove.hip), against the numpy restatement of the sweep
(tests/remove_ref.py) and the CPU oracle's fit of the reduced data.  Tolerances are the fit's own
(tests/helpers.TOL, tests/test_gpu_append.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import remove_ref as R
from tests.helpers import make_data, make_queries, relerr, TOL
from tests.test_gpu_parity import KERNELS

pytestmark = pytest.mark.gpu

SIGMA = 0.5
INDEF = "RationalQuadraticKernel(1.2,2,-1,)"  # tests/test_gpu_append.py: K + sigma^2 I indefinite
SHAPES = [
    (300, 0, 1, 3, 2),
    (300, 44, 17, 3, 2),    # two passes: 16 + 1 vectors
    (257, 0, 1, 3, 1),      # np shrinks 384 -> 256
    (300, 283, 17, 3, 1),   # removes the tail: no rotation
    (640, 130, 5, 2, 3),
    (420, 100, 128, 3, 1),  # eight passes
    (200, 0, 100, 2, 1),    # one block left
    (1100, 0, 1, 2, 17),    # nine chained blocks
]
_refs = {}


def keep_rows(n, first, count):
    return np.r_[0:first, first + count:n]


def oracle_reduced(ks, n, first, count, d, m, sigma=SIGMA):
    """(X, Y, keep, alpha, C, log det) of the oracle on make_data(n, d, m) without rows
    [first, first + count), computed once."""
    key = (ks, n, first, count, d, m, sigma)
    if key not in _refs:
        X, Y = make_data(n, d, m)
        keep = keep_rows(n, first, count)
        a, C = O.fit(ks, X[keep], Y[keep], sigma)
        ld = np.linalg.slogdet(O.kernel_matrix(ks, X[keep]) + sigma * sigma * np.eye(len(keep)))[1]
        for v in (X, Y, a, C):
            v.setflags(write=False)
        _refs[key] = (X, Y, keep, a, C, ld)
    return _refs[key]


def fitted(ctx, ks, X, Y, dtype=np.float64, sigma=SIGMA, flags=0):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X.astype(dtype), Y.astype(dtype))
    M.set_kernel(ks)
    M.set_noise(sigma)
    return M, M.fit(flags)


# ---- the kernel alone (gprx_dev_factor_update) against the restatement in the same dtype ----
_hook = {}


def hook_problem(n, r, lead, dtype):
    """(L, X, target, restatement's backward error) for a random SPD factor and update."""
    key = (n, r, lead, np.dtype(dtype))
    if key not in _hook:
        rng = np.random.default_rng(1000 * n + 10 * r + lead)
        B = rng.standard_normal((n, n)) / np.sqrt(n)
        L = np.linalg.cholesky(B @ B.T + 0.5 * np.eye(n)).astype(dtype)
        X = rng.standard_normal((n, r)).astype(dtype)
        if lead:
            X[:n // 3 + 5] = 0  # leading zero rows, ending inside a block
        Ld, Xd = L.astype(np.float64), X.astype(np.float64)
        target = Ld @ Ld.T + Xd @ Xd.T
        e_ref = R.backward_error(R.update_factor(L, X), target)
        _hook[key] = (L, X, target, e_ref)
    return _hook[key]


def test_hook_width_is_the_restatement_s(ctx):
    assert ctx.factor_update_width() == R.WIDTH


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("r", [1, 5, R.WIDTH, R.WIDTH + 1])
@pytest.mark.parametrize("n", [128, 384, 1152])
def test_factor_update_kernel(ctx, n, r, lead, dtype):
    L, X, target, e_ref = hook_problem(n, r, lead, dtype)
    Lnew, Linv = ctx.factor_update(L, X)
    assert Lnew.dtype == dtype and not np.triu(Lnew, 1).any()
    err = R.backward_error(Lnew, target)
    print(f"factor_update n={n} r={r} lead={lead} {np.dtype(dtype).name}: kernel {err:.3e}, restatement {e_ref:.3e}")
    assert np.all(np.isfinite(Lnew)) and err <= 100 * e_ref
    # Linv: the inverse of every diagonal block, at tests/test_gpu_diag.py's tolerance scaled to the dtype
    u = np.finfo(dtype).eps / np.finfo(np.float64).eps
    for b in range(n // R.DB):
        sb = slice(b * R.DB, (b + 1) * R.DB)
        D, Li = Lnew[sb, sb].astype(np.float64), Linv[sb].astype(np.float64)
        cond = np.linalg.cond(D @ D.T)
        assert not np.triu(Li, 1).any()
        assert np.abs(Li @ D - np.eye(R.DB)).max() < u * (1e-15 * np.sqrt(cond) * 50 + 1e-12)


# ---- the model: parity with the oracle's fit of the reduced data ----
@pytest.mark.parametrize("ks", [KERNELS[0], KERNELS[4], KERNELS[6], KERNELS[2]])
@pytest.mark.parametrize("n,first,count,d,m", SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_remove_parity(ctx, dtype, n, first, count, d, m, ks):
    X, Y, keep, a_ref, _, ld_ref = oracle_reduced(ks, n, first, count, d, m)
    tol = TOL[np.dtype(dtype)]
    M, _ = fitted(ctx, ks, X, Y, dtype)
    info = M.remove(first, count)
    assert info.appended == -count and info.method == 0
    assert M.n == n - count and M.alpha().shape == (n - count, m)
    assert relerr(M.alpha(), a_ref) <= tol
    Xq = make_queries(64, d)
    assert relerr(M.predict(Xq.astype(dtype)), O.predict(ks, X[keep], a_ref, Xq)) <= tol
    assert abs(info.logdet - ld_ref) <= (1e-8 if dtype == np.float64 else 1e-3) * max(1, abs(info.logdet))
    M.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sliding_window(ctx, dtype):
    """Fit 250, then 20 x (append 1, remove the oldest)."""
    ks, d, m = KERNELS[4], 3, 2
    X, Y = make_data(270, d, m)
    M, _ = fitted(ctx, ks, X[:250], Y[:250], dtype)
    for i in range(250, 270):
        assert M.append(X[i:i + 1].astype(dtype), Y[i:i + 1].astype(dtype)).appended == 1
        assert M.remove(0, 1).appended == -1
        assert M.n == 250
    a_ref, _ = O.fit(ks, X[20:], Y[20:], SIGMA)
    assert relerr(M.alpha(), a_ref) <= TOL[np.dtype(dtype)]
    M.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_repeated_removes_cross_a_block_boundary(ctx, dtype):
    ks, d, m = KERNELS[4], 3, 2
    X, Y = make_data(260, d, m)
    M, _ = fitted(ctx, ks, X, Y, dtype)
    for i in range(10):
        assert M.remove(0, 1).appended == -1
        assert M.alpha().shape[0] == 259 - i
    a_ref, _ = O.fit(ks, X[10:], Y[10:], SIGMA)
    assert relerr(M.alpha(), a_ref) <= TOL[np.dtype(dtype)]
    M.close()


@pytest.mark.parametrize("ks", [KERNELS[0], KERNELS[4]])
def test_posterior_after_remove(ctx, ks):
    """The new Linv and the dropped inverse: tests/test_gpu_append.py::test_posterior_after_append's
    checks and tolerances."""
    n, first, count, d, sigma = 320, 60, 20, 3, 0.3
    X, Y, keep, _, C_ref, _ = oracle_reduced(ks, n, first, count, d, 1, sigma)
    M, _ = fitted(ctx, ks, X, Y, sigma=sigma)
    assert M.remove(first, count).appended == -count
    Xa = make_queries(40, d)
    for Xb in (Xa, Xa[::-1].copy()):
        c = M.posterior_cov(Xa, Xb)
        c_ref = O.posterior_cov(ks, X[keep], C_ref, Xa, Xb)
        kab = np.array([O.kernel_eval(ks, a, b, with_grad=False) for a, b in zip(Xa, Xb)])
        assert np.max(np.abs(c - c_ref)) <= 1e-6 * max(1.0, np.max(np.abs(kab)))
    assert relerr(M.core_matrix(), C_ref) <= 1e-6
    M.close()


@pytest.mark.parametrize("ks", [KERNELS[0], KERNELS[4]])
def test_lml_after_remove(ctx, ks):
    n, first, count, d, sigma = 180, 25, 30, 2, 0.4
    X, Y = make_data(n, d)
    keep = keep_rows(n, first, count)
    M, _ = fitted(ctx, ks, X, Y, sigma=sigma)
    M.lml(grad=True)  # (a want_inv fit first: its inverse rows are dropped by the remove)
    assert M.remove(first, count).appended == -count
    v, g, logdet = M.lml(grad=True)
    vr, gr, _, ldr = O.lml(ks, X[keep], Y[keep], sigma)
    assert abs(v - vr) <= 1e-6 * max(1.0, abs(vr))
    assert abs(logdet - ldr) <= 1e-8 * max(1.0, abs(ldr))
    assert relerr(g, gr) <= 1e-6
    M.close()


# ---- refusals and fallbacks ----
def test_refusals_leave_the_model_bit_identical(ctx):
    import gpr_amd
    ks, n, d, m = KERNELS[0], 200, 3, 1
    X, Y = make_data(n, d, m)
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X, Y)
    M.set_kernel(ks)
    M.set_noise(SIGMA)
    with pytest.raises(gpr_amd.GprxError) as e:  # before any fit
        M.remove(0, 1)
    assert e.value.status == 9 and M.n == n
    M.fit()
    Xq = make_queries(64, d)
    a0, p0 = M.alpha(), M.predict(Xq)
    for first, count in [(-1, 1), (0, 0), (0, -3), (n, 1), (n - 1, 2), (0, n)]:
        with pytest.raises(gpr_amd.GprxError) as e:
            M.remove(first, count)
        assert e.value.status == 4, (first, count)  # DIM
        assert M.n == n and np.array_equal(M.alpha(), a0) and np.array_equal(M.predict(Xq), p0)
    M.set_kernel(lambda A, B: O.cross_matrix(ks, A, B))  # a caller-evaluated kernel (set_kernel_matrix)
    M.fit()
    a1, p1 = M.alpha(), M.predict(Xq)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.remove(0, 1)
    assert e.value.status == 9
    assert M.n == n and np.array_equal(M.alpha(), a1) and np.array_equal(M.predict(Xq), p1)
    M.close()


def test_refused_on_a_sharded_context():
    """No distributed kernel runs: the model is not even fitted."""
    import gpr_amd
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        X, Y = make_data(200, 3, 1)
        M = gpr_amd.Model(vctx, np.float64)
        M.set_data(X, Y)
        M.set_kernel(KERNELS[0])
        M.set_noise(SIGMA)
        with pytest.raises(gpr_amd.GprxError) as e:
            M.remove(0, 1)
        assert e.value.status == 9 and "sharded" in str(e.value)
        assert M.n == 200
        M.close()
    finally:
        vctx.close()


def test_remove_from_an_lu_model_refits(ctx):
    """tests/test_gpu_append.py's indefinite RQ tree: the fit falls back to the LU, so the remove
    reduces the data and refits in full."""
    n, first, count, d, sigma = 260, 30, 4, 3, 0.3
    X, Y = make_data(n, d, 1)
    keep = keep_rows(n, first, count)
    Kr = O.kernel_matrix(INDEF, X[keep]) + sigma * sigma * np.eye(len(keep))
    assert np.linalg.eigvalsh(Kr)[0] < 0
    M, info = fitted(ctx, INDEF, X, Y, sigma=sigma)
    assert info.method == 1
    info = M.remove(first, count)
    assert info.appended == 0 and info.method == 1 and M.n == n - count
    a_ref = np.linalg.solve(Kr, Y[keep])
    assert relerr(M.alpha(), a_ref) <= 1e-6
    M.close()


def test_count_above_the_cutover_refits(ctx):
    from gpr_amd import gprx
    ks, d, m = KERNELS[0], 2, 1
    count = gprx.REMOVE_CUTOVER + 1
    n = count + 150
    X, Y, keep, a_ref, _, _ = oracle_reduced(ks, n, 20, count, d, m)
    M, _ = fitted(ctx, ks, X, Y)
    info = M.remove(20, count)
    assert info.appended == 0 and info.method == 0 and M.n == n - count
    assert relerr(M.alpha(), a_ref) <= TOL[np.dtype(np.float64)]
    M.close()


# ---- reuse ----
_POISON_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpr_amd
from tests import remove_ref as R
ctx = gpr_amd.Context(0)
np.savez(sys.argv[2], **R.reuse_observations(lambda dtype: gpr_amd.Model(ctx, dtype), True))
ctx.close()
"""

# (the scenario takes well under a second in this process; the child also starts Python, loads the
# code objects and plans its tile schedules: tests/test_gpu_lifecycle.py's limit)
POISON_CHILD_TIMEOUT_S = 120


def test_reused_model_equals_a_fresh_twin_also_with_poisoned_buffers(ctx, tmp_path):
    """A model driven through other shapes first (fit at 640 / m = 3, refit at 300, append) and then
    reduced equals, bit for bit, a fresh twin given only the last fit, the append and the remove;
    and the same run in a child process with GPRX_POISON=1 (fresh device buffers hold finite
    garbage) gives the same bits: the chain order is fixed and nothing unwritten is read."""
    import gpr_amd
    make = lambda dtype: gpr_amd.Model(ctx, dtype)  # noqa: E731
    mine = R.reuse_observations(make, True)
    twin = R.reuse_observations(make, False)
    bad = [k for k in sorted(mine) if not np.array_equal(mine[k], twin[k])]
    assert not bad, [(k, relerr(mine[k], twin[k])) for k in bad]
    assert mine["float64.info"][-1] == -3 and mine["float32.info"][-1] == -3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = tmp_path / "poisoned.npz"
    r = subprocess.run([sys.executable, "-c", _POISON_CHILD, root, str(f)], env=dict(os.environ, GPRX_POISON="1"),
                       capture_output=True, text=True, timeout=POISON_CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(f) as theirs:
        assert sorted(theirs.files) == sorted(mine)
        bad = [(k, relerr(mine[k], theirs[k])) for k in sorted(mine) if not np.array_equal(mine[k], theirs[k])]
    assert not bad, f"{len(bad)} of {len(mine)} observations differ under GPRX_POISON: {bad}"
