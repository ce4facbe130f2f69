"""gprx_model_loo (Model.loo): leave-one-out means, variances, predictive log probability and its
gradient (k_loo.hip, the gradient kernels' two-vector mode) against the numpy restatement
(tests/loo_ref.py).  Tolerances are the project's (tests/helpers.TOL): 1e-6 normwise relative in
f64, 1e-3 in f32, |v - vr| <= tol max(1, |vr|) for the value.  sigma >= 0.4 keeps
cond(K + sigma^2 I) far inside 1 / tol."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import loo_ref as L
from tests.helpers import make_data, make_queries, relerr, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
CHILD_TIMEOUT_S = 120  # (the child starts Python and loads the code objects: tests/test_gpu_lifecycle.py's limit)
_refs = {}


def reference(ks, n, d, m, sigma, grad):
    """(X, Y, value, mu, s2, grad) of the restatement on make_data(n, d, m), computed once."""
    key = (ks, n, d, m, sigma, grad)
    if key not in _refs:
        X, Y = make_data(n, d, m)
        v, mu, s2, g = L.loo(ks, X, Y, sigma, grad=grad)
        for a in (X, Y, mu, s2) + ((g,) if grad else ()):
            a.setflags(write=False)
        _refs[key] = (X, Y, v, mu, s2, g)
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


def check(got, ref, tol, what, grad=True):
    v, mu, s2, g = got
    vr, mur, s2r, gr = ref
    print(f"loo {what}: value {abs(v - vr) / max(1.0, abs(vr)):.2e}, mean {relerr(mu, mur):.2e}, "
          f"var {relerr(s2, s2r):.2e}" + (f", grad {relerr(g, gr):.2e}" if grad else ""))
    assert mu.shape == mur.shape and s2.shape == s2r.shape
    assert abs(v - vr) <= tol * max(1.0, abs(vr))
    assert relerr(mu, mur) <= tol
    assert relerr(s2, s2r) <= tol
    if grad:
        assert g.shape == gr.shape and relerr(g, gr) <= tol
    else:
        assert g is None


@pytest.mark.parametrize("n,d", [(100, 3), (128, 3), (129, 3), (777, 5)])
def test_shapes_f64(ctx, n, d):
    """Inside one tile, an exact tile, a one-row second tile, seven ragged tiles: the values from a
    fitted model (diag(C) from V alone), then value + gradient (C formed, its diagonal read)."""
    X, Y, *ref = reference(L.GAUSS, n, d, 1, 0.5, True)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    check(M.loo(), ref, TOL[F64], f"n={n} values", grad=False)
    check(M.loo(grad=True), ref, TOL[F64], f"n={n} gradient")
    M.close()


@pytest.mark.parametrize("name", sorted(L.GRAD_TREES))
def test_trees_value_and_gradient(ctx, name):
    """n = 777: the C3 tree (grad_mma_kernel2 with the periodic statistic), Matern 3/2
    (grad_mma_kernel2_m), the RQ + GaussianExp sum, and a product tree, which the pair path
    refuses: the VALU kernel (lml_grad_kernel2)."""
    ks = L.GRAD_TREES[name]
    X, Y, *ref = reference(ks, 777, 5, 1, 0.7, True)
    M = model(ctx, ks, X, Y, 0.7, fit=False)  # (fitted by the call, the inverse riding along)
    check(M.loo(grad=True), ref, TOL[F64], name)
    M.close()


_DIRECT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpr_amd
from tests import loo_ref as L
ctx = gpr_amd.Context(0)
np.savez(sys.argv[2], **L.gpu_observations(ctx, ["gauss"]))
ctx.close()
"""


def test_gaussian_tree_on_the_valu_kernel(tmp_path):
    """GPRX_LML_GRAD=direct (read once per process: a child) takes the Gaussian tree off the MFMA
    pair statistics."""
    X, Y, *ref = reference(L.GAUSS, 777, 5, 1, 0.7, True)
    f = tmp_path / "direct.npz"
    r = subprocess.run([sys.executable, "-c", _DIRECT_CHILD, ROOT, str(f)], env=dict(os.environ, GPRX_LML_GRAD="direct"),
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(f) as o:
        check((float(o["gauss.value"]), o["gauss.mean"], o["gauss.var"], o["gauss.grad"]), ref, TOL[F64], "direct")


@pytest.mark.parametrize("name", ["gauss", "c3"])
def test_f32(ctx, name):
    ks = L.GRAD_TREES[name]
    X, Y, *ref = reference(ks, 600, 4, 1, 0.7, True)
    M = model(ctx, ks, X, Y, 0.7, np.float32)  # (a refined fp32 fit, used as it is)
    got = M.loo()
    assert got[1].dtype == np.float32 and got[2].dtype == np.float32
    check(got, ref, TOL[F32], f"f32 {name} values", grad=False)
    check(M.loo(grad=True), ref, TOL[F32], f"f32 {name} gradient")
    M.close()


def test_three_label_columns(ctx):
    import gpr_amd
    X, Y, *ref = reference(L.GAUSS, 300, 3, 3, 0.5, False)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    got = M.loo()
    assert got[1].shape == (300, 3) and got[2].shape == (300,)
    check(got, ref, TOL[F64], "m=3", grad=False)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.loo(grad=True)
    assert e.value.status == 4  # DIM
    check(M.loo(), ref, TOL[F64], "m=3 after the refused gradient", grad=False)
    M.close()


def _reads(M, Xq):
    mean, deriv = M.predict(Xq, deriv=True)  # the VALU predict
    return [M.alpha(), M.predict(Xq), mean, deriv, M.posterior_cov(Xq, Xq[::-1].copy()), M.core_matrix()]


def test_no_refit_and_no_trace(ctx):
    """A fitted model is read, not refitted: what the other calls return is the same bits before
    and after, and an LML afterwards equals a fresh twin's."""
    X, Y, *ref = reference(L.C3, 300, 3, 1, 0.5, True)
    Xq = make_queries(40, 3)
    M = model(ctx, L.C3, X, Y, 0.5)
    before = _reads(M, Xq)
    check(M.loo(), ref, TOL[F64], "fitted values", grad=False)
    check(M.loo(grad=True), ref, TOL[F64], "fitted gradient")
    after = _reads(M, Xq)
    for k, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(a, b), k
    twin = model(ctx, L.C3, X, Y, 0.5)
    v, g, ld = M.lml(grad=True)
    vt, gt, ldt = twin.lml(grad=True)
    assert v == vt and ld == ldt and np.array_equal(g, gt)
    M.close()
    twin.close()


def test_installed_alpha_is_used_as_it_is(ctx):
    X, Y, v, mu, s2, _ = reference(L.GAUSS, 300, 3, 1, 0.5, False)
    M = model(ctx, L.GAUSS, X, Y, 0.5)
    M.set_alpha(2 * M.alpha())
    _, mean, var, _ = M.loo()
    assert relerr(mean, Y - 2 * (Y - mu)) <= TOL[F64] and relerr(var, s2) <= TOL[F64]
    M.close()


def test_after_append_and_remove(ctx):
    """The factor append and remove keep current serves the call: no refit on a sliding window."""
    n = 300
    X, Y = make_data(n, 3, 1)
    M = model(ctx, L.GAUSS, X[:n - 5], Y[:n - 5], 0.5)
    assert M.append(X[n - 5:], Y[n - 5:]).appended == 5
    check(M.loo(), L.loo(L.GAUSS, X, Y, 0.5), TOL[F64], "after append", grad=False)
    assert M.remove(0, 1).appended == -1
    ref = L.loo(L.GAUSS, X[1:], Y[1:], 0.5, grad=True)
    check(M.loo(), ref, TOL[F64], "after remove", grad=False)
    check(M.loo(grad=True), ref, TOL[F64], "after remove, gradient")
    M.close()


def test_repeated_calls_give_the_same_bits(ctx):
    X, Y, *_ = reference(L.C3, 777, 5, 1, 0.7, True)
    M = model(ctx, L.C3, X, Y, 0.7)
    a, b = M.loo(grad=True), M.loo(grad=True)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    M.close()


def test_unfitted_model_is_fitted_by_the_call(ctx):
    X, Y, *ref = reference(L.GAUSS, 300, 3, 1, 0.5, False)
    M = model(ctx, L.GAUSS, X, Y, 0.5, fit=False)
    check(M.loo(), ref, TOL[F64], "unfitted", grad=False)
    assert M.alpha().shape == (300, 1)  # (fitted now)
    M.close()


def test_not_spd(ctx):
    """Duplicated samples and no noise: the fit inside the call takes no LU fallback."""
    import gpr_amd
    X, Y = make_data(50, 3, 1)
    M = model(ctx, L.GAUSS, np.tile(X, (4, 1)), np.tile(Y, (4, 1)), 0.0, fit=False)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.loo()
    assert e.value.status == 2  # NOT_SPD
    M.close()


def test_refused_states(ctx):
    import gpr_amd
    from gpr_amd import gprx
    X, Y = make_data(200, 3, 1)
    M = model(ctx, L.GAUSS, X, Y, 0.5, flags=gprx.FIT_FORCE_LU)
    alpha = M.alpha()
    for grad in (False, True):
        with pytest.raises(gpr_amd.GprxError) as e:
            M.loo(grad=grad)
        assert e.value.status == 9  # STATE
    assert np.array_equal(M.alpha(), alpha)
    M.close()
    S = model(ctx, L.GAUSS, X, Y, 0.5, fit=False)
    S.set_sparse_cov(0.01 * np.eye(200) + 1e-4 * np.ones((200, 200)))
    with pytest.raises(gpr_amd.GprxError) as e:
        S.loo()
    assert e.value.status == 9
    S.close()
    vctx = gpr_amd.Context(0, virtual=2)  # (no distributed kernel runs: the model is not even fitted)
    try:
        V = model(vctx, L.GAUSS, X, Y, 0.5, fit=False)
        with pytest.raises(gpr_amd.GprxError) as e:
            V.loo()
        assert e.value.status == 9
        V.close()
    finally:
        vctx.close()


class HostGauss:
    """The Gaussian tree with no device form (tests/test_gpu_hostk.py)."""

    def __call__(self, A, B):
        r2 = np.sum((A[:, None, :] - B[None, :, :]) ** 2, axis=-1)
        return 1.3 ** 2 * np.exp(-0.5 * r2 / 0.7 ** 2)


def test_caller_evaluated_kernel(ctx):
    import gpr_amd
    X, Y, *ref = reference(L.GAUSS, 300, 3, 1, 0.5, False)
    M = model(ctx, HostGauss(), X, Y, 0.5)
    check(M.loo(), ref, TOL[F64], "caller-evaluated kernel", grad=False)
    with pytest.raises(gpr_amd.GprxError) as e:
        M.loo(grad=True)
    assert e.value.status == 9
    # (the C ABI refuses it too, and leaves the model as it was)
    g = np.zeros(8)
    st = gprx_loo_status(M, g)
    assert st == 9
    check(M.loo(), ref, TOL[F64], "caller-evaluated kernel, again", grad=False)
    M.close()


def gprx_loo_status(M, g):
    import ctypes
    from gpr_amd import gprx
    v, npar = ctypes.c_double(), ctypes.c_int32()
    return gprx.lib().gprx_model_loo(M.h, gprx.LOO_GRAD, ctypes.byref(v), None, None, gprx._ptr(g), ctypes.byref(npar))


_POISON_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpr_amd
from tests import loo_ref as L
ctx = gpr_amd.Context(0)
np.savez(sys.argv[2], **L.gpu_observations(ctx, sorted(L.GRAD_TREES)))
ctx.close()
"""


def test_poisoned_buffers_give_the_same_bits(ctx, tmp_path):
    """The f64 value + gradient cases in a child process with GPRX_POISON=1 (fresh device buffers
    hold finite garbage): the same bits as here, so nothing unwritten is read."""
    mine = L.gpu_observations(ctx, sorted(L.GRAD_TREES))
    f = tmp_path / "poisoned.npz"
    r = subprocess.run([sys.executable, "-c", _POISON_CHILD, ROOT, str(f)], env=dict(os.environ, GPRX_POISON="1"),
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(f) as theirs:
        assert sorted(theirs.files) == sorted(mine)
        bad = [(k, relerr(mine[k], theirs[k])) for k in sorted(mine) if not np.array_equal(mine[k], theirs[k])]
    assert not bad, f"{len(bad)} of {len(mine)} observations differ under GPRX_POISON: {bad}"
