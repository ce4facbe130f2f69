"""Per-dimension length scales on the device (gprx_model_set_length_scales, gprx_model_lml_scale_grad;
k_ard.hip) against tests/ard_ref.py.

Equivalence: a model with scales ell on X is, bit for bit, a model without scales on X / ell formed in
numpy in the model's dtype (ell narrowed first, one division) -- in every read, after append and
remove, and on a two-virtual-rank context; the same under GPRX_POISON=1.
Gradient: d LML / d ell against the reference's direct differences, normwise relative error within
tests.helpers.TOL (1e-6 in f64, 1e-3 in f32); sigma = 0.5 and ell log-uniform in [0.5, 3] sqrt(d / 3)
keep cond(K + sigma^2 I) <= 2e3 (tests/test_ard_cpu.py), so cond * eps stays far inside both."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ard_ref as A
from tests.helpers import make_data, make_queries, relerr, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
# The child starts Python, loads the code objects and runs all 24 equivalence cases, the sharded
# covariance included: 2.62 s unpoisoned, measured on an MI355X with the library of the commit before
# the sharded covariance joined the poisoned run; times four for a shared machine (10.5 s), rounded
# up to half a minute (the start of a process on a busy machine varies by seconds).
CHILD_TIMEOUT_S = 30
ERR_DIM, ERR_ARG, ERR_STATE = 4, 8, 9
GRAD_SHAPES = [(1, 1), (129, 33), (260, 5), (128, 16), (300, 70)]


@pytest.fixture(scope="module")
def vctx():
    import gpr_amd
    c = gpr_amd.Context(0, virtual=2)
    yield c
    c.close()


def model(ctx, name, X, Y, ell, dtype=np.float64, fit=True, nodes=A.NODES):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(np.asarray(X, dtype), np.asarray(Y, dtype))
    M.set_kernel(nodes[name].to_string())
    M.set_noise(A.SIGMA)
    if ell is not None:
        M.set_length_scales(ell)
    if fit:
        M.fit()
    return M


def _unequal(out):
    reads = sorted(k[2:] for k in out if k.startswith("s."))
    assert reads and sorted(k[2:] for k in out if k.startswith("p.")) == reads
    return [(r, f"{relerr(out['s.' + r], out['p.' + r]):.2e}") for r in reads
            if not np.array_equal(out["s." + r], out["p." + r])]


@pytest.mark.parametrize("n,d", A.EQ_SHAPES)
@pytest.mark.parametrize("name", list(A.EQ_NODES))
def test_scaled_model_equals_prescaled_model_bit_for_bit(ctx, vctx, name, n, d):
    for dt in (F64, F32):
        bad = _unequal(A.gpu_equivalence(ctx, vctx, name, n, d, dt))
        assert not bad, f"{name} ({n}, {d}) {dt.name}: reads that differ (read, relerr): {bad}"


_POISON_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpr_amd
from tests import ard_ref as A
ctx, vctx = gpr_amd.Context(0), gpr_amd.Context(0, virtual=2)
np.savez(sys.argv[2], **A.gpu_equivalence_all(ctx, vctx, sharded_cov=True))
vctx.close()
ctx.close()
"""


def test_equivalence_with_poisoned_buffers(tmp_path):
    """All 24 cases in one child process with GPRX_POISON=1 (fresh device buffers hold finite
    garbage): the scaled copy, the second buffers of append and remove and the staged queries must
    not depend on what a new allocation holds.  The sharded fit contributes its alpha, its predict
    and its posterior_cov (the distributed solve of the queries)."""
    f = tmp_path / "poisoned.npz"
    r = subprocess.run([sys.executable, "-c", _POISON_CHILD, ROOT, str(f)], env=dict(os.environ, GPRX_POISON="1"),
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(f) as o:
        cases = sorted({k.rsplit(".s.", 1)[0] for k in o.files if ".s." in k})
        assert len(cases) == len(A.EQ_NODES) * len(A.EQ_SHAPES) * 2
        for c in cases:
            bad = _unequal({k[len(c) + 1:]: o[k] for k in o.files if k.startswith(c + ".")})
            assert not bad, f"{c} under GPRX_POISON: reads that differ (read, relerr): {bad}"


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("name", ["gauss", "gauss_per"])
def test_predict_derivative_is_in_x(ctx, name, dtype):
    """predict(deriv=True) returns d/dx: the pre-scaled model's derivative (in z = x / ell) / ell."""
    n, d = 260, 5
    X, Y = make_data(n, d, dtype=dtype)
    Xq = make_queries(A.Q, d, dtype=dtype)
    ell = A.length_scales(d)
    Ms = model(ctx, name, X, Y, ell, dtype, nodes=A.EQ_NODES)
    Mp = model(ctx, name, A.scaled(X, ell, dtype), Y, None, dtype, nodes=A.EQ_NODES)
    ms, Ds = Ms.predict(Xq, deriv=True)
    mp, Dp = Mp.predict(A.scaled(Xq, ell, dtype), deriv=True)
    err = relerr(Ds, Dp.astype(np.float64) / ell[None, :, None])
    print(f"ard deriv {name} {dtype.name}: {err:.2e}")
    assert Ds.shape == (A.Q, d, 1) and err <= TOL[dtype]
    assert relerr(ms, mp) <= TOL[dtype]
    Ms.close()
    Mp.close()


@pytest.mark.parametrize("dtype", [F64, F32])
def test_cleared_scales_give_the_unscaled_model(ctx, dtype):
    n, d = 129, 33
    X, Y = make_data(n, d, dtype=dtype)
    Xq = make_queries(A.Q, d, dtype=dtype)
    M = model(ctx, "gauss", X, Y, A.length_scales(d), dtype)
    scaled_alpha = M.alpha()
    M.set_length_scales(None)
    assert M.length_scales is None
    with pytest.raises(Exception):  # (the scaled fit is gone with the metric)
        M.predict(Xq)
    M.fit()
    F = model(ctx, "gauss", X, Y, None, dtype)
    assert not np.array_equal(scaled_alpha, F.alpha())
    assert np.array_equal(M.alpha(), F.alpha())
    assert np.array_equal(M.predict(Xq), F.predict(Xq))
    assert np.array_equal(M.lml(grad=True)[1], F.lml(grad=True)[1])
    M.close()
    F.close()


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("n,d", GRAD_SHAPES)
@pytest.mark.parametrize("name", A.NAMES)
def test_scale_gradient_against_the_reference(ctx, name, n, d, dtype):
    X, Y, ell, Z, ref = A.fixture(name, n, d, dtype)
    M = model(ctx, name, X, Y, ell, dtype)
    assert np.array_equal(M.length_scales, ell)
    g = M.lml_scale_grad()
    err = relerr(g, ref)
    print(f"ard grad {name} ({n}, {d}) {dtype.name}: relerr {err:.2e}, |grad| {np.max(np.abs(ref)):.3g}")
    assert g.shape == (d,) and g.dtype == np.float64
    assert err <= TOL[dtype]
    assert np.array_equal(M.lml_scale_grad(), g)  # deterministic: the same bits again
    if (n, d) == (260, 5):
        v3 = M.lml(grad=True)
        v4 = M.lml(grad=True, scales=True)
        assert len(v3) == 3 and len(v4) == 4
        assert v4[0] == v3[0] and np.array_equal(v4[1], v3[1]) and v4[2] == v3[2]
        assert np.array_equal(v4[3], M.lml_scale_grad())
        assert relerr(v4[3], ref) <= TOL[dtype]
    M.close()


def test_unfitted_model_is_fitted_by_the_call(ctx):
    X, Y, ell, Z, ref = A.fixture("rq_m32", 260, 5)
    M = model(ctx, "rq_m32", X, Y, ell, fit=False)
    assert relerr(M.lml_scale_grad(), ref) <= TOL[F64]
    assert M.alpha().shape == (260, 1)
    M.close()


@pytest.mark.parametrize("dtype", [F64, F32])
def test_gradient_after_append_and_remove(ctx, dtype):
    """The appended / reduced model as it stands (no refit) against the reference on the changed data."""
    n, d, k = 129, 33, 5
    name = "m32_x_gauss"
    X, Y = make_data(n + k, d, dtype=dtype)
    ell = A.length_scales(d)
    ell_t = ell.astype(dtype).astype(np.float64)
    M = model(ctx, name, X[:n], Y[:n], ell, dtype)
    assert M.append(X[n:], Y[n:]).appended == k
    e1 = relerr(M.lml_scale_grad(), A.grad_ell(A.NODES[name], A.scaled(X, ell, dtype), Y, ell_t))
    assert M.remove(3, 2).appended == -2
    keep = np.r_[0:3, 5:n + k]
    e2 = relerr(M.lml_scale_grad(), A.grad_ell(A.NODES[name], A.scaled(X[keep], ell, dtype), Y[keep], ell_t))
    print(f"ard grad {dtype.name} after append {e1:.2e}, after remove {e2:.2e}")
    assert e1 <= TOL[dtype] and e2 <= TOL[dtype]
    M.close()


def test_gradient_is_the_central_difference_of_the_device_value(ctx):
    """lml(grad=False) at ell_j (1 +- 1e-5) on the device, j = 0 and d - 1, (260, 5), f64: agreement
    within 1e-5 of the gradient's largest component."""
    name, n, d, h = "rq_m32", 260, 5, 1e-5
    X, Y, ell, Z, ref = A.fixture(name, n, d)
    M = model(ctx, name, X, Y, ell)
    g = M.lml_scale_grad()
    for j in (0, d - 1):
        v = []
        for s in (1 + h, 1 - h):
            e = ell.copy()
            e[j] *= s
            M.set_length_scales(e)
            v.append(M.lml(grad=False)[0])
        fd = (v[0] - v[1]) / (2 * h * ell[j])
        print(f"ard fd on the device: j = {j}, grad {g[j]:.9g}, central difference {fd:.9g}")
        assert abs(fd - g[j]) <= 1e-5 * np.max(np.abs(g))
    M.close()


def _refused(status, call):
    from gpr_amd.gprx import GprxError
    with pytest.raises(GprxError) as e:
        call()
    assert e.value.status == status, str(e.value)


def test_refusals_leave_the_model_untouched(ctx, vctx):
    import gpr_amd
    from gpr_amd.gprx import FIT_FORCE_LU
    n, d = 130, 4
    X, Y = make_data(n, d)
    Xq = make_queries(A.Q, d)
    ell = A.length_scales(d)

    def untouched(M, status, call):
        before = M.predict(Xq)
        _refused(status, call)
        assert np.array_equal(M.predict(Xq), before)

    # a Periodic tree: its fit and predict work with scales, the gradient is refused
    M = model(ctx, "gauss_per", X, Y, ell, nodes=A.EQ_NODES)
    untouched(M, ERR_STATE, M.lml_scale_grad)
    M.close()
    # no scales set
    M = model(ctx, "gauss", X, Y, None)
    untouched(M, ERR_STATE, M.lml_scale_grad)
    # bad values and a wrong count: refused before anything is dropped
    for bad in (0.0, -1.0, np.nan, np.inf):
        e = ell.copy()
        e[1] = bad
        untouched(M, ERR_ARG, lambda: M.set_length_scales(e))
    untouched(M, ERR_DIM, lambda: M.set_length_scales(np.ones(d + 1)))
    assert M.length_scales is None
    M.close()
    # ... and from set_data when the scales came first
    M = gpr_amd.Model(ctx, np.float64)
    M.set_length_scales(np.ones(d + 1))
    _refused(ERR_DIM, lambda: M.set_data(X, Y))
    M.close()
    # two label columns
    X2, Y2 = make_data(n, d, 2)
    M = model(ctx, "gauss", X2, Y2, ell)
    untouched(M, ERR_DIM, M.lml_scale_grad)
    M.close()
    # a caller-evaluated kernel owns its metric, whichever comes second
    host_kernel = lambda a, b: np.exp(-0.5 * np.sum((a[:, None, :] - b[None, :, :]) ** 2, axis=-1))  # noqa: E731
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X, Y)
    M.set_kernel(host_kernel)
    M.set_noise(A.SIGMA)
    M.fit()
    untouched(M, ERR_STATE, lambda: M.set_length_scales(ell))
    M.close()
    M = gpr_amd.Model(ctx, np.float64)
    M.set_length_scales(ell)
    M.set_data(X, Y)
    _refused(ERR_STATE, lambda: M.set_kernel(host_kernel))
    M.close()
    # an LU factor
    M = model(ctx, "gauss", X, Y, ell, fit=False)
    M.fit(FIT_FORCE_LU)
    untouched(M, ERR_STATE, M.lml_scale_grad)
    M.close()
    # a virtual-rank context
    M = model(vctx, "gauss", X, Y, ell)
    untouched(M, ERR_STATE, M.lml_scale_grad)
    M.close()
