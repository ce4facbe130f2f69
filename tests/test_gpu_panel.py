"""The chained thin-panel forward substitution (k_append.hip) alone, through
gprx_dev_forward_panel: V L^T = R for a panel of 1..128 rows against a factor of 1..10
128-column blocks (no hand-off, one hand-off, a ten-block ticket chain; 16-row padding).

Reference: numpy's triangular solve in float64.  The kernel must be within the project's
tolerance and within 4x the error of the GEMM path (trsm_rows, code from before this kernel) on
the same input: both do the same arithmetic in another summation order, so a larger gap is a
bug.  The hook surrounds the panel with guard rows and columns and compares them bitwise
afterwards (rows beyond `rows` and everything outside the panel must be untouched): a kernel
that writes there fails the call."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import make_data, relerr, uniform, TOL

pytestmark = pytest.mark.gpu

KS = "GaussianKernel(0.7,1.3,)"
_cache = {}


def factor(n):
    """(L, L in float64) of K(X, X) + 0.25 I, and the reference solves, computed once per n."""
    if n not in _cache:
        X, _ = make_data(n, 3)
        L = np.linalg.cholesky(O.kernel_matrix(KS, X) + 0.25 * np.eye(n))
        R = 2.0 * uniform(7, 128 * n).reshape(128, n) - 1.0
        V = np.linalg.solve(L, R.T).T  # V L^T = R
        for a in (L, R, V):
            a.setflags(write=False)
        _cache[n] = (L, R, V)
    return _cache[n]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("rows", [1, 16, 17, 128])
@pytest.mark.parametrize("n", [128, 256, 384, 1280])
def test_forward_panel(ctx, n, rows, dtype):
    L, R, V = factor(n)
    Lt, Rt = L.astype(dtype), R[:rows].astype(dtype)
    Rt0 = Rt.copy()
    Vk = ctx.forward_panel(Lt, Rt)
    Vg = ctx.forward_panel(Lt, Rt, use_gemm=True)
    assert np.array_equal(Rt, Rt0)  # (the wrapper solves a copy)
    assert Vk.shape == (rows, n) and Vk.dtype == np.dtype(dtype)
    ek, eg = relerr(Vk, V[:rows]), relerr(Vg, V[:rows])
    print(f"forward_panel n={n} rows={rows} {np.dtype(dtype).name}: chained {ek:.3e}, gemm {eg:.3e}")
    assert ek <= TOL[np.dtype(dtype)]
    assert ek <= 4 * eg
