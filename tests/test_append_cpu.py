"""gprx_model_append without a GPU: the ABI additions, and the block-boundary algebra the device
code follows (gprx_fit.cpp model_append), restated in numpy against the oracle.

With n samples fitted, k new ones, n0 = floor(n / 128) * 128 and t = n - n0:
  * rows [0, n0) of L do not depend on later rows and are kept;
  * the panel P = L[n0.., 0..n0): its first t rows are the old partial block's, its k new rows
    are K(Xnew, X[0:n0]) L00^{-T}, solved block by block with the diagonal blocks' inverses,
    V_b = (R_b - sum_{j<b} V_j L_bj^T) Linv_b^T  (k_append.hip);
  * the trailing block S = K(act, act) + sigma^2 I - P P^T over the t + k active rows is padded
    with the identity to a multiple of 128 and factored;
  * z = L^{-1} Y for ALL rows against the whole new factor, alpha = L^{-T} z, log det = 2 sum log L_ii.
"""
import ctypes

import numpy as np
import pytest

from gpr_amd import gprx
from oracle import oracle as O
from tests.helpers import make_data, relerr

DB = 128
KERNELS = [
    "GaussianKernel(0.7,1.3,)",
    "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))",
    "SumKernel(GaussianKernel(0.8,1,),WhiteKernel(0.3,))",
    "RationalQuadraticKernel(1.1,0.6,1.5,)",
]


def test_symbols_exported():
    lib = ctypes.CDLL(gprx.LIB_PATH)
    assert hasattr(lib, "gprx_model_append") and hasattr(lib, "gprx_dev_forward_panel")
    assert "gprx_model_append" in gprx.EXPORTED
    assert gprx.APPEND_SOLVE_GEMM == 16


def test_fit_info_keeps_its_size():
    names = [f[0] for f in gprx.FitInfo._fields_]
    assert names[-1] == "appended" and "pad" not in names
    assert ctypes.sizeof(gprx.FitInfo) == 8 * 2 + 4 * 2 + 8 * 3 + 8 * 2 + 4 * 2
    assert gprx.FitInfo.appended.offset == ctypes.sizeof(gprx.FitInfo) - 4


def padded_factor(K, n):
    """The device's stored factor of an n x n matrix: identity-padded to a multiple of 128."""
    npad = -(-n // DB) * DB
    A = np.eye(npad)
    A[:n, :n] = K
    return np.linalg.cholesky(A)


def panel_solve(L, R):
    """V with V L^T = R by 128-column blocks, each with its diagonal block's inverse."""
    V = np.array(R, dtype=np.float64)
    for b in range(L.shape[0] // DB):
        sb = slice(b * DB, (b + 1) * DB)
        acc = V[:, sb].copy()
        for j in range(b):
            sj = slice(j * DB, (j + 1) * DB)
            acc -= V[:, sj] @ L[sb, sj].T
        V[:, sb] = acc @ np.linalg.inv(L[sb, sb]).T
    return V


def append_factor(ks, X, Y, sigma, n, L_old):
    """The factor of all the samples from the factor of the first n, as model_append does it."""
    n1 = X.shape[0]
    k = n1 - n
    n0 = n // DB * DB
    t = n - n0
    np1 = -(-n1 // DB) * DB
    nap = np1 - n0
    L = np.zeros((np1, np1))
    L[:n0, :n0] = L_old[:n0, :n0]
    act = slice(n0, n1)
    if n0 > 0:
        L[n0:n, :n0] = L_old[n0:n, :n0]  # the old partial block's rows of the panel
        L[n:n1, :n0] = panel_solve(L[:n0, :n0], O.cross_matrix(ks, X[n:], X[:n0]))
    S = np.eye(nap)
    S[:t + k, :t + k] = O.kernel_matrix(ks, X[act]) + sigma * sigma * np.eye(t + k)
    S -= L[n0:, :n0] @ L[n0:, :n0].T
    L[n0:, n0:] = np.linalg.cholesky(S)
    Yp = np.zeros((np1, Y.shape[1]))
    Yp[:n1] = Y
    z = panel_solve(L, Yp.T).T  # every label row, against the whole factor
    alpha = np.linalg.solve(L.T, z)[:n1]
    logdet = 2 * np.sum(np.log(np.diag(L)[:n1]))
    return L, alpha, logdet


@pytest.mark.parametrize("ks", KERNELS)
@pytest.mark.parametrize("n,k", [(300, 1), (300, 100), (256, 1), (200, 700)])
def test_block_boundary_algebra_matches_oracle(ks, n, k):
    sigma, d, m = 0.5, 3, 2
    X, Y = make_data(n + k, d, m)
    Xp, Yp = make_data(n, d, m)
    assert np.array_equal(X[:n], Xp) and np.array_equal(Y[:n], Yp)  # a prefix fit can be appended to
    L_old = padded_factor(O.kernel_matrix(ks, X[:n]) + sigma * sigma * np.eye(n), n)
    L, alpha, logdet = append_factor(ks, X, Y, sigma, n, L_old)
    a_ref, _ = O.fit(ks, X, Y, sigma)
    assert relerr(alpha, a_ref) <= 1e-12
    Kf = O.kernel_matrix(ks, X) + sigma * sigma * np.eye(n + k)
    assert abs(logdet - np.linalg.slogdet(Kf)[1]) <= 1e-12 * abs(logdet)
    assert relerr(L[:n + k, :n + k], np.linalg.cholesky(Kf)) <= 1e-12
    # the padding stays the identity at the end of the factor
    pad = L[n + k:, :]
    assert np.array_equal(pad[:, n + k:], np.eye(pad.shape[0])) and not pad[:, :n + k].any()
