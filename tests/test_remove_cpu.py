"""gprx_model_remove without a GPU: the ABI additions, and the rotation sweep the device code
follows (k_remove.hip), restated in numpy (tests/remove_ref.py) against numpy's Cholesky of the
reduced matrix.  Measured with this file: backward error <= 9.3e-15 in f64 and <= 5.5e-6 in f32
(the fitted factor is the f64 one rounded to f32), at sigma = 1e-3 (condition number 1e8) too."""
import ctypes
import os
import re

import numpy as np
import pytest

from gpr_amd import gprx
from oracle import oracle as O
from tests.helpers import make_data
from tests.remove_ref import DB, backward_error, remove_factor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = "GaussianKernel(0.7,1.3,)"
CASES = [(300, 0, 1), (300, 44, 17), (640, 130, 5), (257, 0, 1), (300, 283, 17), (420, 100, 128)]
BOUND = {np.dtype(np.float64): 1e-13, np.dtype(np.float32): 1e-5}
_K = {}


def kernel_matrix(n):
    if n not in _K:
        X, _ = make_data(n, 3, 1)
        _K[n] = O.kernel_matrix(KS, X)
        _K[n].setflags(write=False)
    return _K[n]


def test_symbols_exported():
    lib = ctypes.CDLL(gprx.LIB_PATH)
    for s in ("gprx_model_remove", "gprx_dev_factor_update", "gprx_dev_factor_update_width"):
        assert hasattr(lib, s), s
    assert "gprx_model_remove" in gprx.EXPORTED
    assert hasattr(gprx.Model, "remove")
    assert lib.gprx_abi_version() == 2


def test_fit_info_keeps_its_layout_and_documents_the_removed_count():
    names = [f[0] for f in gprx.FitInfo._fields_]
    assert names[-1] == "appended"
    assert ctypes.sizeof(gprx.FitInfo) == 8 * 2 + 4 * 2 + 8 * 3 + 8 * 2 + 4 * 2
    assert gprx.FitInfo.appended.offset == ctypes.sizeof(gprx.FitInfo) - 4
    header = open(os.path.join(ROOT, "include", "gprx.h")).read()
    field = re.search(r"int32_t appended;.*?\*/", header, flags=re.S).group(0)
    assert "gprx_model_remove" in field and "-count" in field
    cut = int(re.search(r"#define GPRX_REMOVE_CUTOVER (\d+)", header).group(1))
    assert cut == gprx.REMOVE_CUTOVER


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("sigma", [0.5, 1e-3])
@pytest.mark.parametrize("n,f,r", CASES)
def test_rotation_sweep_matches_cholesky_of_the_reduced_matrix(n, f, r, sigma, dtype):
    Kf = kernel_matrix(n) + sigma * sigma * np.eye(n)
    L = np.linalg.cholesky(Kf).astype(dtype)  # the fitted factor, in the model's precision
    Lnew, n1 = remove_factor(L, f, r)
    assert Lnew.dtype == dtype and n1 == n - r
    keep = np.r_[0:f, f + r:n]
    Kr = Kf[np.ix_(keep, keep)]
    err = backward_error(Lnew[:n1, :n1], Kr)
    # against the Cholesky of the reduced matrix itself (f64: the factor is unique, so the
    # factors agree to cond * eps; the bound of the check is the backward error)
    Lr = np.linalg.cholesky(Kr)
    fwd = float(np.max(np.abs(Lnew[:n1, :n1] - Lr)) / np.max(np.abs(Lr)))
    print(f"remove n={n} f={f} r={r} sigma={sigma} {np.dtype(dtype).name}: backward {err:.2e}, factor {fwd:.2e}")
    assert err <= BOUND[np.dtype(dtype)]
    assert np.all(np.diag(Lnew) > 0)
    # rows above f are kept bit for bit; the identity padding stays at the end
    assert np.array_equal(Lnew[:f // DB * DB, :], np.pad(L[:f // DB * DB, :f // DB * DB],
                                                      ((0, 0), (0, Lnew.shape[1] - f // DB * DB))))
    pad = Lnew[n1:, :]
    assert np.array_equal(pad[:, n1:], np.eye(pad.shape[0])) and not pad[:, :n1].any()
