"""Leave-one-out cross-validation (gprx_model_loo) without a GPU: the numpy restatement the GPU
tests compare with (tests/loo_ref.py) against brute-force refits and central differences, the ABI
addition, and the C++ class failing loudly when no GPU is visible.  Measured with this file:
mu and s2 within 1.5e-14 of the brute force, gradients within 2.6e-9 of the central differences."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from gpr_amd import gprx
from gpr_amd import kernels as kn
from tests import loo_ref as L
from tests.helpers import make_data, relerr
from tests.matern_ref import with_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = ["GaussianKernel(0.7,1.3,)",
         "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))",
         "Matern52Kernel(0.8,1.1,)"]
N, D, SIGMA = 60, 2, 0.4


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("ks", TREES)
def test_restatement_against_brute_force(ks, m):
    X, Y = make_data(N, D, m)
    v, mu, s2, _ = L.loo(ks, X, Y, SIGMA)
    K, _ = L.matrices(ks, X)
    mu_b, s2_b = L.brute_force(K + SIGMA * SIGMA * np.eye(N), Y)
    print(f"loo restatement {ks} m={m}: mu {relerr(mu, mu_b):.2e}, s2 {relerr(s2, s2_b):.2e}")
    assert relerr(mu, mu_b) <= 1e-10 and relerr(s2, s2_b) <= 1e-10
    v_b = np.sum(-0.5 * np.log(s2_b)[:, None] - (Y - mu_b) ** 2 / (2 * s2_b[:, None]) - 0.5 * np.log(2 * np.pi))
    assert abs(v - v_b) <= 1e-10 * max(1.0, abs(v_b))
    assert np.all(s2 > 0) and mu.shape == (N, m) and s2.shape == (N,)


@pytest.mark.parametrize("ks", TREES)
def test_gradient_against_central_differences(ks):
    X, Y = make_data(N, D, 1)
    _, _, _, g = L.loo(ks, X, Y, SIGMA, grad=True)
    node = kn.parse_kernel(ks)
    p0 = node.parameters()
    assert g.shape == (len(p0),)
    h = 1e-5
    fd = np.empty(len(p0))
    for i in range(len(p0)):
        pp, pm = list(p0), list(p0)
        pp[i] += h
        pm[i] -= h
        fd[i] = (L.loo(with_params(node, pp).to_string(), X, Y, SIGMA)[0] -
                 L.loo(with_params(node, pm).to_string(), X, Y, SIGMA)[0]) / (2 * h)
    print(f"loo gradient {ks}: {relerr(g, fd):.2e}")
    assert relerr(g, fd) <= 1e-6, (g, fd)


def test_symbol_exported_and_declared():
    lib = ctypes.CDLL(gprx.LIB_PATH)
    assert hasattr(lib, "gprx_model_loo")
    assert "gprx_model_loo" in gprx.EXPORTED
    assert hasattr(gprx.Model, "loo")
    assert lib.gprx_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "gprx.h")).read()
    assert re.search(r"gprx_status gprx_model_loo\(gprx_model\* model, uint32_t flags, double\* value,\s*void\* mean, "
                     r"void\* var, double\* grad,\s*int32_t\* nparams\);", header)
    assert int(re.search(r"#define GPRX_LOO_GRAD (\d+)u", header).group(1)) == gprx.LOO_GRAD == 1


def test_cpp_class_throws_without_a_gpu():
    """(the child sees no device, whatever this machine has)"""
    exe = os.path.join(ROOT, "gpr_amd", "lib", "loo_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([exe, "--no-device"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))] == ["PASS NoDeviceFailsLoudly"]
