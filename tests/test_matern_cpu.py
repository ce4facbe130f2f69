"""Matern 3/2 and 5/2 on the CPU side of the boundary: gpr_amd/kernels.py (constructors, the
string form, the post-order program, parameter counts and order, the refusals), the fixture trees
of tests/matern_ref.py (their conditioning, and the numpy reference's own gradient against central
differences), and the C++ host classes through tests/cpp/matern_cpu_test.cpp."""
import os
import subprocess

import numpy as np
import pytest

from gpr_amd import kernels as kn
from tests.helpers import make_data
from tests import matern_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpr_amd", "lib")


def test_constructors_and_round_trip():
    import gpr_amd
    assert gpr_amd.Matern32 is kn.Matern32 and gpr_amd.Matern52 is kn.Matern52
    a, b = kn.Matern32(0.9, 1.2), kn.Matern52(0.8)
    assert a.name == "Matern32Kernel" and a.params == [0.9, 1.2]
    assert b.name == "Matern52Kernel" and b.params == [0.8, 1.0]
    assert a.to_string() == "Matern32Kernel(0.9,1.2,)" and b.to_string() == "Matern52Kernel(0.8,1,)"
    for name, node in R.NODES.items():
        back = kn.parse_kernel(node.to_string())
        assert back == node, name
        assert back.to_string() == R.TREES[name]


def test_postorder_ops():
    assert kn.OP["Matern32Kernel"] == 8 and kn.OP["Matern52Kernel"] == 9
    assert kn.Matern32(0.9, 1.2).postorder() == [(8, [0.9, 1.2])]
    assert kn.Matern52(0.8, 1.1).postorder() == [(9, [0.8, 1.1])]
    prog = R.NODES["m52per_m32"].postorder()
    assert [op for op, _ in prog] == [9, 5, 7, 8, 6]
    assert prog[0][1] == [1.4, 1.0] and prog[3][1] == [0.7, 0.8]


def test_parameter_counts_and_order():
    assert kn.NPARAMS["Matern32Kernel"] == 2 and kn.NPARAMS["Matern52Kernel"] == 2
    assert R.NODES["m32"].num_params() == 2 and R.NODES["m52"].num_params() == 2
    n = R.NODES["rq_m32"]  # a three-parameter leaf, then the Matern leaf last
    assert n.num_params() == 5 and n.parameters() == [0.7, 0.9, 1.5, 0.8, 1.0]
    n = R.NODES["m32_per"]  # the Matern leaf first
    assert n.num_params() == 5 and n.parameters() == [1.1, 0.9, 0.8, 2.5, 0.8]
    n = R.NODES["2per_m52"]
    assert n.num_params() == 8 and n.parameters() == [0.7, 2.5, 0.8, 0.9, 0.9, 0.5, 1.3, 1.1]


@pytest.mark.parametrize("name", ["Matern32Kernel", "Matern52Kernel"])
def test_refusals(name):
    with pytest.raises(kn.KernelError, match=f"{name}: sigma has to be positive"):
        kn.parse_kernel(f"{name}(0,1,)")
    with pytest.raises(kn.KernelError, match=f"{name}: scale has to be positive"):
        kn.parse_kernel(f"{name}(1,0,)")
    with pytest.raises(kn.KernelError, match=f"{name}::Load: wrong number of kernel parameters."):
        kn.parse_kernel(f"{name}(1,)")
    with pytest.raises(kn.KernelError, match=f"{name}::Load: wrong number of kernel parameters."):
        kn.parse_kernel(f"SumKernel(GaussianKernel(1,1,),{name}(1,2,3,))")
    with pytest.raises(kn.KernelError, match=f"{name}: sigma has to be positive"):
        kn.validate(kn.KernelNode(name, [0.0, 1.0]))
    with pytest.raises(kn.KernelError, match="failed to load kernel"):
        kn.parse_kernel("Matern12Kernel(1,1,)")


def test_fixture_trees():
    """cond(K + sigma^2 I) <= 2e3 at sigma = 0.5 on make_data(300, 3): every fit below sits well
    inside 1 / tolerance."""
    X, _ = make_data(300, 3)
    for name in R.NAMES:
        K = R.kmat(R.NODES[name], X) + R.SIGMA ** 2 * np.eye(300)
        c = np.linalg.cond(K)
        print(f"cond {name}: {c:.3e}")
        assert c <= 2e3, (name, c)
        assert np.array_equal(np.diag(R.kmat(R.NODES[name], X)), np.full(300, R.diag_value(R.NODES[name])))


def test_reference_gradient():
    """The numpy reference's dK/dtheta planes against central differences of its own values, with
    duplicate samples (r = 0) and near-duplicates in the set: finite everywhere, no division by r."""
    X, _ = make_data(24, 3)
    X = np.vstack([X, X[:3], X[3:6] + 1e-9])
    h = 1e-6
    for name, node in R.NODES.items():
        D = R.dmat(node, X)
        assert D.shape == (node.num_params(), 30, 30) and np.all(np.isfinite(D))
        p = node.parameters()
        for q in range(len(p)):
            def at(v):
                pp = list(p)
                pp[q] = v
                return R.kmat(R.with_params(node, pp), X)
            fd = (at(p[q] + h) - at(p[q] - h)) / (2 * h)
            assert np.max(np.abs(fd - D[q])) <= 1e-8 * max(1.0, np.max(np.abs(D[q]))), (name, q)


def test_cpp_host_classes():
    """KernelFactory round trip, operator() against the closed form, GetDerivative against central
    differences at r = 0, small r and large r, SetParameters size errors: no device needed."""
    path = os.path.join(LIB, "matern_cpu_test")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0, out
    assert len(lines) == 4 and all(l.startswith("PASS") for l in lines), out
