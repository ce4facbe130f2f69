"""Leave-one-out cross-validation through the C++ host API (GaussianProcess<T>::LeaveOneOut,
LeaveOneOutLogLikelihood<T>, GaussianProcessInference::Optimize over it): tests/cpp/loo_test.cpp,
built by `make cpptests`, against the values of the numpy restatement (tests/loo_ref.py), which
this test writes out for it."""
import os
import subprocess

import pytest

from tests import loo_ref as L
from tests.helpers import make_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_leave_one_out(tmp_path):
    n, d, sigma, ksigma, kscale = 200, 3, 0.5, 0.7, 1.3
    X, Y = make_data(n, d, 1)
    v, mu, s2, g = L.loo(f"GaussianKernel({ksigma!r},{kscale!r},)", X, Y, sigma, grad=True)
    f = tmp_path / "expected.txt"
    with open(f, "w") as out:
        out.write(f"{n} {d} {sigma!r} {ksigma!r} {kscale!r}\n{v!r}\n{float(g[0])!r} {float(g[1])!r}\n")
        for i in range(n):
            out.write(" ".join(repr(float(t)) for t in (*X[i], Y[i, 0], mu[i, 0], s2[i])) + "\n")
    exe = os.path.join(ROOT, "gpr_amd", "lib", "loo_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0, r.stdout + r.stderr
    assert lines == ["PASS ReadExpected", "PASS LeaveOneOut", "PASS LeaveOneOutLogLikelihood",
                     "PASS OptimizeLeaveOneOut"], r.stdout
