"""Per-dimension length scales through the C++ host API (GaussianProcess<T>::SetLengthScales /
GetLengthScales, GaussianLogLikelihood<T>::GetLengthScaleDerivatives): tests/cpp/ard_test.cpp,
built by `make cpptests`, against what the Python binding returns for the same model, which this
test writes out for it."""
import os
import subprocess

import pytest

from tests import ard_ref as A
from tests.helpers import make_data, make_queries, relerr, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_length_scales(ctx, tmp_path):
    import gpr_amd
    import numpy as np
    n, d, q, ksigma, kscale = 200, 4, 9, 1.1, 0.9
    X, Y = make_data(n, d, 1)
    Xq = make_queries(q, d)
    ell = A.length_scales(d)
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X, Y)
    M.set_kernel(f"GaussianKernel({ksigma!r},{kscale!r},)")
    M.set_noise(A.SIGMA)
    M.set_length_scales(ell)
    M.fit()
    mean = M.predict(Xq)
    g = M.lml_scale_grad()
    M.close()
    # (the Python results are themselves right: the reference on the scaled points)
    assert relerr(g, A.grad_ell(gpr_amd.kernels.Gaussian(ksigma, kscale), X / ell, Y, ell)) <= TOL[np.dtype(np.float64)]
    f = tmp_path / "expected.txt"
    with open(f, "w") as out:
        out.write(f"{n} {d} {q} {A.SIGMA!r} {ksigma!r} {kscale!r}\n")
        out.write(" ".join(repr(float(t)) for t in ell) + "\n")
        out.write(" ".join(repr(float(t)) for t in g) + "\n")
        for i in range(n):
            out.write(" ".join(repr(float(t)) for t in (*X[i], Y[i, 0])) + "\n")
        for i in range(q):
            out.write(" ".join(repr(float(t)) for t in (*Xq[i], mean[i, 0])) + "\n")
    exe = os.path.join(ROOT, "gpr_amd", "lib", "ard_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0, r.stdout + r.stderr
    assert lines == ["PASS ReadExpected", "PASS SetGetPredict", "PASS LengthScaleDerivatives", "PASS Refusals"], r.stdout
