"""The joint posterior and posterior sampling through the C++ host API
(GaussianProcess<T>::GetPosterior, ::Sample): tests/cpp/sample_test.cpp, built by `make cpptests`,
against the values of the numpy restatement (tests/sample_ref.py), which this test writes out for
it."""
import os
import subprocess

import numpy as np
import pytest

from tests import sample_ref as S
from tests.helpers import make_data, make_queries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_posterior_and_sample(tmp_path):
    n, d, q, nsamp, seed, sigma, ksigma, kscale = 200, 3, 40, 3, 11, 0.5, 0.7, 1.3
    X, Y = make_data(n, d, 1)
    Xq = make_queries(q, d)
    mean, Sigma = S.posterior(f"GaussianKernel({ksigma!r},{kscale!r},)", X, Y, Xq, sigma)
    draws = S.sample(mean, Sigma + sigma ** 2 * np.eye(q), 0.0, S.normals(seed, nsamp * q).reshape(nsamp, 1, q))

    def row(values):
        return " ".join(repr(float(t)) for t in values) + "\n"

    f = tmp_path / "expected.txt"
    with open(f, "w") as out:
        out.write(f"{n} {d} {q} {nsamp} {seed} {sigma!r} {ksigma!r} {kscale!r}\n")
        for i in range(n):
            out.write(row((*X[i], Y[i, 0])))
        for p in range(q):
            out.write(row((*Xq[p], mean[p, 0])))
        for p in range(q):
            out.write(row(Sigma[p]))
        for i in range(nsamp):
            out.write(row(draws[i, :, 0]))
    exe = os.path.join(ROOT, "gpr_amd", "lib", "sample_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    assert r.returncode == 0, r.stdout + r.stderr
    assert lines == ["PASS ReadExpected", "PASS GetPosterior", "PASS Sample", "PASS QueuedSample"], r.stdout
