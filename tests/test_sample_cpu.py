"""The numpy restatement of posterior sampling (tests/sample_ref.py) on its own: the generator's
known answers and statistics, the restated posterior against a brute-force one, and the library's
new entry points.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

from gpr_amd import gprx
from tests import loo_ref as L
from tests import sample_ref as S
from tests.helpers import make_data, make_queries, relerr


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words(*w):
    return np.array(w, np.uint64)


def test_philox_known_answers():
    """Random123's published vectors for philox4x32_10 (kat_vectors)."""
    cases = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in cases:
        got = S.philox4x32_10(words(*ctr), words(*key))
        assert [int(x) for x in got] == list(want), [hex(int(x)) for x in got]
    # (vectorised over counters: the same words)
    got = S.philox4x32_10(np.array([c[0] for c in cases], np.uint64), np.array([c[1] for c in cases], np.uint64))
    assert got.shape == (3, 4) and [[int(x) for x in r] for r in got] == [list(c[2]) for c in cases]


def test_normals_do_not_depend_on_the_count():
    full = S.normals(99, 1001)
    assert full.shape == (1001,) and full.dtype == np.float64
    for count in (0, 1, 2, 3, 257, 1000):
        assert np.array_equal(S.normals(99, count), full[:count])
    assert not np.array_equal(S.normals(100, 16), full[:16])
    assert not np.array_equal(S.normals(99 + 2 ** 32, 16), full[:16])  # (the seed's high word is the key's second)


def test_normals_statistics():
    """2^20 normals of seed 12345: the first four moments and the even/odd and lag-1 correlations,
    each within 5 standard errors of a standard normal's (var z = 1, var z^2 = 2, var z^3 = 15,
    var z^4 = 96, var of a product of two independent ones = 1)."""
    n = 1 << 20
    z = S.normals(12345, n)
    assert np.all(np.isfinite(z)) and np.max(np.abs(z)) < 9
    scores = {
        "mean": np.mean(z) / np.sqrt(1.0 / n),
        "variance": (np.mean(z * z) - 1.0) / np.sqrt(2.0 / n),
        "third": np.mean(z ** 3) / np.sqrt(15.0 / n),
        "fourth": (np.mean(z ** 4) - 3.0) / np.sqrt(96.0 / n),
        "even_odd": np.mean(z[0::2] * z[1::2]) / np.sqrt(2.0 / n),
        "lag1": np.mean(z[:-1] * z[1:]) / np.sqrt(1.0 / (n - 1)),
    }
    print("normals z-scores:", {k: round(float(v), 2) for k, v in scores.items()})
    for k, v in scores.items():
        assert abs(v) < 5, (k, v)


def test_restated_posterior_against_the_explicit_inverse():
    for ks, m in ((L.GAUSS, 1), (L.C3, 2), (L.GRAD_TREES["matern32"], 1)):
        X, Y = make_data(150, 3, m)
        Xq = make_queries(40, 3)
        mean, Sigma = S.posterior(ks, X, Y, Xq, 0.5)
        Kall, _ = L.matrices(ks, np.concatenate([X, Xq]))
        bmean, bSigma = S.posterior_brute(Kall[:150, :150], Kall[150:, :150], Kall[150:, 150:], Y, 0.5)
        assert mean.shape == (40, m) and Sigma.shape == (40, 40)
        assert relerr(mean, bmean) < 1e-10 and relerr(Sigma, bSigma) < 1e-10
        assert np.array_equal(Sigma, Sigma.T)
        _, noisy = S.posterior(ks, X, Y, Xq, 0.5, noise=True)
        assert relerr(noisy, Sigma + 0.25 * np.eye(40)) < 1e-15


def test_restated_sample():
    """With Z = I the draws' deviations are the factor's columns; the sample covariance of many
    draws approaches Sigma."""
    X, Y = make_data(100, 3, 2)
    Xq = make_queries(6, 3)
    mean, Sigma = S.posterior(L.GAUSS, X, Y, Xq, 0.5, noise=True)
    D = S.sample(mean[:, :1], Sigma, 0.0, np.eye(6)[:, None, :])[:, :, 0] - mean[:, 0]
    assert np.all(np.tril(D, -1) == 0) and relerr(D.T @ D, Sigma) < 1e-13
    n = 40000
    draws = S.sample(mean, Sigma, 0.0, S.normals(3, n * 2 * 6).reshape(n, 2, 6))
    assert draws.shape == (n, 6, 2)
    dev = draws - mean[None]
    for c in range(2):
        emp = dev[:, :, c].T @ dev[:, :, c] / n
        assert relerr(emp, Sigma) < 5 * np.sqrt(2.0 / n)  # (an entry's standard error is at most sqrt(2 / n) |Sigma|)
    assert abs(np.mean(dev)) < 5 * np.sqrt(np.max(Sigma) / n)  # (entries of one draw are correlated)


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(gprx.LIB_PATH)
    for name in ("gprx_model_posterior", "gprx_model_sample", "gprx_dev_normals"):
        assert hasattr(lib, name), name
    assert {"gprx_model_posterior", "gprx_model_sample"} <= set(gprx.EXPORTED)
    assert all(hasattr(gprx.Model, f) for f in ("posterior", "sample")) and hasattr(gprx.Context, "normals")
    assert lib.gprx_abi_version() == 2
    assert gprx.POST_NOISE == 1


def test_cpp_class_throws_without_a_gpu():
    """(the child sees no device, whatever this machine has)"""
    exe = os.path.join(ROOT, "gpr_amd", "lib", "sample_test")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([exe, "--no-device"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))] == ["PASS NoDeviceFailsLoudly"]
