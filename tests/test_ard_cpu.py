"""Per-dimension length scales on the CPU side: the numpy reference of tests/ard_ref.py is itself
checked here, so that the GPU tests compare against something known to be right -- its gradient in
the length scales (direct differences, 1/2 sum w_ab dK_ab/d ell_j) against central differences of
its own value, <= 1e-7 normwise relative, and the conditioning of every fixture (<= 2e3, so the
project's 1e-6 / 1e-3 tolerances leave room for cond * eps)."""
import numpy as np
import pytest

from tests import ard_ref as A
from tests.helpers import relerr


@pytest.mark.parametrize("n,d", A.SHAPES)
@pytest.mark.parametrize("name", A.NAMES)
def test_reference_gradient_matches_central_differences(name, n, d):
    X, Y, ell, Z, g = A.fixture(name, n, d)
    c = A.cond(A.NODES[name], Z)
    fd = A.fd_grad_ell(A.NODES[name], X, Y, ell)
    err = relerr(g, fd)
    print(f"ard_ref {name} ({n}, {d}): cond {c:.3g}, |grad| {np.max(np.abs(g)):.3g}, fd err {err:.2e}")
    assert g.shape == (d,)
    assert c <= 2e3
    assert err <= 1e-7


def test_scaled_points_follow_the_dtype():
    """Z is ONE division in the model's dtype with ell narrowed first -- what the header promises."""
    X, Y, ell, Z, _ = A.fixture("gauss", 129, 33, np.float32)
    assert Z.dtype == np.float32
    assert np.array_equal(Z, X / ell.astype(np.float32))
    assert np.all((ell >= 0.5 * np.sqrt(33 / 3.0)) & (ell <= 3.0 * np.sqrt(33 / 3.0)))


def test_product_rule_against_a_difference_in_r2():
    """dk/dr2 of the product tree against a central difference of its value along one pair."""
    node = A.NODES["m32_x_gauss"]
    z = np.array([[0.0, 0.0], [0.6, 0.3]])
    h = 1e-6
    _, G = A.k_and_g(node, z)
    r = np.sqrt(0.45)
    kp = A.k_and_g(node, np.array([[0.0], [np.sqrt(r * r + h)]]))[0][0, 1]
    km = A.k_and_g(node, np.array([[0.0], [np.sqrt(r * r - h)]]))[0][0, 1]
    assert abs(G[0, 1] - (kp - km) / (2 * h)) <= 1e-8 * abs(G[0, 1])
