"""numpy references (fp64, direct differences) for kernel trees that hold Matern leaves, and the
fixture trees shared by tests/test_matern_cpu.py and tests/test_gpu_matern*.py.  The CPU oracle
does not know these kernels; every reference here is evaluated recursively over KernelNode."""
import numpy as np

from gpr_amd import kernels as kn

SIGMA = 0.5

_PER = kn.Periodic(0.8, 2.5, 0.8)
NODES = {
    "m32": kn.Matern32(0.9, 1.2),
    "m52": kn.Matern52(0.8, 1.1),
    "gauss_m52": kn.Sum(kn.Gaussian(0.7, 0.9), kn.Matern52(1.3, 0.8)),
    "m32_per": kn.Sum(kn.Matern32(1.1, 0.9), _PER),
    "rq_m32": kn.Sum(kn.RationalQuadratic(0.7, 0.9, 1.5), kn.Matern32(0.8, 1.0)),
    "m32_x_gauss": kn.Product(kn.Matern32(1.2, 1.1), kn.Gaussian(1.5, 1.0)),
    "m52per_m32": kn.Sum(kn.Product(kn.Matern52(1.4, 1.0), _PER), kn.Matern32(0.7, 0.8)),
    "m32_white": kn.Sum(kn.Matern32(0.9, 1.1), kn.White(0.3)),
    "2per_m52": kn.Sum(kn.Sum(kn.Periodic(0.7, 2.5, 0.8), kn.Matern52(0.9, 0.9)), kn.Periodic(0.5, 1.3, 1.1)),
}
TREES = {name: node.to_string() for name, node in NODES.items()}
NAMES = list(TREES)
# the stand-alone MFMA build / predict carries these (no White leaf, one periodic leaf at most)
MMA = ["m32", "m52", "gauss_m52", "m32_per", "rq_m32", "m32_x_gauss", "m52per_m32"]
# a White leaf / two periodic leaves: the VALU build and predict
VALU =["m32_white", "2per_m52"]
SUMS = ["gauss_m52", "m32_per"]  # through append, LU, sparse, sharded


def _diffs(A, B):
    return A[:, None, :] - B[None, :, :]


def _leaf(node, A, B, grad):
    """(K, [dK/dp ...]) of one leaf on all pairs (rows of A) x (rows of B)."""
    df = _diffs(np.asarray(A, np.float64), np.asarray(B, np.float64))
    r2 = np.sum(df * df, axis=-1)
    p = node.params
    nm = node.name
    if nm in ("Matern32Kernel", "Matern52Kernel"):
        l, s = p
        a = np.sqrt((3.0 if nm == "Matern32Kernel" else 5.0) * r2) / abs(l)
        e = np.exp(-a)
        if nm == "Matern32Kernel":
            poly, dl = 1 + a, s * s * a * a * e / l
        else:
            poly, dl = 1 + a + a * a / 3, s * s * (a * a / 3) * (1 + a) * e / l
        return s * s * poly * e, ([dl, 2 * s * poly * e] if grad else None)
    if nm == "GaussianKernel":
        sig, sc = p
        e = np.exp(-0.5 * r2 / sig ** 2)
        return sc * sc * e, ([sc * sc * r2 / sig ** 3 * e, 2 * sc * e] if grad else None)
    if nm == "GaussianExpKernel":
        sig, sc = p
        e = np.exp(2 * sc) * np.exp(-0.5 * r2 * np.exp(-2 * sig))
        return e, ([r2 * np.exp(-2 * sig) * e, 2 * e] if grad else None)
    if nm == "WhiteKernel":
        z = (r2 == 0).astype(np.float64)
        return p[0] ** 2 * z, ([2 * p[0] * z] if grad else None)
    if nm == "RationalQuadraticKernel":
        sc, sig, al = p
        f = 1 + 0.5 * r2 / (sig * sig * al)
        pw = f ** (-al)
        g = [2 * sc * pw, sc * sc * r2 * pw / f / sig ** 3, sc * sc * (r2 / (2 * sig * sig * f * al) - np.log(f)) * pw]
        return sc * sc * pw, (g if grad else None)
    assert nm == "PeriodicKernel", nm
    sc, b, sig = p
    S = np.sum(np.sin(b * df) ** 2, axis=-1)
    F = np.sum(2 * df * np.cos(b * df) * np.sin(b * df), axis=-1)
    e = np.exp(-0.5 * S / sig ** 2)
    g = [2 * sc * e, -0.5 * sc * sc * e * F / sig ** 2, sc * sc * e * S / sig ** 3]
    return sc * sc * e, (g if grad else None)


def _eval(node, A, B, grad):
    if node.is_leaf:
        return _leaf(node, A, B, grad)
    k1, g1 = _eval(node.k1, A, B, grad)
    k2, g2 = _eval(node.k2, A, B, grad)
    if node.name == "SumKernel":
        return k1 + k2, (g1 + g2 if grad else None)
    return k1 * k2, ([g * k2 for g in g1] + [g * k1 for g in g2] if grad else None)


def cross(node, A, B):
    """K(A, B) in fp64."""
    return _eval(kn.as_node(node), A, B, False)[0]


def kmat(node, X):
    return cross(node, X, X)


def dmat(node, X):
    """The stacked dK/dtheta planes (P, n, n), GetParameters() order."""
    return np.stack(_eval(kn.as_node(node), X, X, True)[1])


def with_params(node, p):
    """The same tree with the parameter vector p (GetParameters() order)."""
    if node.is_leaf:
        return kn.KernelNode(node.name, list(p))
    n1 = node.k1.num_params()
    return kn.KernelNode(node.name, k1=with_params(node.k1, p[:n1]), k2=with_params(node.k2, p[n1:]))


def diag_value(node):
    """k(x, x): the sum over product terms of the leaves' s^2."""
    z = np.zeros((1, 1))
    return float(cross(node, z, z)[0, 0])


_cache = {}


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def ref_fit(name, X, Y, sigma=SIGMA, key=None):
    """(alpha, C = (K + sigma^2 I)^-1, log det) from numpy, computed once per key, read-only."""
    if key is not None and key in _cache:
        return _cache[key]
    n = X.shape[0]
    Kn = kmat(NODES[name], np.asarray(X, np.float64)) + sigma * sigma * np.eye(n)
    C = np.linalg.inv(Kn)
    C = 0.5 * (C + C.T)
    out = _ro(np.linalg.solve(Kn, np.asarray(Y, np.float64)), C, float(np.linalg.slogdet(Kn)[1]))
    if key is not None:
        _cache[key] = out
    return out


def ref_predict(name, X, alpha, Xq, deriv=False):
    """mean = K(Xq, X) alpha and the derivative D[q, :, c] = -(xq - X)^T (k_q o alpha_c)."""
    Kx = cross(NODES[name], Xq, X)
    mean = Kx @ alpha
    if not deriv:
        return mean
    D = np.stack([-(Xq[i][None, :] - X).T @ (Kx[i][:, None] * alpha) for i in range(Xq.shape[0])])
    return mean, D


def ref_lml(name, X, y, sigma):
    """(value, gradient, log det): -y^T a / 2 - log det / 2 - n log(2 pi) / 2 and
    tr((a a^T - C) dK/dtheta) / 2."""
    n = X.shape[0]
    Kn = kmat(NODES[name], X) + sigma * sigma * np.eye(n)
    a = np.linalg.solve(Kn, y)
    ld = float(np.linalg.slogdet(Kn)[1])
    C = np.linalg.inv(Kn)
    W = np.outer(a, a) - C
    g = np.array([0.5 * np.sum(W * Dp) for Dp in dmat(NODES[name], X)])
    return float(-0.5 * y @ a - 0.5 * ld - 0.5 * n * np.log(2 * np.pi)), g, ld
