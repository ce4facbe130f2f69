"""numpy fp64 restatement of per-dimension length scales (gprx_model_set_length_scales,
gprx_model_lml_scale_grad; k_ard.hip): the model's kernel is k_tree(x / ell, y / ell), and

    dLML/d ell_j = 1/2 sum_ab (alpha_a alpha_b - C_ab) dK_ab/d ell_j,
    dK_ab/d ell_j = -(2 / ell_j) dk_tree/dr2(a, b) (z_aj - z_bj)^2,   z = x / ell,

summed here from the direct differences (z_aj - z_bj), NOT from the expansion
z_a^2 h_a - z_a (H Z)_a the device kernel multiplies out.  Values come from tests/matern_ref.py;
dk/dr2 is evaluated recursively over KernelNode beside them.  The fixture trees are r2-only (the
gradient refuses Periodic leaves) and are shared by tests/test_ard_cpu.py and tests/test_gpu_ard*.py."""
import numpy as np

from gpr_amd import kernels as kn
from tests import matern_ref as R
from tests.helpers import SEED, make_data, uniform

SIGMA = 0.5

NODES = {
    "gauss": kn.Gaussian(1.1, 0.9),
    "m32": R.NODES["m32"],
    "m52": R.NODES["m52"],
    "rq_m32": R.NODES["rq_m32"],
    "m32_x_gauss": R.NODES["m32_x_gauss"],
    "gauss_white": kn.Sum(kn.Gaussian(0.9, 1.0), kn.White(0.3)),
}
TREES = {name: node.to_string() for name, node in NODES.items()}
NAMES = list(TREES)
SHAPES = [(129, 33), (260, 5), (300, 3)]  # the shapes of the CPU check of the identity


def length_scales(d, seed=SEED + 0xA4D):
    """ell_j log-uniform in [0.5, 3] sqrt(d / 3), from the project's generator."""
    return np.exp(np.log(0.5) + uniform(seed, d) * np.log(6.0)) * np.sqrt(d / 3.0)


def scaled(X, ell, dtype=np.float64):
    """X / ell as the model forms it: ell narrowed to dtype, one division in dtype."""
    dtype = np.dtype(dtype)
    return np.asarray(X, dtype) / np.asarray(ell, np.float64).astype(dtype)


def _r2(Z):
    df = Z[:, None, :] - Z[None, :, :]
    return np.sum(df * df, axis=-1)


def _leaf_g(node, r2):
    """dk/dr2 of one r2 leaf (finite at r2 = 0)."""
    p, nm = node.params, node.name
    if nm == "GaussianKernel":
        sig, sc = p
        return -0.5 / sig ** 2 * sc * sc * np.exp(-0.5 * r2 / sig ** 2)
    if nm == "GaussianExpKernel":
        sig, sc = p
        return -0.5 * np.exp(-2 * sig) * np.exp(2 * sc) * np.exp(-0.5 * r2 * np.exp(-2 * sig))
    if nm == "WhiteKernel":
        return np.zeros_like(r2)
    if nm == "RationalQuadraticKernel":
        sc, sig, al = p
        f = 1 + 0.5 * r2 / (sig * sig * al)
        return -0.5 * sc * sc / (sig * sig) * f ** (-al - 1)
    if nm in ("Matern32Kernel", "Matern52Kernel"):
        l, s = p
        if nm == "Matern32Kernel":
            a = np.sqrt(3.0 * r2) / abs(l)
            return -1.5 * s * s / (l * l) * np.exp(-a)
        a = np.sqrt(5.0 * r2) / abs(l)
        return -(5.0 / 6.0) * s * s / (l * l) * (1 + a) * np.exp(-a)
    raise ValueError("ard_ref: no dk/dr2 for " + nm)


def k_and_g(node, Z):
    """(K, dK/dr2) of the tree on all pairs of the rows of Z, by the product rule."""
    node = kn.as_node(node)
    Z = np.asarray(Z, np.float64)
    if node.is_leaf:
        return R.kmat(node, Z), _leaf_g(node, _r2(Z))
    k1, g1 = k_and_g(node.k1, Z)
    k2, g2 = k_and_g(node.k2, Z)
    if node.name == "SumKernel":
        return k1 + k2, g1 + g2
    return k1 * k2, g1 * k2 + k1 * g2


def lml_value(node, Z, y, sigma=SIGMA):
    """The LML of the model on the (already scaled) points Z, gprx_model_lml's convention."""
    Z = np.asarray(Z, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    n = Z.shape[0]
    Kn = R.kmat(kn.as_node(node), Z) + sigma * sigma * np.eye(n)
    a = np.linalg.solve(Kn, y)
    return float(-0.5 * y @ a - 0.5 * np.linalg.slogdet(Kn)[1] - 0.5 * n * np.log(2 * np.pi))


def cond(node, Z, sigma=SIGMA):
    Z = np.asarray(Z, np.float64)
    return float(np.linalg.cond(R.kmat(kn.as_node(node), Z) + sigma * sigma * np.eye(Z.shape[0])))


def grad_ell(node, Z, y, ell, sigma=SIGMA):
    """dLML/d ell (d,) at the scaled points Z = X / ell, from direct differences."""
    Z = np.asarray(Z, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    ell = np.asarray(ell, np.float64)
    n, d = Z.shape
    K, G = k_and_g(node, Z)
    Kn = K + sigma * sigma * np.eye(n)
    a = np.linalg.solve(Kn, y)
    W = np.outer(a, a) - np.linalg.inv(Kn)
    WG = W * G
    out = np.empty(d)
    for j in range(d):
        dz = Z[:, None, j] - Z[None, :, j]
        out[j] = 0.5 * np.sum(WG * (-(2.0 / ell[j]) * dz * dz))
    return out


def fd_grad_ell(node, X, y, ell, sigma=SIGMA, h=1e-5):
    """Central differences of lml_value in every ell_j (relative step h)."""
    X = np.asarray(X, np.float64)
    ell = np.asarray(ell, np.float64)
    out = np.empty(ell.shape[0])
    for j in range(ell.shape[0]):
        ep, em = ell.copy(), ell.copy()
        ep[j] *= 1 + h
        em[j] *= 1 - h
        out[j] = (lml_value(node, X / ep, y, sigma) - lml_value(node, X / em, y, sigma)) / (ep[j] - em[j])
    return out


_cache = {}


def fixture(name, n, d, dtype=np.float64):
    """(X, Y, ell, Z, grad_ell reference) in dtype for tree `name`, computed once, read-only.  Z and
    the reference follow the dtype's own division, so they describe the model the device holds."""
    key = (name, n, d, np.dtype(dtype).str)
    if key not in _cache:
        X, Y = make_data(n, d, dtype=dtype)
        ell = length_scales(d)
        Z = scaled(X, ell, dtype)
        ell_t = ell.astype(dtype).astype(np.float64)
        g = grad_ell(NODES[name], Z, Y, ell_t)
        for a in (X, Y, ell, Z, g):
            a.setflags(write=False)
        _cache[key] = (X, Y, ell, Z, g)
    return _cache[key]


# ---- what the GPU tests observe (here so that a child process can collect it too) ----------
EQ_NODES = {
    "gauss": NODES["gauss"],
    "gauss_per": kn.Sum(kn.Gaussian(1.1, 0.9), kn.Periodic(0.8, 2.5, 0.8)),
    "m32_white": R.NODES["m32_white"],
    "rq": kn.RationalQuadratic(0.7, 0.9, 1.5),
}
EQ_SHAPES = [(129, 33), (260, 5), (128, 16)]
Q = 37  # query points of an observation


def _observe(ctx, vctx, node, X, Y, Xq, Xa, Ya, ell, dtype, out, tag, sharded_cov):
    """Every read of the equivalence check from one model: X, Xq, Xa as given with `ell` set, or
    (ell None) already scaled by the caller."""
    import gpr_amd

    def new(c):
        M = gpr_amd.Model(c, dtype)
        if ell is not None:
            M.set_length_scales(ell)
        M.set_data(X, Y)
        M.set_kernel(node.to_string())
        M.set_noise(SIGMA)
        return M

    M = new(ctx)
    M.fit()
    out[tag + "alpha"] = M.alpha()
    out[tag + "predict"] = M.predict(Xq)
    out[tag + "posterior_cov"] = M.posterior_cov(Xq, Xq[::-1].copy())
    mean, cov = M.posterior(Xq)
    out[tag + "posterior.mean"], out[tag + "posterior.cov"] = mean, cov
    out[tag + "sample"] = M.sample(Xq, n=3, seed=7)[0]
    v, mu, s2, _ = M.loo()
    out[tag + "loo.value"], out[tag + "loo.mean"], out[tag + "loo.var"] = np.float64(v), mu, s2
    v, g, ld = M.lml(grad=True)
    out[tag + "lml.value"], out[tag + "lml.grad"], out[tag + "lml.logdet"] = np.float64(v), g, np.float64(ld)
    M.fit()
    M.append(Xa[:1], Ya[:1])
    out[tag + "append1.alpha"] = M.alpha()
    M.append(Xa[1:131], Ya[1:131])
    out[tag + "append130.alpha"] = M.alpha()
    out[tag + "append130.predict"] = M.predict(Xq)
    M.remove(3, 2)
    out[tag + "remove.alpha"] = M.alpha()
    out[tag + "remove.predict"] = M.predict(Xq)
    M.close()
    V = new(vctx)
    V.fit()
    out[tag + "virtual.alpha"] = V.alpha()
    out[tag + "virtual.predict"] = V.predict(Xq)
    if sharded_cov:
        out[tag + "virtual.posterior_cov"] = V.posterior_cov(Xq, Xq)
    V.close()


def gpu_equivalence(ctx, vctx, name, n, d, dtype, sharded_cov=True):
    """{"s.<read>": a model with scales on X, "p.<read>": a model without on X / ell}.  sharded_cov:
    also the sharded fit's posterior_cov (the distributed solve of the queries; not part of the fit)."""
    from tests.helpers import make_queries
    dtype = np.dtype(dtype)
    X, Y = make_data(n + 131, d, dtype=dtype)
    Xq = make_queries(Q, d, dtype=dtype)
    ell = length_scales(d)
    out = {}
    node = EQ_NODES[name]
    _observe(ctx, vctx, node, X[:n], Y[:n], Xq, X[n:], Y[n:], ell, dtype, out, "s.", sharded_cov)
    _observe(ctx, vctx, node, scaled(X[:n], ell, dtype), Y[:n], scaled(Xq, ell, dtype), scaled(X[n:], ell, dtype),
             Y[n:], None, dtype, out, "p.", sharded_cov)
    return out


def gpu_equivalence_all(ctx, vctx, dtypes=(np.float64, np.float32), sharded_cov=True):
    out = {}
    for name in EQ_NODES:
        for (n, d) in EQ_SHAPES:
            for dt in dtypes:
                o = gpu_equivalence(ctx, vctx, name, n, d, dt, sharded_cov)
                out.update({f"{name}.{n}.{d}.{np.dtype(dt).name}.{k}": v for k, v in o.items()})
    return out
