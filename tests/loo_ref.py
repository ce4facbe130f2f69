"""numpy restatement of leave-one-out cross-validation (gprx_model_loo, k_loo.hip; Rasmussen &
Williams, GPML 5.4.2), shared by tests/test_loo_cpu.py and tests/test_gpu_loo.py.  With
C = (K + sigma^2 I)^{-1}, c = diag(C), alpha = C y, per label column:

    mu_i = y_i - alpha_i / c_i,   s2_i = 1 / c_i,
    L    = sum_i -1/2 log s2_i - (y_i - mu_i)^2 / (2 s2_i) - 1/2 log 2 pi

and for m = 1, with u = alpha / c, a = C u, w = (1 + alpha^2 / c) / c, H = C diag(w) C:

    dL/dp = sum_kl dK_kl/dp (a_k alpha_l - H_kl / 2).
"""
import numpy as np

from oracle import oracle as O


GAUSS = "GaussianKernel(0.7,1.3,)"
C3 = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"
# the trees of the value + gradient cases: the first four on the MFMA pair statistics, the product
# on the VALU kernel
GRAD_TREES = {
    "gauss": GAUSS,
    "c3": C3,
    "matern32": "Matern32Kernel(0.9,1.2,)",
    "rq_gaussexp": "SumKernel(RationalQuadraticKernel(1.1,0.6,1.5,),GaussianExpKernel(-0.3,0.1,))",
    "product": "ProductKernel(GaussianKernel(1.5,1,),PeriodicKernel(1,1.3,0.9,))",
}


def loo_from_matrices(Kn, Y, dK=None):
    """(value, mu, s2, grad) from Kn = K + sigma^2 I (n x n), the labels Y (n x m) and, for the
    gradient (m = 1), the stacked derivative matrices dK (P x n x n); grad is None without them."""
    Kn = np.asarray(Kn, np.float64)
    Y = np.asarray(Y, np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    C = np.linalg.inv(Kn)
    C = 0.5 * (C + C.T)
    c = np.diag(C).copy()
    alpha = C @ Y
    mu = Y - alpha / c[:, None]
    s2 = 1.0 / c
    value = float(np.sum(-0.5 * np.log(s2)[:, None] - (Y - mu) ** 2 / (2 * s2[:, None]) - 0.5 * np.log(2 * np.pi)))
    grad = None
    if dK is not None:
        assert Y.shape[1] == 1, "the gradient is defined for one label column"
        al = alpha[:, 0]
        u = al / c
        a = C @ u
        w = (1.0 + al * al / c) / c
        H = (C * w[None, :]) @ C
        W = np.outer(a, al) - 0.5 * H
        grad = np.array([np.sum(D * W) for D in np.asarray(dK, np.float64)])
    return value, mu, s2, grad


def matrices(ks, X, grad=False):
    """(K, dK or None) of the tree `ks` on X: the oracle's kernel_matrix and deriv_matrix; trees
    with Matern leaves, which the oracle does not know, from tests/matern_ref.py."""
    X = np.asarray(X, np.float64)
    ks = ks if isinstance(ks, str) else ks.to_string()
    if "Matern" in ks:
        from tests import matern_ref as MR
        return MR.kmat(ks, X), (MR.dmat(ks, X) if grad else None)
    return O.kernel_matrix(ks, X), (O.deriv_matrix(ks, X) if grad else None)


def loo(ks, X, Y, sigma, grad=False):
    """The restatement on the kernel and derivative matrices of the tree `ks`."""
    K, dK = matrices(ks, X, grad)
    return loo_from_matrices(K + sigma * sigma * np.eye(K.shape[0]), Y, dK)


def brute_force(Kn, Y):
    """(mu, s2) by refitting without each sample in turn and predicting it (the noise included in
    the predictive variance, as in the closed form)."""
    Kn = np.asarray(Kn, np.float64)
    Y = np.asarray(Y, np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    n = Kn.shape[0]
    mu = np.empty_like(Y)
    s2 = np.empty(n)
    for i in range(n):
        keep = np.r_[0:i, i + 1:n]
        sol = np.linalg.solve(Kn[np.ix_(keep, keep)], np.c_[Y[keep], Kn[keep, i]])
        mu[i] = Kn[i, keep] @ sol[:, :-1]
        s2[i] = Kn[i, i] - Kn[i, keep] @ sol[:, -1]
    return mu, s2


def gpu_observations(ctx, names, n=777, d=5, sigma=0.7):
    """What the GPU returns for the f64 value + gradient cases, by name: for every tree in `names`
    a model fitted on make_data(n, d), its values alone (diag(C) from V) and its values with the
    gradient; for the Gaussian tree also the small shapes, fitted by the call.  Two processes that
    run this must agree bit for bit."""
    import gpr_amd
    from gpr_amd.synth import make_data
    out = {}

    def record(key, got):
        out[key + ".value"] = np.float64(got[0])
        out[key + ".mean"], out[key + ".var"] = got[1], got[2]
        if got[3] is not None:
            out[key + ".grad"] = got[3]

    def run(key, ks, n, d, fit):
        X, Y = make_data(n, d, 1)
        M = gpr_amd.Model(ctx, np.float64)
        M.set_data(X, Y)
        M.set_kernel(ks)
        M.set_noise(sigma)
        if fit:
            M.fit()
            record(key + ".values", M.loo())
        record(key, M.loo(grad=True))
        M.close()

    for name in names:
        run(name, GRAD_TREES[name], n, d, True)
        if name == "gauss":
            for ns in (100, 128, 129):
                run(f"gauss{ns}", GAUSS, ns, 3, False)
    return out
