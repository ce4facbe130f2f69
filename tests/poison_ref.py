"""The cases of tests/test_gpu_poison.py: library paths that no lifecycle scenario reaches, each run
once under GPRX_POISON=1 (a child process: every fresh device allocation holds bytes 0x41) and once
without, bit for bit.

The model's buffers are grow-only and padded to 128, the context-level entry points allocate their
own per call, the chained and persistent launches keep counter and flag words in context-owned
scratch, and a few partial sums live in stream-ordered allocations.  A kernel that reads a row, a
tile or a word nothing has written gets zeros from a fresh allocation on most days and whatever was
there before on the others; 0x41 makes every day one of the others.

Shapes: the smallest ragged ones with padding in every dimension -- n in {129, 300} (one row past a
tile; two tiles and a ragged third), d in {3, 33} (below and one past the 32-wide feature group),
m in {1, 3} label columns, q in {1, 61} queries.  Nothing here is compared with an oracle: the
suite's parity tests do that; a case is a name and a function returning named arrays.
"""
import numpy as np

from tests.helpers import make_data, make_queries
from tests.lifecycle_ref import C3, G, HostGauss

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
SHAPES = [(129, 3, 1, 1), (300, 33, 3, 61)]  # (n, d, m, q)
SIGMA = 0.5
SEED, DRAWS = 20240607, 3
SPARSE_N = 500
SPARSE = [(40, 3), (130, 33)]  # (inducing points, d): below a tile, and one tile and a ragged second
VIRTUAL = (2, 3)


def _scalars(*v):
    return np.asarray(v, np.float64)


def _spd(n, d, dtype):
    """A well-conditioned SPD matrix of order n in `dtype` (a Gaussian kernel matrix + I / 4)."""
    X, _ = make_data(n, d)
    return (HostGauss(0.7, 1.3)(X, X) + 0.25 * np.eye(n)).astype(dtype)


def _padded_factor(n, d, dtype):
    """The lower Cholesky factor of _spd, identity-padded to the next multiple of 128."""
    npad = -(-n // 128) * 128
    A = np.eye(npad)
    A[:n, :n] = _spd(n, d, F64)
    return np.linalg.cholesky(A).astype(dtype)


# ---------------------------------------------------------------------------------------
# context-level entry points
# ---------------------------------------------------------------------------------------
def case_matrices(ctx, vctx):
    out = {}
    for dt in (F64, F32):
        for n, d, _, _ in SHAPES:
            X, _ = make_data(n, d, dtype=dt)
            out[f"kernel_matrix/{n}x{d}/{dt.name}"] = ctx.kernel_matrix(C3, X, dt)
            out[f"deriv_matrix/{n}x{d}/{dt.name}"] = ctx.deriv_matrix(C3, X, dt)
        for d in (3, 33):
            A, _ = make_data(70, d, dtype=dt)
            B = make_queries(45, d, dtype=dt)
            out[f"cross_matrix/70x45x{d}/{dt.name}"] = ctx.cross_matrix(C3, A, B, dt)
    return out


def case_build_matrix(ctx, vctx):
    out = {}
    for dt in (F64, F32):
        for n, d, _, _ in SHAPES:
            X, _ = make_data(n, d, dtype=dt)
            for path in (0, 1):
                out[f"build_matrix/path{path}/{n}x{d}/{dt.name}"] = ctx.build_matrix(C3, X, SIGMA, path, dt)
    return out


def case_cholesky(ctx, vctx):
    out = {}
    for dt in (F64, F32):
        A = _spd(300, 3, dt)
        Lf, info = ctx.cholesky(A)
        out[f"cholesky/300/{dt.name}"] = Lf
        out[f"cholesky/300/{dt.name}/info"] = _scalars(info)
        out[f"spd_inverse/300/{dt.name}"] = ctx.spd_inverse(A)
    return out


def case_panel_and_update(ctx, vctx):
    out = {}
    for dt in (F64, F32):
        Lp = _padded_factor(300, 3, dt)  # 384 x 384
        for rows in (1, 3, 61):
            R = make_queries(rows, Lp.shape[0], dtype=dt)
            for gemm in (False, True):
                out[f"forward_panel/{rows}/{'gemm' if gemm else 'chain'}/{dt.name}"] = ctx.forward_panel(Lp, R, gemm)
        for r in (1, 3):
            Xu = 0.1 * make_queries(Lp.shape[0], r, dtype=dt)
            Lo, Li = ctx.factor_update(Lp, Xu)
            out[f"factor_update/{r}/L/{dt.name}"] = Lo
            out[f"factor_update/{r}/Linv/{dt.name}"] = Li
    return out


def case_normals(ctx, vctx):
    return {f"normals/{count}/{dt.name}": ctx.normals(SEED, count, dt)
            for dt in (F64, F32) for count in (1, DRAWS * 61 * 3)}


# ---------------------------------------------------------------------------------------
# the joint posterior and sampling, after an append and after a remove
# ---------------------------------------------------------------------------------------
def case_posterior_and_sample(ctx, vctx):
    import gpr_amd
    out = {}
    for dt in (F64, F32):
        for n, d, m, q in SHAPES:
            X, Y = make_data(n + 1, d, m, dtype=dt)
            Xq = make_queries(q, d, dtype=dt)
            M = gpr_amd.Model(ctx, dt)
            M.set_data(X[:n], Y[:n])
            M.set_kernel(C3)
            M.set_noise(SIGMA)
            M.fit()
            for state, change in (("append1", lambda: M.append(X[n:], Y[n:])), ("remove0", lambda: M.remove(0, 1))):
                change()
                tag = f"{state}/{n}x{d}x{m}/q{q}/{dt.name}"
                out[f"posterior/{tag}/mean"], out[f"posterior/{tag}/cov"] = M.posterior(Xq)
                s, jit = M.sample(Xq, n=DRAWS, seed=SEED)
                out[f"sample/{tag}/draws"], out[f"sample/{tag}/jitter"] = s, _scalars(jit)
            M.close()
    return out


# ---------------------------------------------------------------------------------------
# the sparse fit and its likelihood
# ---------------------------------------------------------------------------------------
def case_sparse(ctx, vctx):
    out = {}
    for Mi, d in SPARSE:
        X, Y = make_data(SPARSE_N, d, 3)
        Xm = X[:: SPARSE_N // Mi][:Mi].copy()
        tag = f"{SPARSE_N}x{d}/M{Mi}"
        for k, v in zip(("Kinv", "RV", "RM"), ctx.sparse_fit(G, X, Y, Xm, 0.3, 1e-4)):
            out[f"sparse_fit/{tag}/{k}"] = v
        v, g, ld = ctx.sparse_lml(G, X, Y[:, :1].copy(), Xm, 0.3, 1e-4, grad=True)
        out[f"sparse_lml/{tag}/value_logdet"], out[f"sparse_lml/{tag}/grad"] = _scalars(v, ld), np.asarray(g)
    return out


def case_sparse_reuse(ctx, vctx):
    """The sparse state reused: fewer inducing points on the same padded layout and back (MFMA and
    VALU builds, below one tile), label rows <-> the fused K Y (tests/sparse_reuse_ref.py)."""
    from tests import sparse_reuse_ref as R
    return {f"sparse_reuse/{k}": v
            for k, v in R.collect(ctx, ("shrink_g", "shrink_gw", "shrink_small", "labels")).items()}


# ---------------------------------------------------------------------------------------
# leave-one-out in fp32 (the f64 cases run poisoned in test_gpu_loo.py)
# ---------------------------------------------------------------------------------------
def case_loo_f32(ctx, vctx):
    import gpr_amd
    out = {}
    for n, d, _, _ in SHAPES:
        X, Y = make_data(n, d, 1, dtype=F32)
        M = gpr_amd.Model(ctx, F32)
        M.set_data(X, Y)
        M.set_kernel(C3)
        M.set_noise(SIGMA)
        M.fit()
        v, mean, var, g = M.loo(grad=True)
        tag = f"loo/{n}x{d}/float32"
        out[f"{tag}/value"], out[f"{tag}/mean"], out[f"{tag}/var"], out[f"{tag}/grad"] = _scalars(v), mean, var, g
        M.close()
    return out


# ---------------------------------------------------------------------------------------
# the sharded engine: posterior covariance (variances and pairs) and the LML gradient
# ---------------------------------------------------------------------------------------
def case_sharded(ctx, vctx):
    import gpr_amd
    out = {}
    for g in VIRTUAL:
        for n, d, _, q in SHAPES:
            X, Y = make_data(n, d, 1)
            Xa = make_queries(q, d)
            Xb = Xa[::-1].copy() if q > 1 else make_queries(2, d)[1:]
            M = gpr_amd.Model(vctx[g], F64)
            M.set_data(X, Y)
            M.set_kernel(C3)
            M.set_noise(SIGMA)
            M.fit()
            tag = f"virtual{g}/{n}x{d}/q{q}"
            out[f"{tag}/fit/var"] = M.posterior_cov(Xa, Xa)
            out[f"{tag}/fit/pairs"] = M.posterior_cov(Xa, Xb)
            v, gr, ld = M.lml(grad=True, distributed=True)
            out[f"{tag}/lml/value_logdet"], out[f"{tag}/lml/grad"] = _scalars(v, ld), np.asarray(gr)
            out[f"{tag}/lml/var"] = M.posterior_cov(Xa, Xa)  # (from the LML-mode factor: its own layout)
            out[f"{tag}/lml/pairs"] = M.posterior_cov(Xa, Xb)
            M.close()
    return out


CASES = {
    "matrices": case_matrices,
    "build_matrix": case_build_matrix,
    "cholesky": case_cholesky,
    "panel_and_update": case_panel_and_update,
    "normals": case_normals,
    "posterior_and_sample": case_posterior_and_sample,
    "sparse": case_sparse,
    "sparse_reuse": case_sparse_reuse,
    "loo_f32": case_loo_f32,
    "sharded": case_sharded,
}
SHARDED = ("sharded",)                                    # need vctx
PLAIN = tuple(k for k in CASES if k not in SHARDED)       # need ctx


def collect(ctx, vctx, names=None):
    """{"<case>:<read>": array} of the named cases (default: all).  ctx: a one-GPU context (the
    PLAIN cases); vctx: {g: a context of g virtual ranks} for g in VIRTUAL (the SHARDED cases)."""
    out = {}
    for name in (CASES if names is None else names):
        got = CASES[name](ctx, vctx)
        assert got and not set(got) & set(out), name
        out.update({k: np.asarray(v) for k, v in got.items()})
    return out


def is_poisoned(ctx):
    """A fresh DeviceArray reads back as bytes 0x41: the library's allocations are poisoned."""
    import gpr_amd
    a = gpr_amd.DeviceArray.empty(ctx, (4,))
    raw = a.numpy().view(np.uint8)
    a.free()
    return bool(np.all(raw == 0x41))
