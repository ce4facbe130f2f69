"""numpy restatement of the factor update behind gprx_model_remove (k_remove.hip), shared by
tests/test_remove_cpu.py and tests/test_gpu_remove.py.

Removing rows [f, f + r) of n samples: with the old factor partitioned at f and f + r,
L = [L11 0 0; L21 L22 0; L31 L32 L33], the reduced matrix has the factor [L11 0; L31 L33'] with
L33' L33'^T = L33 L33^T + L32 L32^T.  In the new coordinates L' L'^T = L L^T + X X^T with
X = [0; L32], eliminated by Givens rotations in the kernel's order: passes of `width` vectors,
then column block, column, vector; the rows below a column are independent (vectorised here)."""
import numpy as np

DB = 128
WIDTH = 16  # vectors one launch carries (gprx_dev_factor_update_width)


def update_factor(L, X, width=WIDTH, first_col=0, ncols=None):
    """L' (same dtype as L) with L' L'^T = L L^T + X X^T, columns first_col .. ncols - 1 swept."""
    L = np.array(L, copy=True)
    T = L.dtype.type
    n = L.shape[0]
    ncols = n if ncols is None else ncols
    X = np.asarray(X, dtype=L.dtype).reshape(n, -1)
    for v0 in range(0, X.shape[1], width):
        Xp = np.array(X[:, v0:v0 + width], copy=True)
        for b in range(first_col // DB, -(-ncols // DB)):
            for j in range(b * DB, min((b + 1) * DB, ncols)):
                for v in range(Xp.shape[1]):
                    a, x = L[j, j], Xp[j, v]
                    ss = a * a + x * x
                    ri = T(1) / np.sqrt(ss)  # the kernel's one reciprocal square root
                    rho = ss * ri
                    c, s = a * ri, x * ri
                    col, xv = L[j + 1:, j], Xp[j + 1:, v]
                    t = c * col + s * xv
                    Xp[j + 1:, v] = c * xv - s * col
                    L[j + 1:, j] = t
                    L[j, j] = rho
    return L


def reduced_problem(L, f, r):
    """(L0, X, n1): the old factor (n x n) without rows and columns [f, f + r), identity-padded to a
    multiple of 128, and X = [0; L32] padded with zero rows; n1 = n - r live rows."""
    n = L.shape[0]
    n1 = n - r
    keep = np.r_[0:f, f + r:n]
    npad = -(-n1 // DB) * DB
    L0 = np.eye(npad, dtype=L.dtype)
    L0[:n1, :n1] = L[np.ix_(keep, keep)]
    X = np.zeros((npad, r), dtype=L.dtype)
    X[f:n1] = L[f + r:, f:f + r]
    return L0, X, n1


def remove_factor(L, f, r, width=WIDTH):
    """The padded factor of the reduced matrix from the factor L of the full one, as
    model_remove does it: columns from block f // 128 on are swept, up to the live rows."""
    L0, X, n1 = reduced_problem(L, f, r)
    return update_factor(L0, X, width, first_col=f // DB * DB, ncols=n1), n1


REUSE_KS = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"


def reuse_observations(make_model, reused):
    """What a model answers after fit(300, m = 2), append(5), remove(40, 3), per dtype.  reused: the
    model went through other shapes first (fit at 640 / m = 3, then the steps above); else it is a
    fresh twin given only the last fit, the append and the remove.  Arrays by name."""
    from tests.helpers import make_data, make_queries
    out = {}
    for dtype in (np.float64, np.float32):
        M = make_model(dtype)
        M.set_kernel(REUSE_KS)
        M.set_noise(0.5)
        if reused:
            X, Y = make_data(640, 3, 3)
            M.set_data(X.astype(dtype), Y.astype(dtype))
            M.fit()
        X, Y = make_data(305, 3, 2)
        M.set_data(X[:300].astype(dtype), Y[:300].astype(dtype))
        M.fit()
        M.append(X[300:].astype(dtype), Y[300:].astype(dtype))
        info = M.remove(40, 3)
        tag = np.dtype(dtype).name
        out[tag + ".alpha"] = M.alpha()
        out[tag + ".info"] = np.array([info.logdet, info.datafit, info.info, info.method, info.refine_delta,
                                       info.refine_steps, info.appended], dtype=np.float64)
        Xq = make_queries(61, 3).astype(dtype)
        out[tag + ".predict61"] = M.predict(Xq)
        out[tag + ".predict1"] = M.predict(Xq[:1])
        out[tag + ".cov"] = M.posterior_cov(Xq[:40], Xq[:40][::-1].copy())
        M.close()
    return out


def backward_error(Lnew, target):
    """||L' L'^T - target||_max / ||target||_max, in double."""
    Ld = np.tril(np.asarray(Lnew, dtype=np.float64))
    return float(np.max(np.abs(Ld @ Ld.T - target)) / np.max(np.abs(target)))
