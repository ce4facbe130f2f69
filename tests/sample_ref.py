"""numpy restatement of the joint posterior and of posterior sampling (gprx_model_posterior,
gprx_model_sample, k_sample.hip), shared by tests/test_sample_cpu.py and tests/test_gpu_sample.py.

The normal generator, exactly as the device computes it: Philox4x32-10 (Salmon et al., SC'11;
Random123's constants and round order) with key (seed low, seed high); the normals e = 2c and
2c + 1 come from counter block (c low, c high, 0, 0): with the output words w0..w3,

    u1 = (((w0 | w1 << 32) >> 11) + 0.5) 2^-53,   u2 likewise from w2, w3,
    r  = sqrt(-2 ln u1),   z[2c] = r cos(2 pi u2),   z[2c + 1] = r sin(2 pi u2).

The posterior of a model with samples X, labels Y and noise sigma at the points Xq:

    mean = K(Xq, X) (K + sigma^2 I)^{-1} Y,   Sigma = K(Xq, Xq) - R R^T,   R = K(Xq, X) L^{-T},

and a draw i, label column c: mean[:, c] + Lq z[i, c, :], Lq Lq^T = Sigma + j I.
"""
import numpy as np

from tests import loo_ref as L

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """The ten rounds on arrays of counters: ctr (..., 4) and key (..., 2) of 32-bit words (any
    integer type) -> (..., 4) uint32."""
    c = [np.asarray(ctr)[..., k].astype(np.uint64) & MASK for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) & MASK for k in range(2))
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # (32 x 32 bits: exact in 64)
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def normals(seed, count):
    """The first `count` numbers of the stream `seed`, float64."""
    seed = int(seed) & (2 ** 64 - 1)
    nblk = (int(count) + 1) // 2
    c = np.arange(nblk, dtype=np.uint64)
    ctr = np.stack([c & MASK, c >> S32, np.zeros_like(c), np.zeros_like(c)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64), (nblk, 2))
    w = philox4x32_10(ctr, key).astype(np.uint64)

    def unit(lo, hi):
        return (((lo | (hi << S32)) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53

    r = np.sqrt(-2.0 * np.log(unit(w[:, 0], w[:, 1])))
    a = 2.0 * np.pi * unit(w[:, 2], w[:, 3])
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=-1).reshape(-1)[:int(count)]


def posterior(ks, X, Y, Xq, sigma, noise=False):
    """(mean q x m, Sigma q x q) of the tree `ks`: the kernel matrix of the stacked points [X; Xq]
    (tests/loo_ref.matrices: the oracle, or the Matern restatement), sliced."""
    X, Xq = np.asarray(X, np.float64), np.asarray(Xq, np.float64)
    Y = np.asarray(Y, np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    n = X.shape[0]
    Kall, _ = L.matrices(ks, np.concatenate([X, Xq]))
    K, Kqx, Kqq = Kall[:n, :n], Kall[n:, :n], Kall[n:, n:]
    Lf = np.linalg.cholesky(K + sigma * sigma * np.eye(n))
    R = np.linalg.solve(Lf, Kqx.T).T  # (a general solve of a triangular matrix: exact enough here)
    mean = R @ np.linalg.solve(Lf, Y)
    Sigma = Kqq - R @ R.T
    Sigma = 0.5 * (Sigma + Sigma.T)
    if noise:
        Sigma = Sigma + sigma * sigma * np.eye(Xq.shape[0])
    return mean, Sigma


def posterior_brute(K, Kqx, Kqq, Y, sigma):
    """The same from the explicit inverse."""
    C = np.linalg.inv(K + sigma * sigma * np.eye(K.shape[0]))
    return Kqx @ C @ Y, Kqq - Kqx @ C @ Kqx.T


def sample(mean, Sigma, j, Z):
    """Draws (n x q x m) from N(mean, Sigma + j I) with the normals Z (n x m x q)."""
    q = Sigma.shape[0]
    Lq = np.linalg.cholesky(Sigma + j * np.eye(q))
    return mean[None, :, :] + np.einsum("pr,icr->ipc", Lq, np.asarray(Z, np.float64))
