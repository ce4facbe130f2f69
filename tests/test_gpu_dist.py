"""The storage-sharded multi-GPU fit (gprx_dist.cpp + potrf_tiles_kernel<T, true> + k_dsolve.hip)
on one GPU.

gprx_ctx_create_virtual runs g VIRTUAL ranks in this process: each keeps only the lower tiles of
its row blocks, runs its own persistent tile launch on a share of the CUs, and receives the
other ranks' tiles through its bounded window and the diagonal inverses into its Linv array --
pushed by the producing tasks themselves (device stores + flags, no host in the loop), exactly
as the ranks of a node push into each other's IPC-mapped mailboxes.  The back substitution,
the fp32 refinement's solves and the LML's inverse (C = U U^T riding along) are sharded too.
gprx_ctx_create_peer runs the same engine across PROCESSES (two processes sharing the GPU, IPC
mappings, a gloo all-gather for the bootstrap): test_peer_two_processes."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import make_data, make_queries, relerr, TOL

pytestmark = pytest.mark.gpu

C3K = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"
RQK = "RationalQuadraticKernel(1.1,0.6,1.5,)"


def _fit(ctx, ks, X, Y, sigma, dtype, flags=0):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X, Y)
    M.set_kernel(ks)
    M.set_noise(sigma)
    info = M.fit(flags)
    return M, info


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("ks", [C3K, RQK])
@pytest.mark.parametrize("n,m", [(700, 1), (1500, 3)])
def test_virtual_ranks_f64(g, ks, n, m):
    import gpr_amd
    d, sigma = 5, 0.5
    X, Y = make_data(n, d, m)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, ks, X, Y, sigma, np.float64)
        a_ref, _ = O.fit(ks, X, Y, sigma, want_core=False)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        Xq = make_queries(50, d)
        assert relerr(M.predict(Xq), O.predict(ks, X, a_ref, Xq)) <= 1e-6
        K = O.kernel_matrix(ks, X) + sigma * sigma * np.eye(n)
        assert abs(info.logdet - np.linalg.slogdet(K)[1]) <= 1e-9 * max(1.0, abs(info.logdet))
        df_ref = float(np.sum(Y.reshape(n, m) * a_ref.reshape(n, m)))  # trace(Y^T K^-1 Y) = z^T z
        assert abs(info.datafit - df_ref) <= 1e-8 * abs(df_ref)
        M.close()
    finally:
        vctx.close()


@pytest.mark.parametrize("g,gb", [(2, 3), (3, 2)])
def test_virtual_ranks_grouped(g, gb, monkeypatch):
    """Row blocks dealt in groups of gb consecutive blocks (GPRX_DIST_GROUP forces the group
    size the simulated makespan otherwise picks): ownership, local storage, send slots and the
    remote-input checks all follow the ownership table."""
    import gpr_amd
    monkeypatch.setenv("GPRX_DIST_GROUP", str(gb))
    n, d, m, sigma = 1700, 4, 2, 0.5
    X, Y = make_data(n, d, m)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, C3K, X, Y, sigma, np.float64)
        a_ref, _ = O.fit(C3K, X, Y, sigma, want_core=False)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        K = O.kernel_matrix(C3K, X) + sigma * sigma * np.eye(n)
        assert abs(info.logdet - np.linalg.slogdet(K)[1]) <= 1e-9 * max(1.0, abs(info.logdet))
        M.close()
    finally:
        vctx.close()


@pytest.mark.parametrize("g", [2, 4])
def test_virtual_ranks_f32(g):
    import gpr_amd
    n, d, sigma = 1100, 4, 0.6
    X, Y = make_data(n, d, 1)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, _ = _fit(vctx, C3K, X32, Y32, sigma, np.float32)
        a_ref, _ = O.fit(C3K, X32, Y32, sigma, np.float32, want_core=False)
        assert relerr(M.alpha(), a_ref) <= 1e-3
        M.close()
    finally:
        vctx.close()


def test_virtual_ranks_repeat_and_lml_value():
    """Several fits on one engine (counters, flags and receive buffers reset per fit), the
    LML value from the distributed factor, and a factor-based call after them."""
    import gpr_amd
    n, d, sigma = 900, 3, 0.4
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        M, _ = _fit(vctx, C3K, X, Y, sigma, np.float64)
        a1 = M.alpha()
        M.fit()
        assert np.array_equal(a1, M.alpha())  # fixed schedules and summation orders: bit-identical
        v, _, logdet = M.lml(grad=False)
        vr, _, _, ldr = O.lml(C3K, X, Y, sigma, with_grad=False)
        assert abs(logdet - ldr) <= 1e-9 * abs(ldr)
        # the exact value from its pieces (include/Likelihood.h:166-202) ...
        a_ref, _ = O.fit(C3K, X, Y, sigma, want_core=False)
        v_exact = -0.5 * float(Y.reshape(-1) @ a_ref.reshape(-1)) - 0.5 * ldr - n / 2 * np.log(2 * np.pi)
        assert abs(v - v_exact) <= 1e-8 * abs(v_exact)
        # ... and the reference's value, whose determinant underflows double here (clamped)
        vc, _, _ = M.lml(grad=False, compat=True)
        assert abs(vc - vr) <= 1e-6 * abs(vr)
        # the factor-based calls assemble the tiles (test_virtual_ranks_posterior_and_core):
        # at the training points the posterior variance is at most the noise-free prior
        pv = M.posterior_cov(X[:3], X[:3])
        assert np.all(np.isfinite(pv)) and np.all(pv >= -1e-10)
        M.close()
    finally:
        vctx.close()


def test_virtual_ranks_c3_shape():
    """A C3-shaped fit (N = 4096, d = 32) over 2 virtual ranks against the single-GPU fit."""
    import gpr_amd
    n, d, sigma = 4096, 32, 1.0
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=2)
    sctx = gpr_amd.Context(0)
    try:
        Md, infod = _fit(vctx, C3K, X, Y, sigma, np.float64)
        Ms, infos = _fit(sctx, C3K, X, Y, sigma, np.float64)
        assert relerr(Md.alpha(), Ms.alpha()) <= 1e-10
        assert abs(infod.logdet - infos.logdet) <= 1e-10 * abs(infos.logdet)
        print(f"virtual 2 ranks N=4096: {infod.ms_factor:.2f} ms wall")
        Md.close()
        Ms.close()
    finally:
        vctx.close()
        sctx.close()


INDEF = "RationalQuadraticKernel(1.2,2,-1,)"  # K + s^2 I indefinite (tests/test_gpu_lu.py)


@pytest.mark.parametrize("g", [2, 3])
def test_virtual_ranks_lu_fallback(g):
    """An indefinite K on a distributed context: the sharded Cholesky meets a non-positive
    pivot and every rank refactors with the partial-pivot LU in double, as the reference's
    default inversion does (lib/GaussianProcess.cpp:545-559) -- the same fit that succeeds on
    one GPU succeeds here, with the same alpha, predictions and LML gradient."""
    import gpr_amd
    n, d, m, sigma = 700, 3, 2, 0.3
    X, Y = make_data(n, d, m)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, INDEF, X, Y, sigma, np.float64)
        assert info.method == 1 and info.info > 0
        a_ref, C_ref = O.fit(INDEF, X, Y, sigma)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        Xq = make_queries(40, d)
        assert relerr(M.predict(Xq), O.predict(INDEF, X, a_ref, Xq)) <= 1e-6
        assert relerr(M.core_matrix(), C_ref) <= 1e-6
        with pytest.raises(gpr_amd.GprxError) as e:
            M.fit(gpr_amd.gprx.FIT_NO_LU_FALLBACK)
        assert e.value.status == 2
        M.close()
        Y1 = Y[:, :1].copy()
        M = gpr_amd.Model(vctx, np.float64)
        M.set_data(X, Y1)
        M.set_kernel(INDEF)
        M.set_noise(sigma)
        v, grad, logdet = M.lml(grad=True)
        vr, gr, _, ldr = O.lml(INDEF, X, Y1, sigma)
        assert relerr(grad, gr) <= 1e-6
        M.close()
    finally:
        vctx.close()


def test_virtual_ranks_force_lu():
    """GPRX_FIT_FORCE_LU (the SVD inversion methods) on a distributed context: the LU on every
    rank, never a Cholesky that could reject the matrix."""
    import gpr_amd
    n, d, sigma = 500, 3, 0.5
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        M, info = _fit(vctx, C3K, X, Y, sigma, np.float64, flags=gpr_amd.gprx.FIT_FORCE_LU)
        assert info.method == 1
        a_ref, _ = O.fit(C3K, X, Y, sigma, want_core=False)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        M.close()
    finally:
        vctx.close()


def test_virtual_ranks_not_spd_and_nonfinite():
    import gpr_amd
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        X, Y = make_data(600, 3, 1)
        M, _ = _fit(vctx, C3K, X, Y, 0.5, np.float64)
        M.set_kernel(INDEF)
        M.set_noise(0.3)
        with pytest.raises(gpr_amd.GprxError) as e:
            M.fit(gpr_amd.gprx.FIT_NO_LU_FALLBACK)
        assert e.value.status == 2
        X[100, 1] = np.nan
        M.set_data(X, Y)
        M.set_kernel(C3K)
        with pytest.raises(gpr_amd.GprxError) as e:
            M.fit()
        assert "not finite" in str(e.value)
        M.close()
    finally:
        vctx.close()


PRODK = "ProductKernel(GaussianKernel(1.2,0.8,),RationalQuadraticKernel(1,0.7,2,))"


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("ks", [C3K, RQK, PRODK])
def test_virtual_ranks_lml_grad(g, ks):
    """LML value + gradient on a distributed context (row-block partials of the gradient
    summed over the ranks; C from the factor assembled from the tiles) vs the oracle."""
    import gpr_amd
    n, d, sigma = 900, 3, 0.4
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M = gpr_amd.Model(vctx, np.float64)
        M.set_data(X, Y)
        M.set_kernel(ks)
        M.set_noise(sigma)
        v, grad, logdet = M.lml(grad=True)
        vr, gr, _, ldr = O.lml(ks, X, Y, sigma)
        assert abs(logdet - ldr) <= 1e-9 * abs(ldr)
        assert relerr(grad, gr) <= 1e-6
        vc, _, _ = M.lml(grad=False, compat=True)
        assert abs(vc - vr) <= 1e-6 * max(1.0, abs(vr))
        M.close()
    finally:
        vctx.close()


def test_rccl_one_rank_lml_grad():
    """The same on a one-rank RCCL communicator (GPRX_LML_DISTRIBUTED): the all-reduce of the
    gradient partials runs through RCCL."""
    import gpr_amd
    n, d, sigma = 700, 4, 0.5
    X, Y = make_data(n, d, 1)
    dctx = gpr_amd.Context(0, dist=(0, 1, gpr_amd.unique_id()))
    try:
        M = gpr_amd.Model(dctx, np.float64)
        M.set_data(X, Y)
        M.set_kernel(C3K)
        M.set_noise(sigma)
        v, grad, logdet = M.lml(grad=True, distributed=True)
        vr, gr, _, ldr = O.lml(C3K, X, Y, sigma)
        assert abs(logdet - ldr) <= 1e-9 * abs(ldr)
        assert relerr(grad, gr) <= 1e-6
        M.close()
    finally:
        dctx.close()


@pytest.mark.parametrize("g", [2, 3])
def test_virtual_ranks_posterior_and_core(g):
    """operator()(x,y) / GetCredibleInterval (lib/GaussianProcess.cpp:84-114) and the core
    matrix (:513-528) on a distributed fit: the factor every rank holds as tiles (its own and the
    received ones) is assembled once into a dense factor, then the single-GPU solves run."""
    import gpr_amd
    n, d, sigma = 900, 4, 0.5
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, _ = _fit(vctx, C3K, X, Y, sigma, np.float64)
        _, C_ref = O.fit(C3K, X, Y, sigma)
        Xa, Xb = make_queries(40, d), make_queries(40, d)[::-1].copy()
        assert relerr(M.posterior_cov(Xa, Xb), O.posterior_cov(C3K, X, C_ref, Xa, Xb)) <= 1e-6
        var = M.posterior_cov(Xa, Xa)
        assert relerr(var, O.posterior_cov(C3K, X, C_ref, Xa, Xa)) <= 1e-6
        assert relerr(M.core_matrix(), C_ref) <= 1e-6
        M.fit()  # a refit drops the assembled factor; the next call assembles the new one
        assert relerr(M.posterior_cov(Xa, Xa), var) <= 1e-12
        M.close()
    finally:
        vctx.close()


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_virtual_ranks_posterior_sharded(g, dtype):
    """The posterior covariance on a sharded fit without the dense factor: the queries' forward
    substitution runs across the ranks (dist_pvar_kernel: each rank's own rows of L, the query
    columns V_k pushed through the receive windows, the row sums all-reduced).  Variances and
    pairs (x != y) against the oracle; more queries than one solve takes (several batches); the
    model must not have gathered the N x N factor, and no rank may hold more than its rows."""
    import gpr_amd
    n, d, sigma = 1400, 4, 0.5
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, _ = _fit(vctx, C3K, X.astype(dtype), Y.astype(dtype), sigma, dtype)
        info = M.dist_info()
        assert info["posterior_chunks"] >= 1
        Xd = X.astype(dtype).astype(np.float64)
        _, C_ref = O.fit(C3K, Xd, Y.astype(dtype).astype(np.float64), sigma)
        qn = info["posterior_chunks"] * 128 + 77  # more than one batch of variances
        Xa = make_queries(qn, d).astype(dtype).astype(np.float64)
        Xb = Xa[::-1].copy()
        tol = TOL[np.dtype(dtype)]
        for xb in (Xa, Xb):
            c = M.posterior_cov(Xa.astype(dtype), xb.astype(dtype))
            ref = O.posterior_cov(C3K, Xd, C_ref, Xa, xb)
            kab = np.array([O.kernel_eval(C3K, a, b, with_grad=False) for a, b in zip(Xa, xb)])
            # a difference of O(1) terms: compared on the scale of k(x, y), as on one GPU
            assert np.max(np.abs(c - ref)) <= tol * max(1.0, np.max(np.abs(kab)))
        after = M.dist_info()
        assert after["dense_factor"] == 0
        assert after["bytes_storage"] <= n * n * np.dtype(dtype).itemsize / g * 1.3 + 40 * 128 * 128 * 8
        M.close()
    finally:
        vctx.close()


def test_virtual_ranks_posterior_growing_batch():
    """The sharded posterior solve with a query batch that grows and shrinks on one model: q = 40
    (one chunk of 128 columns), q = 128 + 77 (two chunks: every per-rank workspace of the solve
    grows), q = 40 again (the larger workspace reused).  The ranks' partial-sum buffers are sized
    before the first rank's launch: growing one between the launches frees the old buffer, which
    can block the host while the rank already launched waits, bounded, for tiles of a rank not
    yet launched.  Variances and pairs, each against the oracle at the tolerances of
    test_virtual_ranks_posterior_sharded and bit for bit against a fresh model on the same
    context that makes only that call.
    n = 257: posterior_chunks >= 2 (asserted; needed for a batch to grow within one solve) already
    holds at one row block, where rank 1 owns no matrix rows and nothing waits; at three row blocks
    (rank 0 owns blocks 0 and 2, rank 1 block 1) each rank waits for the other's tiles, which is
    the smallest shape at which the order of the launches matters."""
    import gpr_amd
    n, d, sigma = 257, 4, 0.5
    X, Y = make_data(n, d, 1)
    _, C_ref = O.fit(C3K, X, Y, sigma)
    tol = TOL[np.dtype(np.float64)]
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        M, _ = _fit(vctx, C3K, X, Y, sigma, np.float64)
        assert M.dist_info()["posterior_chunks"] >= 2
        for q in (40, 128 + 77, 40):
            Xa = make_queries(q, d)
            for xb in (Xa, Xa[::-1].copy()):
                c = M.posterior_cov(Xa, xb)
                ref = O.posterior_cov(C3K, X, C_ref, Xa, xb)
                kab = np.array([O.kernel_eval(C3K, a, b, with_grad=False) for a, b in zip(Xa, xb)])
                err = float(np.max(np.abs(c - ref)))
                print(f"growing batch q = {q}, {'variances' if xb is Xa else 'pairs'}: error {err:.2e}")
                assert err <= tol * max(1.0, np.max(np.abs(kab)))
                F, _ = _fit(vctx, C3K, X, Y, sigma, np.float64)
                fresh = F.posterior_cov(Xa, xb)
                F.close()
                assert np.array_equal(c, fresh), f"q = {q}: differs from a fresh model, relerr {relerr(c, fresh):.2e}"
        assert M.dist_info()["dense_factor"] == 0
        M.close()
    finally:
        vctx.close()


def test_virtual_ranks_small_window(monkeypatch):
    """A 2-panel window (GPRX_DIST_WINDOW) and single-panel update chunks over 3 ranks: every
    window slot is refilled many times, so the release protocol (a producer may overwrite slot
    p mod ww only after every consumer released panel p) is exercised on every panel."""
    import gpr_amd
    monkeypatch.setenv("GPRX_DIST_WINDOW", "2")
    n, d, m, sigma = 2000, 4, 2, 0.5
    X, Y = make_data(n, d, m)
    vctx = gpr_amd.Context(0, virtual=3)
    try:
        M, info = _fit(vctx, C3K, X, Y, sigma, np.float64)
        assert M.dist_info()["ww"] == 2
        a_ref, _ = O.fit(C3K, X, Y, sigma, want_core=False)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        M.close()
    finally:
        vctx.close()


@pytest.mark.parametrize("g,ww", [(6, 64), (8, 16), (5, 4)])
def test_virtual_ranks_window_slots_verified(g, ww, monkeypatch, capfd):
    """GPRX_DIST_CHECK: every window read is verified against a tag the producer wrote with the
    tile (this fit's epoch and the panel) before and after the read -- a slot refilled before
    its consumers released it shows up as a stale or overwritten read.  Repeated fits at C3
    size with windows smaller than the matrix (every slot reused), 5-8 ranks."""
    import gpr_amd
    monkeypatch.setenv("GPRX_DIST_CHECK", "1")
    monkeypatch.setenv("GPRX_DIST_WINDOW", str(ww))
    n, d, sigma = 16384 if g > 5 else 8192, 32, 1.0
    X, Y = make_data(n, d, 1)
    a_ref = _single_alpha(X, Y, sigma)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M = gpr_amd.Model(vctx, np.float64)
        M.set_data(X, Y)
        M.set_kernel(C3K)
        M.set_noise(sigma)
        for _ in range(3):
            M.fit()
            assert relerr(M.alpha(), a_ref) <= 1e-10
        assert M.dist_info()["ww"] == ww
        err = capfd.readouterr().err
        assert "stale window reads" not in err, err
        M.close()
    finally:
        vctx.close()


@pytest.mark.parametrize("g", [2, 5])
def test_virtual_ranks_written_through_pushes(g, monkeypatch, capfd):
    """The cross-device push flavour (GPRX_DIST_WT=1: 16-byte sc0 sc1 stores, no L2 write-back
    fence before the flag; the default for ranks on different GPUs) forced on virtual ranks, with
    every window read verified (GPRX_DIST_CHECK) and repeated fits bit-identical."""
    import gpr_amd
    monkeypatch.setenv("GPRX_DIST_WT", "1")
    monkeypatch.setenv("GPRX_DIST_CHECK", "1")
    monkeypatch.setenv("GPRX_DIST_WINDOW", "8")
    n, d, m, sigma = 4000, 8, 2, 0.5
    X, Y = make_data(n, d, m)
    a_ref, _ = O.fit(C3K, X, Y, sigma, want_core=False)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, C3K, X, Y, sigma, np.float64)
        a0 = M.alpha()
        assert relerr(a0, a_ref) <= 1e-6
        for _ in range(2):
            M.fit()
            assert np.array_equal(M.alpha(), a0)
        assert "stale window reads" not in capfd.readouterr().err
        M.close()
    finally:
        vctx.close()


@pytest.mark.parametrize("g", [2, 4])
def test_virtual_ranks_storage_is_sharded(g, monkeypatch):
    """Per-rank device memory of the sharded fit: the packed lower tiles of the rank's own row
    blocks (~N^2/(2g)), the window (ww panels of N x 128) and O(N x 128) of diagonal inverses,
    label tiles, flags and tables -- never the N^2 factor (the verdict's round-2 finding: 0.56
    N^2 per rank at g = 8).  C3-shaped, N = 8192."""
    import gpr_amd
    n, d, sigma = 8192, 32, 1.0
    # a window budget of 150 MiB: 16 panels of (nc + 1) tiles fit, 32 do not
    monkeypatch.setenv("GPRX_DIST_WINDOW_MB", "150")
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, C3K, X, Y, sigma, np.float64)
        di = M.dist_info()
        s, nb = 8, 128
        assert di["ww"] <= 16 and di["ww"] * (n // nb + 1) * nb * nb * s <= 150 * 2**20
        nc = n // nb
        # own row blocks (cyclic groups): at most ceil(nc / (g gb)) gb blocks, the worst-placed
        # rank's rows are the latest ones: bound its lower tiles by the last blocks of the matrix
        per_rank_blocks = -(-nc // (g * di["gb"])) * di["gb"]
        worst = sum(i + 1 for i in range(nc - per_rank_blocks, nc)) + nc  # + the label block
        assert di["bytes_storage"] <= worst * nb * nb * s
        assert di["bytes_storage"] <= 1.25 * (n * n / (2 * g)) * s + nc * nb * nb * s
        window = di["ww"] * (nc + 1) * nb * nb * s
        small = 16 * n * nb * s  # Linv, label tiles, alpha / z areas, partials, flags, tables
        assert di["bytes_rank"] <= di["bytes_storage"] + window + small
        assert di["bytes_rank"] < n * n * s / 2  # far below the dense lower factor
        a_ref = _single_alpha(X, Y, sigma)
        assert relerr(M.alpha(), a_ref) <= 1e-10
        print(f"g={g}: storage {di['bytes_storage'] / 2**20:.1f} MiB, rank total {di['bytes_rank'] / 2**20:.1f} MiB, "
              f"window {di['ww']} panels, chunk {di['chunk_w']}, gb {di['gb']}; dense lower factor "
              f"{n * n * s / 2 / 2**20:.1f} MiB")
        M.close()
    finally:
        vctx.close()


def _single_alpha(X, Y, sigma, ks=C3K, dtype=np.float64):
    import gpr_amd
    c = gpr_amd.Context(0)
    try:
        M, _ = _fit(c, ks, X, Y, sigma, dtype)
        a = M.alpha()
        M.close()
        return a
    finally:
        c.close()


C4K = "RationalQuadraticKernel(1,0.3,1,)"


@pytest.mark.parametrize("g", [1, 2])
def test_virtual_ranks_c4_fp32_refined(g):
    """BASELINE configs[3] at full size: N = 32768, d = 32, RationalQuadratic fp32 over the
    sharded fit, alpha refined in fp64 through the sharded forward / back substitutions (the
    reference inverts fp32 GPs in double, include/LAPACKUtils.h:85-97), against the fp64 fit of
    the same float data at 1e-5 (the BASELINE fp32 bar is 1e-3)."""
    import gpr_amd
    n, d, sigma = 32768, 32, 1.0
    X, Y = make_data(n, d, 1)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    a64 = _single_alpha(X32.astype(np.float64), Y32.astype(np.float64), float(np.float32(sigma)), C4K)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, C4K, X32, Y32, sigma, np.float32)
        err = relerr(M.alpha(), a64)
        print(f"C4 g={g}: refine steps {info.refine_steps}, delta {info.refine_delta:.2e}, "
              f"alpha vs fp64 {err:.2e}, factor {info.ms_factor:.1f} ms, refine {info.ms_refine:.1f} ms")
        assert info.refine_steps >= 1 and err <= 1e-5
        M.close()
    finally:
        vctx.close()


def test_rccl_one_rank_c4_fp32_refined():
    """The same refinement through GPRX_FIT_DISTRIBUTED on a one-rank RCCL communicator."""
    import gpr_amd
    n, d, sigma = 32768, 32, 1.0
    X, Y = make_data(n, d, 1)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    a64 = _single_alpha(X32.astype(np.float64), Y32.astype(np.float64), float(np.float32(sigma)), C4K)
    dctx = gpr_amd.Context(0, dist=(0, 1, gpr_amd.unique_id()))
    try:
        M, info = _fit(dctx, C4K, X32, Y32, sigma, np.float32, flags=gpr_amd.gprx.FIT_DISTRIBUTED)
        assert relerr(M.alpha(), a64) <= 1e-5
        M.close()
    finally:
        dctx.close()


@pytest.mark.parametrize("g", [2, 3])
def test_virtual_ranks_f32_vs_oracle_fp32(g):
    """fp32 over the sharded fit vs the oracle's fp32 path (the reference's cast-to-double LU,
    include/LAPACKUtils.h:85-97) at the BASELINE fp32 tolerance, and vs the double solve of the
    same float data at 1e-5 (the fp64 refinement reaches it)."""
    import gpr_amd
    n, d, sigma = 1500, 5, 0.6
    X, Y = make_data(n, d, 2)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, RQK, X32, Y32, sigma, np.float32)
        a = M.alpha()
        # the oracle's fp32 path: K in float, inverted in double, C Y in float (its own rounding
        # is ~1e-5 here): the BASELINE fp32 bar
        a_ref, _ = O.fit(RQK, X32, Y32, sigma, np.float32, want_core=False)
        assert relerr(a, a_ref) <= 1e-3
        # the refinement reaches the double solve of the same float data and float parameters
        # (the reference stores an fp32 GP's kernel parameters in float)
        rq32 = "RationalQuadraticKernel({},{},{},)".format(*[repr(float(np.float32(v))) for v in (1.1, 0.6, 1.5)])
        a64, _ = O.fit(rq32, X32.astype(np.float64), Y32.astype(np.float64), float(np.float32(sigma)),
                       want_core=False)
        assert relerr(a, a64) <= 1e-5, (info.refine_steps, info.refine_delta, M.dist_info())
        M.close()
    finally:
        vctx.close()


PEER_SCRIPT = r"""
import os, sys, json
import numpy as np
rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
sys.path.insert(0, os.environ["GPRX_ROOT"])
os.environ["GPRX_DIST_SHARED_GPU"] = "1"
import gpr_amd   # (library first, no PyTorch: /opt/rocm's runtime, as bench.py)
from gpr_amd.hostcoll import SocketGroup
from gpr_amd.synth import make_data
dist = SocketGroup(rank, world, port=port)
ctx = gpr_amd.Context(0, peer=(rank, world, dist.allgather_fn()))
assert gpr_amd.runtime_info()["single_copy"] and not gpr_amd.runtime_info()["torch_loaded_first"]
res = {}
X, Y = make_data(1800, 5, 2)
ks = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"
for dt in (np.float64, np.float32):
    M = gpr_amd.Model(ctx, dt)
    M.set_data(X.astype(dt), Y.astype(dt))
    M.set_kernel(ks)
    M.set_noise(0.5)
    info = M.fit()
    res[np.dtype(dt).name] = {"alpha": M.alpha().astype(np.float64).ravel().tolist(), "logdet": info.logdet,
                              "refine_steps": info.refine_steps}
    M.close()
M = gpr_amd.Model(ctx, np.float64)
M.set_data(X, Y[:, :1].copy())
M.set_kernel(ks)
M.set_noise(0.5)
v, g, ld = M.lml(grad=True)
res["lml"] = {"value": v, "grad": list(g), "logdet": ld}
M.close()
ctx.close()
if rank == 0:
    with open(out, "w") as f:
        json.dump(res, f)
dist.barrier()
dist.close()
"""


def test_peer_two_processes(tmp_path):
    """The multi-process form (gprx_ctx_create_peer): two processes share the GPU (each on half
    the CUs, GPRX_DIST_SHARED_GPU), bootstrap through a gloo all-gather, map each other's
    mailboxes with IPC handles and run the sharded fit, fp32 refinement and LML gradient with the
    device-initiated exchange between processes -- the real multi-GPU code path, the peer
    stores crossing process boundaries instead of xGMI.  Checked against the oracle."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "peer.py"
    script.write_text(PEER_SCRIPT)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = str(so.getsockname()[1])
    out = tmp_path / "res.json"
    env = dict(os.environ, GPRX_ROOT=root)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "2", port, str(out)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    res = json.loads(out.read_text())
    X, Y = make_data(1800, 5, 2)
    a_ref, _ = O.fit(C3K, X, Y, 0.5, want_core=False)
    assert relerr(np.array(res["float64"]["alpha"]).reshape(a_ref.shape), a_ref) <= 1e-6
    K = O.kernel_matrix(C3K, X) + 0.25 * np.eye(1800)
    assert abs(res["float64"]["logdet"] - np.linalg.slogdet(K)[1]) <= 1e-9 * abs(res["float64"]["logdet"])
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    a32, _ = O.fit(C3K, X32, Y32, 0.5, np.float32, want_core=False)
    assert res["float32"]["refine_steps"] >= 1
    assert relerr(np.array(res["float32"]["alpha"]).reshape(a32.shape), a32) <= 1e-5
    vr, gr, _, ldr = O.lml(C3K, X, Y[:, :1].copy(), 0.5)
    assert abs(res["lml"]["logdet"] - ldr) <= 1e-9 * abs(ldr)
    assert relerr(np.array(res["lml"]["grad"]), gr) <= 1e-6


def test_peer_two_processes_lml_c3():
    """The sharded LML at C3's size across two PROCESSES (peer context, one GPU shared): with a
    64-panel window the peer's mailbox was 2.19 GB and hipIpcOpenMemHandle of it never returned
    (DESIGN.md 6); the window is now its own allocation in pieces below 2 GiB (2.16 GB at 64 panels:
    two pieces), so the width is the simulation's choice again.  Both ranks must finish and agree
    with the single-GPU likelihood."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = str(so.getsockname()[1])
    probe = os.path.join(root, "scripts", "peer_lml_probe.py")
    procs = [subprocess.Popen([sys.executable, "-u", probe, str(r), "2", port, "16384"], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=120)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    vals = [float(l.split("lml done")[1].split()[0]) for log in logs for l in log.splitlines() if "lml done" in l]
    assert len(vals) == 2 and vals[0] == vals[1]
    import gpr_amd
    from gpr_amd.synth import C3, make_data
    ctx = gpr_amd.Context(0)
    try:
        X, Y = make_data(16384, C3["d"], C3["m"])
        M = gpr_amd.Model(ctx, np.float64)
        M.set_data(X, Y)
        M.set_kernel(C3["kernel"])
        M.set_noise(C3["sigma"])
        v, _, _ = M.lml(grad=True)
        M.close()
    finally:
        ctx.close()
    assert abs(vals[0] - v) <= 1e-9 * abs(v)


def _run_peers(tmp_path, script, args, timeout, env_extra=None):
    """Run `script` as two processes (rank, world = 2, port, *args); return their outputs."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path / "peer_script.py"
    path.write_text(script)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = str(so.getsockname()[1])
    env = dict(os.environ, GPRX_ROOT=root, **(env_extra or {}))
    procs = [subprocess.Popen([sys.executable, "-u", str(path), str(r), "2", port] + [str(a) for a in args], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            logs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return logs


PEER_SKEW_SCRIPT = r"""
import os, sys, time
import numpy as np
rank, world, port, out, n, sleep_s = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]), float(sys.argv[6])
sys.path.insert(0, os.environ["GPRX_ROOT"])
os.environ["GPRX_DIST_SHARED_GPU"] = "1"
import gpr_amd   # (library first, no PyTorch: /opt/rocm's runtime, as bench.py)
from gpr_amd.hostcoll import SocketGroup
from gpr_amd.synth import make_data, make_queries
dist = SocketGroup(rank, world, port=port)
ctx = gpr_amd.Context(0, peer=(rank, world, dist.allgather_fn()))
X, Y = make_data(n, 5, 1)
Xq = make_queries(30, 5)
ks = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"
M = gpr_amd.Model(ctx, np.float64)
M.set_data(X, Y)
M.set_kernel(ks)
M.set_noise(0.5)
M.fit()
a1 = M.alpha()
c1 = M.posterior_cov(Xq, Xq)   # the dense factor gathered from both processes' storage pieces
if rank == 1:
    time.sleep(sleep_s)        # this rank enters the next fit seconds after its peer
M.set_noise(0.7)
M.fit()
a2 = M.alpha()
c2 = M.posterior_cov(Xq, Xq[::-1].copy())
np.savez(f"{out}.r{rank}.npz", a1=a1, c1=c1, a2=a2, c2=c2, info=np.array(M.dist_info()["ww"] if M.dist_info() else 0))
M.close()
ctx.close()
dist.barrier()
dist.close()
"""


def test_peer_rank_skew_and_pieces(tmp_path):
    """Two processes whose second fit starts 5 s apart (rank 1 sleeps: I/O, GC): the reference's
    Initialize has no timing condition between callers (lib/GaussianProcess.cpp:118-130), and a
    host barrier before each sharded launch keeps the per-wait time limit from seeing the skew.
    The storage and window are forced into 4 MiB pieces (GPRX_DIST_PIECE_MB), so the posterior
    covariance's factor gather reads the peer's storage through several IPC mappings.  Both fits'
    alpha and posterior covariances against the oracle, on both ranks."""
    import gpr_amd  # noqa: F401  (the library must load here too)
    n = 1800
    out = tmp_path / "res"
    _run_peers(tmp_path, PEER_SKEW_SCRIPT, [out, n, 5.0], timeout=240, env_extra={"GPRX_DIST_PIECE_MB": "4"})
    X, Y = make_data(n, 5, 1)
    Xq = make_queries(30, 5)
    for r in range(2):
        res = np.load(f"{out}.r{r}.npz")
        for sig, a, c, xb in ((0.5, res["a1"], res["c1"], Xq), (0.7, res["a2"], res["c2"], Xq[::-1].copy())):
            a_ref, C_ref = O.fit(C3K, X, Y, sig)
            assert relerr(a, a_ref) <= 1e-6
            assert relerr(c, O.posterior_cov(C3K, X, C_ref, Xq, xb)) <= 1e-6


@pytest.mark.parametrize("g", [2, 3])
def test_virtual_ranks_pieces(g, monkeypatch):
    """Storage and window split into 2 MiB pieces (separate allocations, as every allocation
    another process maps must stay below 2 GiB): the kernels address a rank's row blocks by
    offsets across its pieces and the window slots through the piece table.  Fit, LML gradient
    and posterior covariance against the oracle."""
    import gpr_amd
    monkeypatch.setenv("GPRX_DIST_PIECE_MB", "2")
    n, d, sigma = 1500, 4, 0.5
    X, Y = make_data(n, d, 1)
    vctx = gpr_amd.Context(0, virtual=g)
    try:
        M, info = _fit(vctx, C3K, X, Y, sigma, np.float64)
        a_ref, C_ref = O.fit(C3K, X, Y, sigma)
        assert relerr(M.alpha(), a_ref) <= 1e-6
        Xa = make_queries(25, d)
        assert relerr(M.posterior_cov(Xa, Xa), O.posterior_cov(C3K, X, C_ref, Xa, Xa)) <= 1e-6
        _, gr, ld = M.lml(grad=True, distributed=True)
        _, grr, _, ldr = O.lml(C3K, X, Y, sigma)  # (the value is the reference's clamp here: compare log det)
        assert abs(ld - ldr) <= 1e-9 * abs(ldr)
        assert relerr(np.asarray(gr), grr) <= 1e-6
        M.close()
    finally:
        vctx.close()


# (this one keeps torch.distributed, imported first: libgprx then runs on the runtime and RCCL
# the PyTorch wheel bundles -- the other supported binding, gpr_amd.runtime_info())
PEER_BIG_SCRIPT = r"""
import os, sys
import numpy as np
rank, world, port, out, n = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5])
sys.path.insert(0, os.environ["GPRX_ROOT"])
os.environ["GPRX_DIST_SHARED_GPU"] = "1"
import torch.distributed as dist
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
import gpr_amd
from gpr_amd.gprx import torch_allgather
from gpr_amd.synth import C3, make_data, make_queries
ctx = gpr_amd.Context(0, peer=(rank, world, torch_allgather()))
X, Y = make_data(n, C3["d"], C3["m"])
M = gpr_amd.Model(ctx, np.float64)
M.set_data(X, Y)
M.set_kernel(C3["kernel"])
M.set_noise(C3["sigma"])
info = M.fit()
Xq = make_queries(64, C3["d"])
cov = M.posterior_cov(Xq, Xq)
rt = gpr_amd.runtime_info()
assert rt["single_copy"] and rt["torch_loaded_first"], rt
if rank == 0:
    np.savez(out, alpha=M.alpha(), cov=cov, storage=np.array(M.dist_info()["bytes_storage"]))
M.close()
ctx.close()
dist.barrier()
dist.destroy_process_group()
"""


def test_peer_two_processes_n32768_fp64(tmp_path):
    """N = 32768 fp64 over two processes: each rank's packed storage is 2.17 GB, above the 2 GiB
    an IPC mapping may have (round 3 left it unmapped and refused the gather); it is now two
    pieces.  alpha and the posterior covariance (the dense factor gathered across the processes)
    against the single-GPU fit of the same data."""
    import gpr_amd
    from gpr_amd.synth import C3
    n = 32768
    out = tmp_path / "big.npz"
    _run_peers(tmp_path, PEER_BIG_SCRIPT, [out, n], timeout=400)
    res = np.load(out)
    assert int(res["storage"]) > 2 ** 31
    X, Y = make_data(n, C3["d"], C3["m"])
    ctx = gpr_amd.Context(0)
    try:
        M = gpr_amd.Model(ctx, np.float64)
        M.set_data(X, Y)
        M.set_kernel(C3["kernel"])
        M.set_noise(C3["sigma"])
        M.fit()
        Xq = make_queries(64, C3["d"])
        assert relerr(res["alpha"], M.alpha()) <= 1e-9
        assert relerr(res["cov"], M.posterior_cov(Xq, Xq)) <= 1e-9
        M.close()
    finally:
        ctx.close()


def test_bench_two_processes_rccl_fallback(tmp_path):
    """bench.py's N > 1 path as the driver launches it (torch.distributed.run, one process per
    rank), rehearsed on one GPU (GPRX_DIST_SHARED_GPU) with the RCCL initialisation failed on
    purpose (GPRX_RCCL_FAIL): every rank falls back to the peer context over the socket group,
    the sharded fit runs, the failure is reported in dist_error, and the processes map one HIP
    runtime (/opt/rocm's; no PyTorch in a bench rank)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = str(so.getsockname()[1])
    env = dict(os.environ, GPRX_DIST_SHARED_GPU="1", GPRX_RCCL_FAIL="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", port, os.path.join(root, "bench.py"), "--gpus", "2", "--full", "--steps", "2",
           "--warmup", "1", "--ntrain", "2048", "--configs", "0", "--lml", "0", "--build-iters", "0", "--cpu-n", "0",
           "--predict-q", "256", "--variance-q", "0", "--cpu-lml-ns", "", "--cpu-predict-q", "0"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["dist_transport"].startswith("peer (fallback"), line["dist_transport"]
    assert "GPRX_RCCL_FAIL" in line["dist_error"]
    assert line["config"]["parallelism"].startswith("sharded")
    rt = line["runtime"]
    assert rt["single_copy"] and not rt["torch_loaded_first"], rt


def test_bench_spawns_ranks_without_launcher():
    """`bench.py --gpus 2` with NO launcher: bench.py starts the two ranks
    itself, before any GPU call, and relays rank 0's one JSON line.  Rehearsed on one GPU
    (GPRX_DIST_SHARED_GPU: both ranks on device 0, the peer context).  The line must say
    n_gpus 2 and ranks_seen 2, and carry per rank the device, the transport, the Linv / tile
    pushes per fit and their bytes, and the measured diagonal-chain step,
    consistent across the ranks."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["GPRX_DIST_SHARED_GPU"] = "1"
    env["GPRX_BENCH_TIMEOUT_S"] = "280"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--full", "--steps", "2", "--warmup", "1",
           "--configs", "0", "--ntrain", "4096", "--lml", "0", "--build-iters", "0", "--cpu-n", "0",
           "--predict-q", "256", "--variance-q", "0", "--cpu-lml-ns", "", "--cpu-predict-q", "0"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["value"] > 0
    assert line["launcher"] == "bench.py spawn"
    assert line["config"]["parallelism"].startswith("sharded"), line["dist_error"]
    ranks = sorted(line["ranks"], key=lambda x: x["rank"])
    assert [x["rank"] for x in ranks] == [0, 1] and all(x["world"] == 2 for x in ranks)
    for x in ranks:
        assert x["transport"] == "peer" and x["device"] == 0 and x["pci"]
        # every rank owns diagonal blocks: it pushes each Linv_k to its one peer, and final tiles
        assert x["push_linv"] > 0 and x["push_tiles"] > 0
        assert x["push_bytes"] == (x["push_linv"] + x["push_tiles"]) * 128 * 128 * 8
        assert x["chain_step_us_median"] is not None and 1.0 < x["chain_step_us_median"] < 5000.0
        assert x["diag_steps_owned"] > 0
    # the ranks' diagonal blocks partition the 32 steps, and a Linv push per owned block
    assert sum(x["diag_steps_owned"] for x in ranks) == 4096 // 128
    assert sum(x["push_linv"] for x in ranks) == 4096 // 128
    assert line["distinct_devices"] == 1  # (one shared GPU here; one per rank on a node)


PEER_SLICE_SCRIPT = r"""
import os, sys
import numpy as np
rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
sys.path.insert(0, os.environ["GPRX_ROOT"])
os.environ["GPRX_DIST_SHARED_GPU"] = "1"
import gpr_amd
from gpr_amd.hostcoll import SocketGroup
from gpr_amd.synth import make_data, make_queries
grp = SocketGroup(rank, world, port=port)
ctx = gpr_amd.Context(0, peer=(rank, world, grp.allgather_fn()))
X, Y = make_data(1500, 5, 1)
Xq = make_queries(37, 5)
ks = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"
M = gpr_amd.Model(ctx, np.float64)
M.set_data(X, Y)
M.set_kernel(ks)
M.set_noise(0.5)
M.fit()
lo, hi = gpr_amd.query_shard(37, rank, world)
v_own = M.posterior_cov(Xq[lo:hi], Xq[lo:hi])           # variances, each process its own slice
c_own = M.posterior_cov(Xq[lo:hi], Xq[::-1][lo:hi].copy())  # pairs x != y, own slices
e = Xq[:0]
v_one = M.posterior_cov(Xq[:9], Xq[:9]) if rank == 0 else M.posterior_cov(e, e)  # rank 1: no pairs
v_all = M.posterior_cov(Xq, Xq)                          # identical arguments everywhere
np.savez(f"{out}.r{rank}.npz", v_own=v_own, c_own=c_own, v_one=v_one, v_all=v_all, lo=lo, hi=hi,
         pv=np.array(M.dist_info()["posterior_bytes_rank"]))
M.close()
ctx.close()
grp.barrier()
grp.close()
"""


def test_peer_posterior_differing_slices(tmp_path):
    """posterior_cov on a sharded fit is a collective: two processes passing their OWN query_shard
    slices (different q, different queries; one process with none) get their own variances and
    covariances -- the arguments are agreed first and differing ones solved together -- instead
    of a hang or another process's values (round-4 advisor finding).  Against the oracle; the
    posterior workspace per rank is K(Z, X_own): the queries x that rank's rows only."""
    n = 1500
    out = tmp_path / "res"
    _run_peers(tmp_path, PEER_SLICE_SCRIPT, [out], timeout=240)
    X, Y = make_data(n, 5, 1)
    Xq = make_queries(37, 5)
    _, C_ref = O.fit(C3K, X, Y, 0.5)
    for r in range(2):
        res = np.load(f"{out}.r{r}.npz")
        lo, hi = int(res["lo"]), int(res["hi"])
        assert relerr(res["v_own"], O.posterior_cov(C3K, X, C_ref, Xq[lo:hi], Xq[lo:hi])) <= 1e-6
        assert relerr(res["c_own"], O.posterior_cov(C3K, X, C_ref, Xq[lo:hi], Xq[::-1][lo:hi].copy())) <= 1e-6
        assert relerr(res["v_all"], O.posterior_cov(C3K, X, C_ref, Xq, Xq)) <= 1e-6
        if r == 0:
            assert relerr(res["v_one"], O.posterior_cov(C3K, X, C_ref, Xq[:9], Xq[:9])) <= 1e-6
        else:
            assert res["v_one"].size == 0
        # (K(Z, X_own): at most the padded chunks x this rank's ~half of the 12 row blocks, not all N)
        assert 0 < int(res["pv"]) <= 8 * 128 * 2 * 7 * 128
