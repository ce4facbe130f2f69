"""Label blocks wider than three columns, against the CPU oracle in fp64.

What depends on the number of label columns m: the label row tiles of the factorisation
(mp = round_up(m, 128): a second one from m = 129), the per-column loops and flag arrays of the
chained substitutions, model_append's 128-row slabs of label rows, refine_f32's per-column
launches, the LU solve's groups of eight right-hand sides, the data-fit reduction, the direct
predict kernel's passes over 64 columns of Z = [alpha | alpha o X] and the sharded fit's limit of
128 columns.

The columns of make_labels really differ (amplitude, frequency, input dimension, phase), and
every error is the maximum over columns of the column's own relative error, so one wrong column
cannot hide under the matrix norm.  Tolerances are those of the existing tests of the same
entry point (tests/test_gpu_parity.py, test_gpu_append.py, test_gpu_lu.py, test_gpu_dist.py,
test_gpu_sparse.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import SEED, make_data, make_queries, relerr, uniform, TOL
from tests.test_gpu_trees import TREES

gpu = pytest.mark.gpu

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = [np.float64, np.float32]
SIGMA = 0.5
GAUSS = "GaussianKernel(0.7,1.3,)"                              # MFMA build, per-column MFMA refine
GWHITE = "SumKernel(GaussianKernel(0.8,1,),WhiteKernel(0.3,))"  # direct build, direct refine (ncz = m)
GPER = "SumKernel(GaussianKernel(0.7,1.3,),PeriodicKernel(0.9,2.5,0.8,))"
PER = "PeriodicKernel(0.9,2.5,0.8,)"
C3K = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"
# one kernel per (NPER, R2) instantiation of predict_kernel
PREDICT_KERNELS = {"gauss": GAUSS, "gauss_per": GPER, "per": PER, "2per_sum": TREES["2per_sum"],
                   "2per_sum_gauss": TREES["2per_sum_gauss"]}


def make_labels(n, d, m):
    """X of make_data(n, d) and Y[:, c] = (1 + 0.25 (c mod 7)) sin(2 pi (1 + c mod 3) X[:, c mod d] + 0.37 c)
    + 0.1 (2u - 1), u = uniform(SEED + 0x9E37, n m) as n x m.  Like make_data, the first n rows of a
    longer set are the set of n rows: a test that appends fits a prefix and appends the rest."""
    X, _ = make_data(n, d)
    c = np.arange(m)
    u = uniform(SEED + 0x9E37, n * m).reshape(n, m)
    Y = (1 + 0.25 * (c % 7)) * np.sin(2 * np.pi * (1 + c % 3) * X[:, c % d] + 0.37 * c) + 0.1 * (2 * u - 1)
    return X, Y


def colerr(a, ref):
    """Maximum over label columns (the last axis) of relerr of the column; for the derivative
    (q x d x m) over every slab [:, k, c]."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape
    a, ref = a.reshape(a.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return max(relerr(a[:, c], ref[:, c]) for c in range(ref.shape[1]))


_refs = {}


def oracle_fit(ks, n, d, m, sigma=SIGMA):
    """(X, Y, alpha, log det, data fit) of the oracle on make_labels(n, d, m), computed once, read-only."""
    key = (ks, n, d, m, sigma)
    if key not in _refs:
        X, Y = make_labels(n, d, m)
        a, _ = O.fit(ks, X, Y, sigma, want_core=False)
        ld = np.linalg.slogdet(O.kernel_matrix(ks, X) + sigma * sigma * np.eye(n))[1]
        for v in (X, Y, a):
            v.setflags(write=False)
        _refs[key] = (X, Y, a, ld, float(np.sum(Y * a)))
    return _refs[key]


def model(ctx, ks, X, Y, dtype=np.float64, sigma=SIGMA):
    import gpr_amd
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X.astype(dtype), Y.astype(dtype))
    M.set_kernel(ks)
    M.set_noise(sigma)
    return M


def check_fit(M, info, ks, ref, dtype, q=70):
    """alpha per column, log det, data fit and the predicted mean per column."""
    X, Y, a_ref, ld_ref, df_ref = ref
    tol = TOL[np.dtype(dtype)]
    small = 1e-8 if np.dtype(dtype) == F64 else 1e-3
    ea = colerr(M.alpha(), a_ref)
    Xq = make_queries(q, X.shape[1])
    ep = colerr(M.predict(Xq.astype(dtype)), O.predict(ks, X, a_ref, Xq))
    eld = abs(info.logdet - ld_ref) / max(1.0, abs(ld_ref))
    edf = abs(info.datafit - df_ref) / abs(df_ref)
    print(f"n={X.shape[0]} m={Y.shape[1]} {np.dtype(dtype).name}: alpha {ea:.3e} predict {ep:.3e} "
          f"logdet {eld:.3e} datafit {edf:.3e}")
    assert ea <= tol
    assert ep <= tol
    assert eld <= small
    assert edf <= small


# ---------------------------------------------------------------------------------------
# the fixtures themselves (CPU)
# ---------------------------------------------------------------------------------------
def test_fixture_columns_differ():
    """Any two columns of the oracle's alpha, each scaled to unit max-norm, differ by at least ten
    times the fp32 tolerance (so a column read or written in another's place is an error far above
    every tolerance used here), and column c of the m-column fit is the single-column fit of
    Y[:, c] (the reference itself keeps the columns apart)."""
    n, d, m = 300, 3, 130
    X, Y, a, _, _ = oracle_fit(GAUSS, n, d, m)
    A = a / np.max(np.abs(a), axis=0)
    gap = min(np.max(np.abs(A[:, i] - A[:, j])) for i in range(m) for j in range(i))
    assert gap >= 10 * TOL[F32], gap
    for c in range(m):
        a1, _ = O.fit(GAUSS, X, Y[:, c:c + 1], SIGMA, want_core=False)
        assert relerr(a[:, c], a1[:, 0]) <= 1e-12, c
    Xp, Yp = make_labels(n + 100, d, m)  # (what test_append relies on)
    assert np.array_equal(Xp[:n], X) and np.array_equal(Yp[:n], Y)


# ---------------------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ks", [GAUSS, GWHITE], ids=["gauss", "gauss_white"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,m", [(300, 3, 4), (300, 3, 64), (300, 3, 65), (300, 3, 128), (300, 3, 129),
                                   (300, 3, 130), (100, 4, 129)])
def test_fit_parity(ctx, ks, dtype, n, d, m):
    """One label row tile (m <= 128) and two; three 128-blocks (the chained solves stream tiles
    j > k + 1) and one."""
    ref = oracle_fit(ks, n, d, m)
    M = model(ctx, ks, ref[0], ref[1], dtype)
    info = M.fit()
    assert info.method == 0
    check_fit(M, info, ks, ref, dtype)
    M.close()


@gpu
@pytest.mark.parametrize("m", [7, 8, 9, 130])
def test_forced_lu(ctx, m):
    """lu_solve's groups of eight right-hand sides: one short of a group, a whole group, one
    more, and seventeen groups with a ragged last one."""
    from gpr_amd import gprx
    ref = oracle_fit(GAUSS, 300, 3, m)
    M = model(ctx, GAUSS, ref[0], ref[1])
    info = M.fit(gprx.FIT_FORCE_LU)
    assert info.method == 1
    check_fit(M, info, GAUSS, ref, np.float64)
    M.close()


# ---------------------------------------------------------------------------------------
# append
# ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,k", [(300, 1), (300, 100)])
@pytest.mark.parametrize("m", [5, 128, 129])
@pytest.mark.parametrize("gemm", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_append(ctx, dtype, gemm, m, n, k):
    """The label rows of the extended factor, solved in slabs of 128 rows by the chained panel
    kernel (a second slab from m = 129) or by trsm_rows over mp rows; inside the padding and with
    the re-layout (ld1 = np1 + mp)."""
    from gpr_amd import gprx
    d = 3
    ref = oracle_fit(GAUSS, n + k, d, m)
    X, Y = ref[0], ref[1]
    M = model(ctx, GAUSS, X[:n], Y[:n], dtype)
    M.fit()
    info = M.append(X[n:].astype(dtype), Y[n:].astype(dtype), gprx.APPEND_SOLVE_GEMM if gemm else 0)
    assert info.appended == k and info.method == 0
    assert M.n == n + k and M.alpha().shape == (n + k, m)
    check_fit(M, info, GAUSS, ref, dtype, q=64)
    M.close()


# ---------------------------------------------------------------------------------------
# the direct predict kernel alone
# ---------------------------------------------------------------------------------------
# (d, m, deriv): ncz = m (1 + d) columns of Z with derivatives, m without; 64 columns per pass
PREDICT_SHAPES = [
    (7, 8, True),    # ncz 64: one full pass
    (4, 13, True),   # ncz 65: a second pass of one column
    (32, 1, True),   # ncz 33 (the C3 width)
    (32, 2, True),   # ncz 66
    (63, 1, True),   # ncz 64
    (64, 1, True),   # ncz 65 (the C5 width)
    (33, 3, True),   # ncz 102
    (3, 64, False),
    (3, 65, False),
    (3, 130, False),  # three passes, the last one of two columns
]
# fp32 too: every row with ncz 65, 66 or 102
PREDICT_F32 = {(4, 13, True), (64, 1, True), (3, 65, False), (32, 2, True), (33, 3, True)}


@gpu
@pytest.mark.parametrize("kname", list(PREDICT_KERNELS))
@pytest.mark.parametrize("d,m,deriv,dtype",
                         [(d, m, dv, np.float64) for d, m, dv in PREDICT_SHAPES]
                         + [(d, m, dv, np.float32) for d, m, dv in PREDICT_SHAPES if (d, m, dv) in PREDICT_F32])
def test_predict_alone(ctx, kname, d, m, deriv, dtype):
    """The oracle's alpha installed with set_alpha, no fit: what fails here is the predict
    kernel's.  q = 1, one full query block, one more query, four ragged blocks.

    With q = 1 a column is one value and its relative error is that value's own.  The predicted
    functions change sign (alpha does, from sample to sample), and a value at a zero crossing has
    no relative accuracy in any arithmetic: at make_queries' first point the (d, m) = (4, 13)
    Gaussian mean has a column 7e5 eps off in fp64 and 5e-2 off in fp32, against 1e-13 and 1e-5 over
    the column of 200 queries.  So the 200 queries are ordered by the oracle's predictions alone:
    first comes the query whose values are, over every column and slab, farthest from zero on the
    scale of that column's maximum, where the single value's error is closest to the normwise error
    the tolerances are stated for (tests/helpers.relerr).  The other cases take prefixes of the
    same order."""
    ks = PREDICT_KERNELS[kname]
    n = 200
    X, Y, a_ref, _, _ = oracle_fit(ks, n, d, m)
    tol = TOL[np.dtype(dtype)]
    M = model(ctx, ks, X, Y, dtype)
    M.set_alpha(a_ref)
    Xq_all = make_queries(200, d)
    mr_all, Dr_all = O.predict(ks, X, a_ref, Xq_all, with_deriv=True)
    cols = np.abs(np.concatenate([mr_all, Dr_all.reshape(200, -1)], axis=1) if deriv else mr_all)
    first = int(np.argmax(np.min(cols / np.max(cols, axis=0), axis=1)))
    order = np.r_[first, np.delete(np.arange(200), first)]
    Xq_all, mr_all, Dr_all = Xq_all[order], mr_all[order], Dr_all[order]
    worst = 0.0
    for q in (1, 64, 65, 200):
        Xq = Xq_all[:q].astype(dtype)
        if deriv:
            mean, D = M.predict(Xq, deriv=True)
            ed = colerr(D, Dr_all[:q])
            worst = max(worst, ed)
            assert ed <= tol, q
        else:
            mean = M.predict(Xq)
        em = colerr(mean, mr_all[:q])
        worst = max(worst, em)
        assert em <= tol, q
    print(f"predict {kname} d={d} m={m} deriv={deriv} {np.dtype(dtype).name}: worst over q {worst:.3e}")
    M.close()


# ---------------------------------------------------------------------------------------
# the sharded fit
# ---------------------------------------------------------------------------------------
@gpu
def test_sharded_fit_128_columns_and_refusal():
    """The sharded fit keeps the labels in one 128-row block: m = 128 fits, m = 129 is refused
    with GPRX_ERR_DIM before any device work, and the context goes on fitting."""
    import gpr_amd
    n, d = 700, 5
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        ref = oracle_fit(C3K, n, d, 128)
        M = model(vctx, C3K, ref[0], ref[1])
        info = M.fit()
        check_fit(M, info, C3K, ref, np.float64, q=50)
        M.close()
        X, Y = make_labels(n, d, 129)
        M = model(vctx, C3K, X, Y)
        with pytest.raises(gpr_amd.GprxError) as e:
            M.fit()
        assert e.value.status == 4 and "at most 128 label columns" in str(e.value)  # GPRX_ERR_DIM
        M.close()
        ref = oracle_fit(C3K, n, d, 1)
        M = model(vctx, C3K, ref[0], ref[1])
        info = M.fit()
        check_fit(M, info, C3K, ref, np.float64, q=50)
        M.close()
    finally:
        vctx.close()


# ---------------------------------------------------------------------------------------
# the sparse fit
# ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ks,sigma,jitter", [(GAUSS, 0.3, 1e-4), (TREES["2per_sum_gauss"], 0.5, 1e-4)],
                         ids=["gauss", "2per_sum_gauss"])
@pytest.mark.parametrize("m", [5, 129])
def test_sparse_fit(ctx, ks, sigma, jitter, m):
    """RV per column; Kinv and RM do not depend on the labels: bit for bit those of the m = 1
    call on the same inputs (for the Gaussian that call takes the labels through the cross
    build's epilogue instead of a label row tile)."""
    n, d, Mi = 700, 3, 40
    X, Y = make_labels(n, d, m)
    Xm = X[:: n // Mi][:Mi].copy()
    Kinv, RV, RM = ctx.sparse_fit(ks, X, Y, Xm, sigma, jitter)
    Ki_r, RV_r, RM_r = O.sparse_fit(ks, X, Y, Xm, sigma, jitter)
    assert colerr(RV, RV_r) <= TOL[F64]
    assert relerr(Kinv, Ki_r) <= TOL[F64] and relerr(RM, RM_r) <= TOL[F64]
    Kinv1, RV1, RM1 = ctx.sparse_fit(ks, X, Y[:, :1].copy(), Xm, sigma, jitter)
    assert relerr(RV1[:, 0], RV_r[:, 0]) <= TOL[F64]
    assert np.array_equal(Kinv, Kinv1)
    assert np.array_equal(RM, RM1)
