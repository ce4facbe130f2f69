"""The sparse-GP reuse scenarios without a GPU (tests/sparse_reuse_ref.py).

1. The table is sound: every step is conditioned so that the oracle comparison of
   test_gpu_sparse_reuse.py cannot fail on the oracle's own account.
2. The runner can fail: a numpy context that keeps a 128-padded persistent block like the
   library's, with switches that each plant one defect; every scenario passes with all switches
   off, and each defect is reported at the first step where it matters.
3. The clearing plan (sparse_plan.cpp through gprx_dev_sparse_clear_plan): every scenario and a few
   hundred random call sequences replayed on a mask of the block's possibly non-zero elements --
   whatever a chunk's accumulation reads is written by that chunk or known to be zero.  The rule
   before the rows [M, Mp) were tracked, restated here, fails the same replay; at C5's shapes both
   give the same memsets.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from gpr_amd import gprx
from oracle import oracle as O
from tests import matern_ref
from tests import sparse_reuse_ref as R
from tests.helpers import relerr

F64, F32 = R.F64, R.F32


def _distinct(dtype):
    """The distinct (kernel, inputs, sigma, jitter) of the table's good steps of one dtype."""
    seen, out = set(), []
    for _, _, st in R.all_steps():
        key = (st["n"], st["d"], st["M"], st["m"], st["ks"], st["sigma"], st["jitter"], st["seed"])
        if st["raises"] is None and st["dtype"] == dtype and key not in seen:
            seen.add(key)
            out.append(st)
    return out


# ---------------------------------------------------------------------------------------
# 1. the table is sound
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bar", [(F64, 1e-8), (F32, 1e-3)])
def test_table_is_well_conditioned(dtype, bar):
    """cond(S) <= 2e7 and cond(Kmm + jitter I) <= 1e4 for every step, and the oracle's RV and RM
    against a direct solve of S assembled in long double (from the step's inputs as rounded to its
    dtype): fp64 1e-8 -- two orders under the 1e-6 of the GPU comparison -- and fp32 at its 1e-3."""
    steps = _distinct(dtype)
    assert steps
    worst = [0.0, 0.0, 0.0]
    for st in steps:
        X, Y, Xm = R.inputs(st)
        _, RV, RM, S, K = R.numpy_sparse_fit(st["ks"], X, Y, Xm, st["sigma"], st["jitter"])
        cS, cK = np.linalg.cond(S), np.linalg.cond(K)
        assert cS <= 2e7 and cK <= 1e4, (st, cS, cK)
        worst[0], worst[1] = max(worst[0], cS), max(worst[1], cK)
        if "Matern" in st["ks"]:
            continue  # (no oracle form: the direct solve is the reference of that step)
        _, RV_o, RM_o = O.sparse_fit(st["ks"], X, Y, Xm, st["sigma"], st["jitter"], dtype)
        e = max(relerr(RV_o, RV), relerr(RM_o, RM))
        assert e <= bar, (st, e)
        worst[2] = max(worst[2], e)
    print(f"{dtype.name}: {len(steps)} steps, cond(S) <= {worst[0]:.2e}, cond(K) <= {worst[1]:.2e}, "
          f"oracle vs direct <= {worst[2]:.2e}")


def test_failing_steps_fail_for_their_reason():
    """The NaN step's NaN row is not an inducing point and the sigma = 0 step has nothing else
    wrong.  The table has no NOT_SPD step: with lifecycle_ref's indefinite kernel S stays positive
    definite at these shapes, so such a step would not raise."""
    failing = [st for _, _, st in R.all_steps() if st["raises"] is not None]
    assert sorted(st["raises"] for st in failing) == [R.ERR_NONFINITE, R.ERR_ARG]
    for st in failing:
        X, Y, Xm = R.inputs(st)
        if st["raises"] == R.ERR_NONFINITE:
            assert np.isnan(X).sum() == 1 and np.all(np.isfinite(Xm))
        else:
            assert st["sigma"] == 0.0 and np.all(np.isfinite(X))
    st = R.fit(600, 8, 140, 1, R.INDEF, seed=5)
    S = R.numpy_sparse_fit(st["ks"], *R.inputs(st), st["sigma"], st["jitter"])[3]
    assert np.linalg.eigvalsh(S)[0] > 0


# ---------------------------------------------------------------------------------------
# 2. the runner can fail
# ---------------------------------------------------------------------------------------
class FakeError(RuntimeError):
    def __init__(self, status):
        super().__init__(f"status {status}")
        self.status = status


class FakeSparseContext:
    """sparse_fit / sparse_lml in numpy along the library's steps: a persistent streamed block per
    dtype (column-major there, (row, column) here) that follows the library's clearing rule, chunks
    of the library's sizes, the rank-k accumulation over whole 128-row tiles and the split-K
    slices' columns, the identity written on the padding's diagonal only.  defect plants one of
      rows    -- rows [M, Mp) not cleared on shrink (the library before sparse_plan.cpp)
      cols    -- columns past nc not cleared after a longer chunk
      labels  -- the fused accumulation also reads the label rows, kept from an m = 3 call
      kernel  -- the previous kernel's parameters kept when the tree is the same
    """

    def __init__(self, defect=None):
        assert defect in (None, "rows", "cols", "labels", "kernel")
        self.defect = defect
        self.blocks = {}
        self.tree = None

    def close(self):
        self.blocks = None

    def _kernel(self, ks):
        skeleton = re.sub(r"[-0-9.e]+,", "", ks)
        if self.defect == "kernel" and self.tree and self.tree[0] == skeleton:
            return self.tree[1]
        self.tree = (skeleton, ks)
        return ks

    def _normal_eq(self, ks, X, Y, Xm, sigma, jitter, dtype):
        if not sigma > 0:
            raise FakeError(R.ERR_ARG)
        ks = self._kernel(ks)
        X, Y, Xm = (np.asarray(a, np.float64) for a in (X, Y, Xm))
        (n, _), M, m = X.shape, Xm.shape[0], Y.shape[1]
        sh = R.shapes(n, M, m, ks not in R.VALU, os.environ.get(R.CHUNK_ENV))
        Mp, mp, ld, fused = sh["Mp"], sh["mp"], sh["ld"], sh["fused"]
        blk = self.blocks.setdefault(np.dtype(dtype).name, dict(key=None))
        if blk["key"] != (ld, sh["acols"], Mp):  # a new block layout: zero it whole
            blk.update(key=(ld, sh["acols"], Mp), A=np.zeros((ld, sh["acols"])), zero=0, rows=0)
        A = blk["A"]
        is2 = 1.0 / (sigma * sigma)
        S = np.zeros((ld, Mp))
        bad, off = False, 0
        for nc, rows_read, cols_read in sh["chunks"]:
            ncp = R._up(nc, 16)
            if blk["zero"] > nc:
                if self.defect != "cols":
                    A[:, nc:blk["zero"]] = 0
                blk["zero"] = nc
            if blk["rows"] > M:
                if self.defect != "rows":
                    A[M:blk["rows"], :blk["zero"]] = 0
                blk["rows"] = M
            blk["rows"], blk["zero"] = max(blk["rows"], M), max(blk["zero"], ncp)
            Xc, Yc = X[off:off + nc], Y[off:off + nc]
            Kc = matern_ref.cross(ks, Xm, Xc)
            bad = bad or not np.all(np.isfinite(Kc))
            A[:M, :nc] = Kc
            if not fused:
                A[Mp:Mp + mp, :ncp] = 0
                A[Mp:Mp + m, :nc] = Yc.T
            r = ld if (fused and self.defect == "labels") else rows_read
            with np.errstate(invalid="ignore"):
                S[:r] += is2 * (A[:r, :cols_read] @ A[:Mp, :cols_read].T)
                if fused:
                    S[Mp, :M] += is2 * (Kc @ Yc[:, 0])
            off += nc
        K = matern_ref.cross(ks, Xm, Xm) + jitter * np.eye(M)
        S[:M, :M] += K
        S[np.arange(M, Mp), np.arange(M, Mp)] = 1.0  # the diagonal of the padding, nothing else
        if bad or not np.all(np.isfinite(K)):
            raise FakeError(R.ERR_NONFINITE)
        Sl = np.tril(S[:Mp])
        Ss = Sl + np.tril(Sl, -1).T
        try:
            if not np.all(np.isfinite(Ss)):
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(Ss)
        except np.linalg.LinAlgError:
            raise FakeError(R.ERR_NOT_SPD) from None
        return ks, Ss, L, S[Mp:Mp + m, :].T.copy(), K, M

    def sparse_fit(self, ks, X, Y, Xm, sigma, jitter, dtype=np.float64):
        _, Ss, _, b, K, M = self._normal_eq(ks, X, Y, Xm, sigma, jitter, dtype)
        return tuple(np.ascontiguousarray(a, dtype) for a in
                     (np.linalg.inv(K), np.linalg.solve(Ss, b)[:M], np.linalg.inv(Ss)[:M, :M]))

    def sparse_lml(self, ks, X, y, Xm, sigma, jitter, dtype=np.float64, grad=True, compat=False):
        y = np.asarray(y, np.float64)
        ks, _, L, b, K, _ = self._normal_eq(ks, X, y[:, None], Xm, sigma, jitter, dtype)
        n = y.shape[0]
        z = np.linalg.solve(L, b[:, 0])
        ld = n * np.log(sigma * sigma) + 2 * np.sum(np.log(np.diag(L))) - np.linalg.slogdet(K)[1]
        v = -0.5 * (y @ y / (sigma * sigma) - z @ z) - 0.5 * ld - 0.5 * n * np.log(2 * np.pi)
        # (the gradient does not pass through the block: the oracle's, of the kernel in effect)
        g = None
        if grad:
            key = (ks, sigma, jitter, np.dtype(dtype).name, np.asarray(X).tobytes(), np.asarray(Xm).shape)
            if key not in _GRADS:
                _GRADS[key] = np.asarray(O.sparse_lml(ks, X, y, Xm, sigma, jitter, dtype)[1], np.float64)
            g = _GRADS[key].copy()
        return float(v), g, float(ld)


_GRADS = {}


@pytest.mark.parametrize("name", list(R.SCENARIOS))
def test_runner_passes_on_a_sound_context(name):
    R.run(name, FakeSparseContext)


# (defect, the scenario built for it, the first step where it matters, what notices)
PLANTED = [
    ("rows", "shrink_g", 1, "twin"),      # 140 -> 130
    ("rows", "shrink_gw", 1, "twin"),
    ("rows", "shrink_small", 1, "twin"),  # 40 -> 33
    ("rows", "shrink_lml", 1, "twin"),    # the LML at 130 after the fit at 140
    ("rows", "failures", 5, "twin"),      # 130 after 140, the NaNs of the failed call among the rows
    ("cols", "rows", 1, "oracle"),        # n = 1300: the ragged second chunk after the first (a fresh context too)
    ("labels", "labels", 2, "twin"),      # m = 1 fused after m = 3
    ("kernel", "kernels", 7, "twin"),     # G's tree with new parameters
]


@pytest.mark.parametrize("defect,name,step,kind", PLANTED)
def test_runner_reports_a_planted_defect(defect, name, step, kind):
    with pytest.raises(R.Mismatch) as e:
        R.run(name, lambda: FakeSparseContext(defect))
    assert (e.value.scenario, e.value.step, e.value.kind) == (name, step, kind), str(e.value)


# ---------------------------------------------------------------------------------------
# 3. the clearing plan
# ---------------------------------------------------------------------------------------
def _lib():
    L = ctypes.CDLL(gprx.LIB_PATH)
    L.gprx_dev_sparse_clear_plan.restype = ctypes.c_int32
    L.gprx_dev_sparse_clear_plan.argtypes = [ctypes.c_void_p] + [ctypes.c_int64] * 6 + [ctypes.c_void_p]
    return L


class HookRule:
    """The library's rule (gprx_dev_sparse_clear_plan)."""

    def __init__(self):
        self.L, self.state = _lib(), np.zeros(6, np.int64)

    def __call__(self, blk, ld, cols, Mp, M, nc):
        rects = np.zeros(12, np.int64)
        k = self.L.gprx_dev_sparse_clear_plan(self.state.ctypes.data, blk, ld, cols, Mp, M, nc, rects.ctypes.data)
        assert 0 <= k <= 3
        return [tuple(int(v) for v in rects[4 * q:4 * q + 4]) for q in range(k)]


class ParentRule:
    """The rule before the rows were tracked: the block zeroed whole when its address, ld or
    columns change, else only the columns [nc, zero) that a longer chunk left."""

    def __init__(self):
        self.key, self.zero = None, 0

    def __call__(self, blk, ld, cols, Mp, M, nc):
        out = []
        if self.key != (blk, ld, cols):
            out.append((0, ld, 0, cols))
            self.key, self.zero = (blk, ld, cols), 0
        if self.zero > nc:
            out.append((0, ld, nc, self.zero - nc))
            self.zero = nc
        self.zero = max(self.zero, R._up(nc, 16))
        return out


def replay(calls, rule, ncu=256, record=None):
    """calls: (n, M, m, mma, chunk_env).  One grow-only allocation at a fixed address, so a layout
    is laid over whatever the earlier ones left: everything counts as possibly non-zero then.
    Returns None, or (call, chunk, rows, columns) of the first accumulation that would read
    an element neither stored by its chunk nor known to be zero."""
    dirty, layout = None, None
    for ci, (n, M, m, mma, chunk_env) in enumerate(calls):
        sh = R.shapes(n, M, m, mma, chunk_env, ncu)
        Mp, ld, cols = sh["Mp"], sh["ld"], sh["acols"]
        if layout != (ld, cols):
            dirty, layout = np.ones((ld, cols), bool), (ld, cols)
        for ki, (nc, rows_read, cols_read) in enumerate(sh["chunks"]):
            assert cols_read <= cols
            rects = rule(1, ld, cols, Mp, M, nc)
            if record is not None:
                record.append(rects)
            for r0, nr, c0, ncl in rects:
                assert 0 <= r0 and r0 + nr <= ld and 0 <= c0 and c0 + ncl <= cols and nr > 0 and ncl > 0
                dirty[r0:r0 + nr, c0:c0 + ncl] = False
            ncp = R._up(nc, 16)
            stored = np.zeros((ld, cols), bool)
            stored[:M, :nc] = True
            if not sh["fused"]:
                stored[Mp:, :ncp] = True
            stale = dirty[:rows_read, :cols_read] & ~stored[:rows_read, :cols_read]
            if stale.any():
                rr, cc = np.nonzero(stale)
                return ci, ki, (int(rr.min()), int(rr.max()) + 1), (int(cc.min()), int(cc.max()) + 1)
            dirty[:M, :nc] = True
            if not sh["fused"]:
                dirty[Mp:, :ncp] = False  # written whole: the labels, zeros around them
                dirty[Mp:Mp + m, :nc] = True
    return None


def _calls(name):
    return [(st["n"], st["M"], st["m"], st["ks"] not in R.VALU, st["chunk"])
            for st in R.SCENARIOS[name] if st["raises"] != R.ERR_ARG and st["dtype"] == F64]


@pytest.mark.parametrize("ncu", [256, 304, 8])
@pytest.mark.parametrize("name", list(R.SCENARIOS))
def test_clearing_plan_covers_every_scenario(name, ncu):
    assert replay(_calls(name), HookRule(), ncu) is None


@pytest.mark.parametrize("name", ["shrink_g", "shrink_gw", "shrink_small", "shrink_lml"])
def test_parent_rule_fails_the_shrink_scenarios(name):
    """The first shrink (call 1, its first chunk) reads the rows [M, earlier M) of the earlier call."""
    calls = _calls(name)
    bad = replay(calls, ParentRule())
    assert bad is not None
    ci, ki, rows, _ = bad
    assert (ci, ki) == (1, 0) and rows == (calls[1][1], calls[0][1])


def _random_calls(rng, count):
    return [(int(rng.choice([600, 1300])), int(rng.choice([33, 40, 128, 129, 130, 140])), int(rng.choice([1, 3])),
             bool(rng.integers(2)), [None, 256, 1024][rng.integers(3)]) for _ in range(count)]


def test_clearing_plan_covers_random_sequences():
    rng = np.random.default_rng(0x53505253)
    parent_bad = 0
    for _ in range(300):
        calls = _random_calls(rng, 8)
        assert replay(calls, HookRule()) is None, calls
        parent_bad += replay(calls, ParentRule()) is not None
    assert parent_bad > 30  # (the replay can tell the two rules apart on these sequences)


def test_clearing_plan_clears_less_than_the_block():
    """A shrink clears rows [M, earlier M) over the dirty columns, not the block."""
    rule = HookRule()
    assert rule(7, 384, 896, 256, 140, 600) == [(0, 384, 0, 896)]
    assert rule(7, 384, 896, 256, 140, 600) == [(0, 384, 600, 8)]
    assert rule(7, 384, 896, 256, 130, 600) == [(0, 384, 600, 8), (130, 10, 0, 600)]
    assert rule(7, 384, 896, 256, 140, 500) == [(0, 384, 500, 108)]
    assert rule(7, 384, 896, 256, 129, 640) == [(129, 11, 0, 512)]
    assert rule(8, 384, 896, 256, 129, 640) == [(0, 384, 0, 896)]  # another allocation
    assert rule(8, 384, 896, 128, 100, 640)[0] == (0, 384, 0, 896)  # the label rows elsewhere in the same ld


def test_clearing_plan_is_the_parent_rule_at_c5():
    """C5 (bench.py: n = 1e6, M = 2048, m = 1, the default chunk) has M a multiple of 128: three
    fits in a row get the same memsets from the rule and from its predecessor."""
    n, M, m = 1_000_000, 2048, 1
    sh = R.shapes(n, M, m, True, None)
    assert sh["chunk"] == 262144 and [c[0] for c in sh["chunks"]] == [262144] * 3 + [213568]
    new, old = HookRule(), ParentRule()
    for _ in range(3):
        for nc, _, _ in sh["chunks"]:
            a, b = new(1, sh["ld"], sh["acols"], sh["Mp"], M, nc), old(1, sh["ld"], sh["acols"], sh["Mp"], M, nc)
            assert a == b and all(r[0] == 0 and r[1] == sh["ld"] for r in a)
