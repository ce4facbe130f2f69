"""CPU side of the model-lifecycle tests (tests/lifecycle_ref.py, tests/test_gpu_lifecycle.py).

* The step table is sound: every fitted step's K + sigma^2 I is conditioned well inside the
  tolerances, in fp64 and from fp32-rounded inputs, so the oracle comparison cannot fail on its own.
* The runner can fail: FakeModel is a numpy model with the Model interface that keeps its state
  in 128-padded grow-only buffers, as the library does, and has switches that each plant one
  defect of the kind the GPU tests are there to catch.  With all switches off the runner passes;
  with any one on it reports a mismatch at the step where the defect first matters.
* Model.set_kernel(callable) on DeviceArray data raises instead of keeping the old kernel.
"""
import functools
import re

import numpy as np
import pytest
import scipy.linalg as sla

from gpr_amd import gprx
from gpr_amd.gprx import GprxError
from oracle import oracle as O
from tests import lifecycle_ref as L


# ---------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spectrum(ks, total, n, d, sigma, f32):
    X, _ = L.make_data(total, d, 1)
    w = np.linalg.eigvalsh(L.kernel_plus_noise(ks, X[:n], sigma, L.F32 if f32 else L.F64))
    return float(w[0]), float(np.max(np.abs(w)) / np.min(np.abs(w)))


@pytest.mark.parametrize("name", sorted(L.SCENARIOS))
def test_table_is_well_conditioned(name):
    seen = 0
    for i, step, st in L.fitted_states(L.SCENARIOS[name]):
        for f32 in (False, True):
            lo, cond = _spectrum(st.ks, st.total, st.n, st.d, st.sigma, f32)
            if st.ks == L.INDEF:
                assert lo < 0 and cond <= 1e6, (name, i, lo, cond)
            else:
                assert lo > 0 and cond <= 1e4, (name, i, lo, cond)
        if st.last[0] == "lml":
            assert st.m == 1, (name, i)
            # the oracle's long-double determinant is its slow part: n <= 300, but for the two LMLs
            # the scenarios place at larger shapes (b: 700, e: 431 after the appends; 0.3 s in the
            # oracle at n = 700)
            assert st.n <= 300 or (name, st.n) in (("b", 700), ("e1", 431)), (name, i, st.n)
        seen += 1
    assert seen >= 2


def test_twin_is_defined_by_the_last_refit():
    """The state walk the twins are built from: setters drop the fit, appends accumulate after the
    last refitting call, an LML is a refit."""
    states = {i: st for i, _, st in L.fitted_states(L.SCENARIOS["e1"])}
    ends = sorted(states)
    assert [(states[i].last[0], states[i].n_fit, states[i].appends, states[i].n) for i in ends] == [
        ("fit", 300, [], 300), ("fit", 300, [1], 301), ("fit", 300, [1, 130], 431), ("lml", 431, [], 431),
        ("fit", 129, [], 129), ("fit", 129, [3], 132)]


# ---------------------------------------------------------------------------------------
# a numpy model with the library's buffer discipline, and planted defects
# ---------------------------------------------------------------------------------------
DEFECTS = ("stale_padding", "stale_tab", "noise_keeps_inverse", "failed_fit_answers", "stale_workspace")


class GrowBuf:
    """A grow-only buffer (DevBuf): a larger request reallocates (zero-filled, as a fresh
    allocation usually is), a smaller one sees whatever the larger problem left."""

    def __init__(self):
        self.a = np.zeros(0)

    def view(self, rows, cols):
        if self.a.size < rows * cols:
            self.a = np.zeros(rows * cols)
        return self.a[:rows * cols].reshape((rows, cols), order="F")  # column-major, ld = rows


class FakeInfo:
    def __init__(self, logdet, datafit, method):
        self.logdet, self.datafit, self.method = logdet, datafit, method
        self.refine_steps, self.appended = 1, 0


def _up(x):
    return (x + 127) // 128 * 128


class FakeModel:
    """The oracle's formulas on 128-padded grow-only arrays.  defects (any of DEFECTS):
    stale_padding        a smaller problem does not clear the padding rows of the matrix buffer;
    stale_tab            a tree without periodic leaves still adds the old tree's periodic term
                         from the sin/cos table it no longer writes;
    noise_keeps_inverse  set_noise leaves inv_ready set: the core matrix is the old inverse;
    failed_fit_answers   a fit marks the model fitted before its status is known;
    stale_workspace      the query workspace is not zeroed outside the q x n block."""

    def __init__(self, dtype=np.float64, defects=()):
        assert set(defects) <= set(DEFECTS)
        self.defects = set(defects)
        self.n = self.d = self.m = 0
        self.A, self.Ra, self.Rb = GrowBuf(), GrowBuf(), GrowBuf()
        self.fitted = self.has_alpha = self.inv_ready = self.per_live = False
        self.tab = self.ks = self.sigma = None
        self.method = 0

    def close(self):
        pass

    def _unfit(self, keep_inverse=False):
        self.fitted = self.has_alpha = False
        if not keep_inverse:
            self.inv_ready = False

    def set_data(self, X, Y):
        self.X = np.array(X, np.float64)
        self.Y = np.array(Y, np.float64).reshape(len(self.X), -1)
        (self.n, self.d), self.m = self.X.shape, self.Y.shape[1]
        self._unfit()

    def set_kernel(self, ks):
        self.ks, self.nper = ks, ks.count("PeriodicKernel")
        if self.nper:
            self.per_live, self.tab_ks = True, re.search(r"PeriodicKernel\([^)]*\)", ks).group(0)
        elif "stale_tab" not in self.defects:
            self.per_live = False
        self._unfit()

    def set_noise(self, sigma):
        self.sigma = float(sigma)
        self._unfit(keep_inverse="noise_keeps_inverse" in self.defects)

    def _need(self, ok):
        if not ok:
            raise GprxError(9, "fake: model is not fitted")

    def _build(self):
        try:
            K = O.kernel_matrix(self.ks, self.X)
        except O.OracleError:  # a non-finite sample
            K = np.full((self.n, self.n), np.nan)
        if self.nper:
            self.tab = self.X.copy()  # (stands for the per-sample sin/cos tables)
        elif self.per_live and self.tab is not None and self.tab.shape[1] == self.d:
            r = min(self.n, len(self.tab))
            K[:r, :r] += O.kernel_matrix(self.tab_ks, self.tab[:r])
        return K

    def fit(self, flags=0, want_inv=False):
        n, npad = self.n, _up(self.n)
        K = self._build()
        if "failed_fit_answers" in self.defects:
            self.fitted = self.has_alpha = True
        else:
            self._unfit(keep_inverse=True)
        if not np.isfinite(K).all():
            raise GprxError(1, "fake: kernel matrix contains entries which are not finite.")
        A = self.A.view(npad, npad)
        if "stale_padding" not in self.defects:
            A[:] = 0
        A[:n, :n] = K + self.sigma ** 2 * np.eye(n)
        pad = np.arange(n, npad)
        A[pad, pad] = 1  # identity padding
        Yp = np.zeros((npad, self.m))
        Yp[:n] = self.Y
        method, Lc = (1, None) if flags & gprx.FIT_FORCE_LU else (0, None)
        if method == 0:
            try:
                Lc = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                if flags & gprx.FIT_NO_LU_FALLBACK:
                    raise GprxError(2, "fake: kernel matrix is not positive definite")
                method = 1
        if method == 0:
            alpha = sla.solve_triangular(Lc.T, sla.solve_triangular(Lc, Yp, lower=True), lower=False)
            logdet = 2 * float(np.sum(np.log(np.diag(Lc))))
        else:
            alpha = np.linalg.solve(A, Yp)
            logdet = float(np.linalg.slogdet(A)[1])
        self.Lc, self.method, self._alpha = Lc, method, alpha[:n].copy()
        if want_inv:  # the inverse rides along; later setters invalidate it
            self.C, self.inv_ready = np.linalg.inv(A)[:n, :n], True
        self.fitted = self.has_alpha = True
        return FakeInfo(logdet, float(np.sum(self.Y * self._alpha)), method)

    def lml(self, grad=True):
        if self.m != 1:
            raise GprxError(4, "fake: only one output dimension is supported")
        info = self.fit(0, want_inv=grad)
        v = -0.5 * info.datafit - 0.5 * info.logdet - self.n / 2.0 * np.log(2 * np.pi)
        g = None
        if grad:
            W = np.outer(self._alpha[:, 0], self._alpha[:, 0]) - self._core()
            g = np.array([0.5 * np.sum(W * D) for D in O.deriv_matrix(self.ks, self.X)])
        return v, g, info.logdet

    def alpha(self):
        self._need(self.has_alpha)
        return self._alpha.copy()

    def predict(self, Xq, deriv=False):
        self._need(self.has_alpha)
        mean, D = O.predict(self.ks, self.X, self._alpha, np.asarray(Xq, np.float64), with_deriv=True)
        return (mean, D) if deriv else mean

    def _core(self):
        if self.inv_ready:
            return self.C
        npad = _up(self.n)
        return np.linalg.inv(self.A.view(npad, npad))[:self.n, :self.n]

    def core_matrix(self):
        self._need(self.fitted)
        return self._core().copy()

    def _rows(self, buf, Xq, qp, npad):
        R = buf.view(qp, npad)
        if "stale_workspace" not in self.defects:
            R[:] = 0
        R[:len(Xq), :self.n] = O.cross_matrix(self.ks, Xq, self.X)
        return R

    def posterior_cov(self, Xa, Xb):
        self._need(self.fitted)
        Xa, Xb = np.asarray(Xa, np.float64), np.asarray(Xb, np.float64)
        q, qp, npad = len(Xa), _up(len(Xa)), _up(self.n)
        Ra, Rb = self._rows(self.Ra, Xa, qp, npad), self._rows(self.Rb, Xb, qp, npad)
        kab = np.array([O.kernel_eval(self.ks, a, b, with_grad=False) for a, b in zip(Xa, Xb)]).reshape(-1)
        if self.method == 0:  # the solves run over qp x npad
            Va = sla.solve_triangular(self.Lc, Ra.T, lower=True)
            Vb = sla.solve_triangular(self.Lc, Rb.T, lower=True)
            return kab - np.sum(Va * Vb, axis=0)[:q]
        return kab - np.sum(Ra.T * np.linalg.solve(self.A.view(npad, npad), Rb.T), axis=0)[:q]


def _fake(defects=()):
    return lambda dtype: FakeModel(dtype, defects)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_runner_passes_a_sound_model(name):
    r = L.run_scenario(name, _fake(), np.float64)
    assert not r.report, L.format_report(r.report, L.SCENARIOS[name])
    assert all(not e[3] for e in r.log) and len(r.log) >= 2


def _step_index(name, nth, **match):
    """Index of the nth (from 0) step of the scenario whose fields equal `match`."""
    hits = [i for i, s in enumerate(L.SCENARIOS[name]) if all(s.get(k) == v for k, v in match.items())]
    return hits[nth]


# (defect, scenario, the step where it first matters)
PLANTED = [
    ("stale_padding", "b", lambda: _step_index("b", 1, op="fit")),           # the first smaller problem: 700 -> 130
    ("stale_padding", "d", lambda: _step_index("d", 1, op="fit")),           # the refit at n = 130
    ("stale_tab", "a", lambda: _step_index("a", 0, op="set_kernel", ks=L.G) + 1),  # nper 1 -> 0
    ("noise_keeps_inverse", "a", lambda: len(L.SCENARIOS["a"]) - 1),         # set_noise after the last LML's inverse
    ("failed_fit_answers", "c", lambda: _step_index("c", 0, op="fit", raises=2)),
    ("stale_workspace", "d", lambda: _step_index("d", 0, op="query", q=5)),  # q = 5 after q = 300
]


@pytest.mark.parametrize("defect,name,where", PLANTED, ids=[f"{d}-{n}" for d, n, _ in PLANTED])
def test_runner_reports_a_planted_defect(defect, name, where):
    r = L.run_scenario(name, _fake([defect]), np.float64, stop_at_first=True)
    assert r.report, f"{defect} went unnoticed in scenario {name}"
    assert r.report[0][0] == where(), L.format_report(r.report, L.SCENARIOS[name])


def test_every_defect_is_planted_somewhere():
    assert {d for d, _, _ in PLANTED} == set(DEFECTS)


# ---------------------------------------------------------------------------------------
# Model.set_kernel(callable) with no host copy of the data
# ---------------------------------------------------------------------------------------
def _stub_model():
    M = gprx.Model.__new__(gprx.Model)  # no library, no device: the Python-side state only
    M.ctx, M.h, M.dtype = None, None, np.dtype(np.float64)
    M.n, M.d, M.m, M.kernel, M._Xh = 50, 3, 1, "old", None  # as after set_data(DeviceArray, DeviceArray)
    return M


def test_host_kernel_on_device_data_is_refused():
    M = _stub_model()
    with pytest.raises(TypeError):
        M.set_kernel(lambda A, B: np.zeros((len(A), len(B))))
    assert M.kernel == "old"


def test_device_data_under_a_host_kernel_is_refused():
    M = _stub_model()
    M.kernel = lambda A, B: np.zeros((len(A), len(B)))

    class Dev(gprx.DeviceArray):
        def __init__(self, shape):
            self.ctx, self.p, self.dtype, self._base, self.shape = None, None, np.dtype(np.float64), None, shape

    with pytest.raises(TypeError):
        M.set_data(Dev((50, 3)), Dev((50, 1)))
