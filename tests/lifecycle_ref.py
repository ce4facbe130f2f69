"""Scenario runner of the model-lifecycle tests (test_gpu_lifecycle.py, test_lifecycle_cpu.py).

A gprx_model is long-lived and every real caller reuses it: hyperparameter loops, appends,
re-initialisation after new data.  Behind it sit grow-only device buffers whose layout changes
from call to call and a dozen state flags.  The runner drives ONE model through a table of steps
and, after every step that leaves it fitted, compares a fixed list of reads (`observe`)

* with the same reads of a TWIN, bit for bit: a fresh model on the same context that is given
  only what defines the state -- the current data, kernel and noise, the last refitting call
  (fit(flags) / lml(grad); both refactor from scratch) and the appends made after it.  The twin
  makes none of the earlier calls and none of the earlier queries;
* with the CPU oracle at the suite's tolerances (tests/helpers.TOL, and the log-det and
  covariance forms of test_gpu_parity.py::test_fit_predict / test_posterior_cov_and_core).

Nothing here is looser than bit equality against the twin: an append step's twin makes the same
prefix fit and the same appends, so it runs the same launches on the same shapes.

The step table is plain data, so the CPU test can walk it without a model (`fitted_states`).
"""
import functools

import numpy as np

from gpr_amd import gprx
from gpr_amd.gprx import GprxError
from oracle import oracle as O
from tests.helpers import make_data, make_queries, relerr, TOL

C3 = "SumKernel(GaussianKernel(2,0.15,),PeriodicKernel(0.1,3.141592653589793,1,))"
C3B = "SumKernel(GaussianKernel(1.4,0.4,),PeriodicKernel(0.3,2.2,0.7,))"
G = "GaussianKernel(0.7,1.3,)"
RQ = "RationalQuadraticKernel(1.1,0.6,1.5,)"
GW = "SumKernel(GaussianKernel(0.8,1,),WhiteKernel(0.3,))"
PR = "ProductKernel(GaussianKernel(1.5,1,),PeriodicKernel(1,1.3,0.9,))"
INDEF = "RationalQuadraticKernel(1.2,2,-1,)"

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
CORE_MAX_N = 300  # core_matrix() is read where n <= 300
Q_BIG, Q_ONE, Q_COV = 61, 1, 40


class HostGauss:
    """The numpy Gaussian of test_gpu_hostk.py (a kernel with no device form): parameters as
    GaussianKernel(sig, sc,)."""

    def __init__(self, sig, sc):
        self.sig, self.sc = sig, sc

    def __call__(self, A, B):
        r2 = np.sum((A[:, None, :] - B[None, :, :]) ** 2, axis=-1)
        return self.sc ** 2 * np.exp(-0.5 * r2 / self.sig ** 2)


# ---------------------------------------------------------------------------------------
# the step table
# ---------------------------------------------------------------------------------------
def set_data(n, d, m, total=None, nan_row=None):
    """Rows [0, n) of make_data(total or n, d, m); nan_row: that row of X gets one NaN."""
    return dict(op="set_data", n=n, d=d, m=m, total=total or n, nan_row=nan_row, fitted=False)


def set_kernel(ks, host=None):
    """ks: the kernel string (the oracle's too); host: a callable evaluated by the caller instead."""
    return dict(op="set_kernel", ks=ks, host=host, fitted=False)


def set_noise(sigma):
    return dict(op="set_noise", sigma=sigma, fitted=False)


def fit(flags=0, method=None, raises=None, refined=False):
    """method: the FitInfo.method the step must report; raises: the GprxError status it must fail
    with (the model is then unfitted: alpha, predict and posterior_cov must all raise);
    refined: FitInfo.refine_steps >= 1."""
    return dict(op="fit", flags=flags, method=method, raises=raises, refined=refined, fitted=raises is None)


def lml(grad=True):
    return dict(op="lml", grad=grad, fitted=True)


def append(k):
    """The next k rows of the data pool (set_data's total)."""
    return dict(op="append", k=k, fitted=True)


def query(kind, q, deriv=False):
    """One big or small read between fits ('cov' / 'cov_same' / 'predict'), compared with the same
    read of a twin."""
    return dict(op="query", kind=kind, q=q, deriv=deriv, fitted=None)


def check():
    """Observe again without a model call in between (after queries)."""
    return dict(op="check", fitted=True)


def set_alpha_of_twin():
    """set_alpha(alpha of a twin fitted in the current state): predict equals the twin's bit for
    bit; the factor-based posterior_cov raises (the setters before it dropped the factor)."""
    return dict(op="set_alpha", fitted=False)


def set_sparse_cov():
    """Make a sparse GP's W resident (the model's data stand for the inducing points)."""
    return dict(op="set_sparse_cov", fitted=None)


def _b_step(n, d, m, ks):
    return [set_data(n, d, m), set_kernel(ks), fit()]


SCENARIOS = {
    # a. hyperparameter loop: noise only, same tree / new parameters, the LML layout grows by the
    # identity rows and shrinks back, nper 1 -> 0 -> 1, the VALU gradient fallback (PR)
    "a": [set_data(300, 5, 1), set_kernel(C3), set_noise(0.5), fit(),
          set_noise(0.3), fit(),
          set_kernel(C3B), fit(),
          lml(True),
          lml(False),
          fit(),
          set_kernel(G), fit(),
          set_kernel(C3), fit(),
          set_kernel(PR), lml(True), set_kernel(C3), lml(True),
          set_noise(0.5), fit()],  # (a noise change right after an inverse was formed)
    # b. shrink and grow: 6 tiles -> 2 -> 2 -> 6 -> 3 -> 3, d across 32 both ways, labels 5 -> 1 -> 17 -> 2
    "b": [set_noise(0.5)] + _b_step(700, 33, 5, GW) + _b_step(130, 2, 1, G) + _b_step(129, 1, 1, C3)
         + _b_step(700, 33, 1, C3) + [lml(True), fit()] + _b_step(300, 5, 17, G) + _b_step(257, 3, 2, RQ),
    # c. factor method changes and failures (the fixture of test_gpu_lu.py)
    "c": [set_data(260, 3, 1), set_noise(0.3), set_kernel(G), fit(method=0),
          set_kernel(INDEF), fit(method=1),
          set_kernel(G), fit(method=0),
          set_kernel(INDEF), fit(gprx.FIT_NO_LU_FALLBACK, raises=2),
          set_kernel(G), fit(method=0),
          fit(gprx.FIT_FORCE_LU, method=1), fit(method=0),
          set_data(260, 3, 1, nan_row=77), fit(raises=1),  # (the NaN shows when K is built)
          set_data(130, 3, 1), fit(method=0)],
    # d. query workspace reuse at a smaller qp, again after a refit at a smaller n
    "d": [set_data(300, 5, 1), set_kernel(C3), set_noise(0.5), fit(),
          query("cov", 300), query("cov", 5), query("predict", 300, deriv=True), query("predict", 1), check(),
          set_data(130, 5, 1), fit(),
          query("cov", 300), query("cov", 5), query("predict", 300, deriv=True), query("predict", 1), check()],
    # f. kernel route changes: device tree, caller-evaluated K, device tree, installed alpha,
    # then a sparse W that a new kernel and a dense fit must supersede
    "f": [set_data(200, 3, 1), set_noise(0.5), set_kernel(G), fit(),
          set_kernel(G, host=HostGauss(0.7, 1.3)), fit(),
          set_kernel(C3), fit(),
          set_noise(0.4), set_alpha_of_twin(),
          fit(),
          set_sparse_cov(), set_kernel(G), fit()],
    # g. fp32 refinement state
    "g": [set_data(517, 8, 3), set_kernel(G), set_noise(0.5), fit(refined=True),
          set_data(200, 2, 1), set_kernel(GW), fit(),
          fit(gprx.FIT_F32_NO_REFINE),
          fit(),
          lml(True),
          fit()],
    # h. sharded engine reuse (a virtual-rank context)
    "h": [set_kernel(C3), set_noise(0.5), set_data(700, 5, 2), fit(), set_data(260, 5, 2), fit(),
          set_data(1536, 5, 2), fit()],
    # i. the two interleaved models (test_gpu_lifecycle.py orders the calls)
    "i1": [set_data(300, 5, 1), set_kernel(C3), set_noise(0.5), fit(), check(), check()],
    "i2": [set_data(130, 2, 2), set_kernel(G), set_noise(0.5), fit(), set_data(130, 2, 1), lml(True)],
}


def scenario_e(m):
    """e. append, then something else: inside the padding, past it (the factor is re-laid), an
    LML (m = 1 only), new data, an append again."""
    return ([set_data(300, 3, m, total=431), set_kernel(C3), set_noise(0.5), fit(), append(1), append(130)]
            + ([lml(True)] if m == 1 else []) + [set_data(129, 3, m, total=132), fit(), append(3)])


SCENARIOS["e1"] = scenario_e(1)
SCENARIOS["e2"] = scenario_e(2)

SHARDED_READS = ("alpha", "pred", "cov")  # scenario h: no core matrix (it gathers a dense factor: a state change)


# ---------------------------------------------------------------------------------------
# what defines the model's state
# ---------------------------------------------------------------------------------------
class State:
    """Data, kernel, noise, the last refitting call and the appends after it."""

    def __init__(self):
        self.n = self.d = self.m = self.total = 0
        self.nan_row = None
        self.ks = None      # the kernel string (the oracle's)
        self.host = None    # the caller-evaluated form, if that is what the model holds
        self.sigma = None
        self.last = None    # ("fit", flags) | ("lml", grad)
        self.n_fit = 0      # rows the last refitting call saw
        self.appends = []
        self.fitted = False
        self.method = 0

    def pool(self, dtype=F64):
        X, Y = make_data(self.total, self.d, self.m)
        X, Y = X.astype(dtype), Y.astype(dtype)
        if self.nan_row is not None:
            X[self.nan_row, self.d // 2] = np.nan
        return X, Y

    def data(self, dtype=F64, n=None):
        X, Y = self.pool(dtype)
        n = self.n if n is None else n
        return X[:n].copy(), Y[:n].copy()

    def apply(self, step):
        op = step["op"]
        if op == "set_data":
            self.n, self.d, self.m, self.total, self.nan_row = step["n"], step["d"], step["m"], step["total"], step["nan_row"]
            self.fitted, self.last, self.appends = False, None, []
        elif op == "set_kernel":
            self.ks, self.host = step["ks"], step["host"]
            self.fitted, self.last, self.appends = False, None, []
        elif op == "set_noise":
            self.sigma = step["sigma"]
            self.fitted, self.last, self.appends = False, None, []
        elif op == "fit":
            self.last, self.n_fit, self.appends = ("fit", step["flags"]), self.n, []
            self.fitted = step["raises"] is None
            if step["method"] is not None:
                self.method = step["method"]
        elif op == "lml":
            self.last, self.n_fit, self.appends, self.fitted = ("lml", step["grad"]), self.n, [], True
        elif op == "append":
            self.appends = self.appends + [step["k"]]
            self.n += step["k"]
        elif op == "set_alpha":
            self.fitted = False

    def key(self):
        return (self.ks, self.total, self.n, self.d, self.m, self.sigma)


def fitted_states(steps):
    """(step index, step, State copy) after every step that leaves the model fitted."""
    import copy
    st = State()
    for i, step in enumerate(steps):
        st.apply(step)
        if step["fitted"]:
            yield i, step, copy.copy(st)


def kernel_plus_noise(ks, X, sigma, dtype=F64):
    """K + sigma^2 I by the oracle, in double, from inputs rounded to `dtype`."""
    X = np.asarray(X, np.float64).astype(dtype).astype(np.float64)
    return O.kernel_matrix(ks, X) + float(sigma) ** 2 * np.eye(X.shape[0])


# ---------------------------------------------------------------------------------------
# the oracle's answers (computed once per state, shared, read-only)
# ---------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def queries(d, dtype=F64):
    Xq = make_queries(Q_BIG, d).astype(dtype)
    Xa = make_queries(Q_COV, d).astype(dtype)
    return Xq, Xq[:Q_ONE].copy(), Xa, Xa[::-1].copy()


@functools.lru_cache(maxsize=None)
def oracle_fit(ks, total, n, d, m, sigma):
    X, Y = make_data(total, d, m)
    X, Y = X[:n], Y[:n]
    a_ref, C_ref = O.fit(ks, X, Y, sigma, np.float64)
    Xq, Xq1, Xa, Xb = queries(d)
    mean, D = O.predict(ks, X, a_ref, Xq, np.float64, with_deriv=True)
    out = dict(alpha=a_ref, C=C_ref, mean=mean, D=D,
               cov_same=O.posterior_cov(ks, X, C_ref, Xa, Xa), cov_rev=O.posterior_cov(ks, X, C_ref, Xa, Xb),
               kscale=max(1.0, max(abs(O.kernel_eval(ks, a, b, with_grad=False)) for a, b in zip(Xa, Xb)),
                          max(abs(O.kernel_eval(ks, a, a, with_grad=False)) for a in Xa)),
               logdet=np.linalg.slogdet(O.kernel_matrix(ks, X) + sigma * sigma * np.eye(n))[1])
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def oracle_cov_f32(ks, total, n, d, m, sigma):
    """The oracle's fp32 path (K in float, inverted in double), as
    test_posterior_variance_f32_near_training_points uses it."""
    X, Y = make_data(total, d, m)
    X32, Y32 = X[:n].astype(np.float32), Y[:n].astype(np.float32)
    _, C = O.fit(ks, X32, Y32, sigma, np.float32)
    _, _, Xa, Xb = queries(d, F32)
    return _frozen(dict(C=C, cov_same=O.posterior_cov(ks, X32, C, Xa, Xa, np.float32),
                        cov_rev=O.posterior_cov(ks, X32, C, Xa, Xb, np.float32)))


@functools.lru_cache(maxsize=None)
def oracle_lml(ks, total, n, d, sigma):
    """(value, gradient, log det) of the oracle's likelihood.  The reference narrows the determinant
    to the scalar type and clamps it (include/Likelihood.h:180-188), which the library reproduces
    only on request (LML_COMPAT); where exp(log det) leaves the double range (n = 700, d = 33) the
    clamped value says nothing about the likelihood, and the value is put together from the
    oracle's own pieces instead: -Y^T alpha / 2 - log det / 2 - n log(2 pi) / 2."""
    X, Y = make_data(total, d, 1)
    v, g, det, ld = O.lml(ks, X[:n], Y[:n], sigma)
    if not (np.isfinite(float(det)) and float(det) > np.finfo(np.float64).tiny):
        alpha = oracle_fit(ks, total, n, d, 1, sigma)["alpha"]
        v = -0.5 * float(np.sum(Y[:n] * alpha)) - 0.5 * ld - n / 2.0 * np.log(2 * np.pi)
    return v, np.asarray(g), ld


# ---------------------------------------------------------------------------------------
# observe
# ---------------------------------------------------------------------------------------
def observe(M, st, dtype, reads=None):
    """The fixed, ordered reads of a fitted model; none changes its state."""
    Xq, Xq1, Xa, Xb = queries(st.d, dtype)
    obs = {}
    if reads is None or "alpha" in reads:
        obs["alpha"] = M.alpha()
    if reads is None or "pred" in reads:
        obs["mean61"] = M.predict(Xq)           # the MFMA mean path
        obs["mean1"] = M.predict(Xq1)
        obs["mean61d"], obs["D61"] = M.predict(Xq, deriv=True)   # the VALU path
        obs["mean1d"], obs["D1"] = M.predict(Xq1, deriv=True)
    if reads is None or "cov" in reads:
        obs["cov_same"] = M.posterior_cov(Xa, Xa)
        obs["cov_rev"] = M.posterior_cov(Xa, Xb)
    if (reads is None or "core" in reads) and st.n <= CORE_MAX_N:
        obs["core"] = M.core_matrix()
    return obs


def _info_array(ret):
    """The FitInfo of a fit / append (log det, data fit, method), or an LML's value, log det, gradient."""
    if isinstance(ret, tuple):
        v, g, ld = ret
        return np.concatenate([[v, ld], np.zeros(0) if g is None else np.asarray(g, np.float64)])
    return np.array([ret.logdet, ret.datafit, float(ret.method)])


def vs_oracle(obs, info, st, dtype):
    """[(read, error, bound)] of every read that misses the oracle at the suite's tolerances."""
    bad = []
    tol = TOL[np.dtype(dtype)]
    f64 = np.dtype(dtype) == F64
    R = oracle_fit(*st.key())

    def rel(name, got, ref):
        e = relerr(got, ref)
        if not e <= tol:
            bad.append((name, e, tol))

    if "alpha" in obs:
        rel("alpha", obs["alpha"], R["alpha"])
    if "mean61" in obs:
        rel("mean61", obs["mean61"], R["mean"])
        rel("mean1", obs["mean1"], R["mean"][:Q_ONE])
        rel("mean61d", obs["mean61d"], R["mean"])
        rel("D61", obs["D61"], R["D"])
        rel("mean1d", obs["mean1d"], R["mean"][:Q_ONE])
        rel("D1", obs["D1"], R["D"][:Q_ONE])
    Rc = R if f64 else (oracle_cov_f32(*st.key()) if "cov_same" in obs or "core" in obs else None)
    for name in ("cov_same", "cov_rev"):
        if name in obs:  # a difference of O(1) terms: on the scale of k(x, y)
            e = float(np.max(np.abs(obs[name] - Rc[name])))
            if not e <= tol * R["kscale"]:
                bad.append((name, e, tol * R["kscale"]))
    if "core" in obs:
        rel("core", obs["core"], Rc["C"])
    ld_tol = 1e-8 if f64 else 1e-3
    if st.last[0] == "lml":
        vr, gr, ldr = oracle_lml(st.ks, st.total, st.n, st.d, st.sigma)
        e = abs(info[0] - vr)
        if not e <= tol * max(1.0, abs(vr)):
            bad.append(("lml value", e, tol * max(1.0, abs(vr))))
        e = abs(info[1] - ldr)
        if not e <= ld_tol * max(1.0, abs(ldr)):
            bad.append(("lml logdet", e, ld_tol * max(1.0, abs(ldr))))
        if info.size > 2:
            e = relerr(info[2:], gr)
            if not e <= tol:
                bad.append(("lml grad", e, tol))
    else:
        e = abs(info[0] - R["logdet"])
        if not e <= ld_tol * max(1.0, abs(info[0])):
            bad.append(("logdet", e, ld_tol * max(1.0, abs(info[0]))))
    return bad


# ---------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------
class Runner:
    """One reused model driven through steps.  new_model(dtype) -> a Model-like object.
    twins / oracle: make those comparisons; collect: a dict that receives every observation
    ("<step>:<read>") for a process-to-process comparison.  Mismatches go to .report as
    (step index, what, detail); .log has one line per compared step."""

    def __init__(self, new_model, dtype, reads=None, twins=True, oracle=True, collect=None, tag=""):
        self.new_model, self.dtype, self.reads = new_model, np.dtype(dtype), reads
        self.twins, self.oracle, self.collect, self.tag = twins, oracle, collect, tag
        self.M = new_model(self.dtype)
        self.st = State()
        self.info = None
        self.i = -1
        self.report = []
        self.log = []
        self.observing = True  # False: fitted steps are not observed (the caller orders the reads)

    def close(self):
        self.M.close()

    # -- the twin ----------------------------------------------------------------------
    def _setup(self, T, st, n):
        X, Y = st.data(self.dtype, n)
        T.set_data(X, Y)
        T.set_kernel(st.host if st.host is not None else st.ks)
        T.set_noise(st.sigma)

    def twin(self, fit_now=None):
        """A fresh model in the reused model's state: (model, info array of its last fitting call)."""
        st = self.st
        T = self.new_model(self.dtype)
        last = fit_now or st.last
        self._setup(T, st, st.n if fit_now else st.n_fit)
        ret = T.fit(last[1]) if last[0] == "fit" else T.lml(grad=last[1])
        if not fit_now:
            Xp, Yp = st.pool(self.dtype)
            n = st.n_fit
            for k in st.appends:
                ret = T.append(Xp[n:n + k], Yp[n:n + k])
                n += k
        return T, _info_array(ret)

    # -- one step ----------------------------------------------------------------------
    def _miss(self, what, detail=""):
        self.report.append((self.i, what, detail))

    def _must_raise(self, what, fn):
        try:
            fn()
        except GprxError:
            return
        self._miss(f"{what} answered", "expected GprxError: the model is not fitted")

    def do(self, step):
        self.i += 1
        M, st, op = self.M, self.st, step["op"]
        st.apply(step)
        if op == "set_data":
            M.set_data(*st.data(self.dtype))
        elif op == "set_kernel":
            M.set_kernel(st.host if st.host is not None else st.ks)
        elif op == "set_noise":
            M.set_noise(st.sigma)
        elif op == "fit":
            if step["raises"] is not None:
                try:
                    M.fit(step["flags"])
                    self._miss("fit did not fail", f"expected status {step['raises']}")
                except GprxError as e:
                    if e.status != step["raises"]:
                        self._miss("fit failed differently", str(e))
                Xq, _, Xa, _ = queries(st.d, self.dtype)
                self._must_raise("alpha", M.alpha)
                self._must_raise("predict", lambda: M.predict(Xq))
                self._must_raise("posterior_cov", lambda: M.posterior_cov(Xa, Xa))
            else:
                ret = M.fit(step["flags"])
                self.info = _info_array(ret)
                if step["method"] is not None and ret.method != step["method"]:
                    self._miss("method", f"{ret.method}, expected {step['method']}")
                if step["refined"] and not ret.refine_steps >= 1:
                    self._miss("refine_steps", str(ret.refine_steps))
        elif op == "lml":
            self.info = _info_array(M.lml(grad=step["grad"]))
        elif op == "append":
            Xp, Yp = st.pool(self.dtype)
            ret = M.append(Xp[st.n - step["k"]:st.n], Yp[st.n - step["k"]:st.n])
            if ret.appended != step["k"]:
                self._miss("appended", f"{ret.appended}, expected {step['k']}")
            self.info = _info_array(ret)
        elif op == "query":
            self._query(step)
        elif op == "set_alpha":
            self._set_alpha()
        elif op == "set_sparse_cov":
            n = st.n  # any symmetric W will do: a later dense fit must not answer from it
            M.set_sparse_cov((0.01 * np.eye(n) + 1e-4 * np.ones((n, n))).astype(self.dtype))
        if step["fitted"] and self.observing:
            self.compare()

    def _read(self, M, step):
        Q = make_queries(step["q"], self.st.d).astype(self.dtype)
        if step["kind"] == "predict":
            r = M.predict(Q, deriv=step["deriv"])
            return dict(zip(("mean", "D"), r)) if step["deriv"] else {"mean": r}
        return {"cov": M.posterior_cov(Q, Q[::-1].copy())}

    def _bits(self, mine, theirs, what=""):
        """Compare two dicts of arrays bit for bit; the names that differ."""
        diff = []
        for k in mine:
            if not np.array_equal(mine[k], theirs[k]):
                diff.append(k)
                self._miss(f"{what}{k} differs from the twin", f"relerr {relerr(mine[k], theirs[k]):.3e}")
        return diff

    def _query(self, step):
        mine = self._read(self.M, step)
        if self.collect is not None:
            self.collect.update({f"{self.tag}{self.i}:q:{k}": v for k, v in mine.items()})
        if self.twins:
            T, _ = self.twin()
            diff = self._bits(mine, self._read(T, step), "query ")
            T.close()
            self.log.append((self.i, f"{step['kind']} q={step['q']}", len(mine), diff))

    def _set_alpha(self):
        st = self.st
        T, _ = self.twin(fit_now=("fit", 0))
        self.M.set_alpha(T.alpha())
        mine = observe(self.M, st, self.dtype, ("pred",))
        if self.collect is not None:
            self.collect.update({f"{self.tag}{self.i}:installed:{k}": v for k, v in mine.items()})
        diff = self._bits(mine, observe(T, st, self.dtype, ("pred",)), "installed alpha: ")
        T.close()
        _, _, Xa, _ = queries(st.d, self.dtype)
        self._must_raise("posterior_cov", lambda: self.M.posterior_cov(Xa, Xa))
        self.log.append((self.i, "set_alpha", len(mine), diff))

    def compare(self):
        """observe(reused) against the twin (bits) and the oracle (tolerances)."""
        st = self.st
        obs = observe(self.M, st, self.dtype, self.reads)
        if self.collect is not None:
            self.collect.update({f"{self.tag}{self.i}:{k}": v for k, v in obs.items()})
            self.collect[f"{self.tag}{self.i}:info"] = self.info
        diff = []
        if self.twins:
            T, tinfo = self.twin()
            tobs = observe(T, st, self.dtype, self.reads)
            T.close()
            diff = self._bits(dict(obs, info=self.info), dict(tobs, info=tinfo))
        if self.oracle:
            for name, e, bound in vs_oracle(obs, self.info, st, self.dtype):
                self._miss(f"{name} misses the oracle", f"{e:.3e} > {bound:.1e}")
        self.log.append((self.i, st.last[0] + (f"+{len(st.appends)} appends" if st.appends else ""), len(obs) + 1, diff))

    def run(self, steps, stop_at_first=False):
        for step in steps:
            self.do(step)
            if stop_at_first and self.report:
                break
        return self.report

    def summary(self, name):
        nobs = sum(e[2] for e in self.log)
        nbad = sum(len(e[3]) for e in self.log)
        return (f"lifecycle {name}[{self.dtype.name}]: {len(self.log)} compared steps, {nobs} reads, "
                + ("all bit-equal to the twin" if nbad == 0 else f"{nbad} reads differ from the twin"))


def run_scenario(name, new_model, dtype, stop_at_first=False, **kw):
    """Run one table scenario on a fresh reused model; returns the Runner (report, log)."""
    r = Runner(new_model, dtype, **kw)
    try:
        r.run(SCENARIOS[name], stop_at_first)
    finally:
        r.close()
    return r


def format_report(report, steps=None):
    return "\n".join(f"step {i}{' ' + steps[i]['op'] if steps else ''}: {what} ({detail})" for i, what, detail in report)


# the scalar types each scenario runs in (test_gpu_lifecycle.py's own parametrisation)
SCENARIO_DTYPES = {"a": (F64, F32), "b": (F64, F32), "c": (F64,), "d": (F64,), "e1": (F64, F32), "e2": (F64, F32),
                   "f": (F64,), "g": (F32,), "h": (F64,), "i": (F64,)}
UNSHARDED = ("a", "b", "c", "d", "e1", "e2", "f", "g", "i")  # scenario h needs a virtual-rank context


def run_interleaved(new_model, dtype=F64, **kw):
    """Scenario i: two models share the context's scratch (ticket and counter words, cached
    schedules): fit M1, fit M2, observe M1, LML on M2 (its labels narrowed to one column first: the
    likelihood takes m = 1), observe M1, observe M2.  Returns the two (closed) Runners."""
    tag = kw.pop("tag", "")
    r1, r2 = Runner(new_model, dtype, tag=tag + "M1/", **kw), Runner(new_model, dtype, tag=tag + "M2/", **kw)
    s1, s2 = SCENARIOS["i1"], SCENARIOS["i2"]
    try:
        for step in s1[:3]:
            r1.do(step)
        for step in s2[:3]:
            r2.do(step)
        r1.observing = r2.observing = False
        r1.do(s1[3])        # fit M1
        r2.do(s2[3])        # fit M2
        r1.compare()        # observe M1
        r2.do(s2[4])
        r2.do(s2[5])        # LML on M2
        r1.compare()        # observe M1
        r2.compare()        # observe M2
    finally:
        r1.close()
        r2.close()
    return r1, r2


def collect_reused(names, new_model, dtypes=None, reads=None):
    """Every observation of the reused models of `names` (no twins, no oracle): what the poisoned
    child process and its parent compare.  dtypes: None = each scenario's own (SCENARIO_DTYPES);
    reads: as Runner's (SHARDED_READS for scenario h, whose new_model makes models of a virtual-rank
    context).  "i" is the interleaving of run_interleaved."""
    out = {}
    for name in names:
        for dt in (dtypes or SCENARIO_DTYPES[name]):
            kw = dict(reads=reads, twins=False, oracle=False, collect=out, tag=f"{name}/{np.dtype(dt).name}/")
            for r in (run_interleaved(new_model, dt, **kw) if name == "i" else [run_scenario(name, new_model, dt, **kw)]):
                assert not r.report, format_report(r.report)
    return out
