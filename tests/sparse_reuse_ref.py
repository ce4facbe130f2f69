"""Scenario runner of the sparse-GP reuse tests (test_gpu_sparse_reuse.py, test_sparse_reuse_cpu.py).

The sparse GP's device state (gprx_sparse.cpp SparseNE: about eighteen grow-only buffers, two status
words and the streamed Kmn block, which is cleared only where the clearing plan of sparse_plan.cpp
says so) lives in the context and survives from call to call; every SparseGaussianProcess of a
process and every step of a sparse hyper-parameter search share it.  The runner drives ONE context
through a table of calls and compares what each call returns

* with a TWIN, bit for bit: the same single call on a fresh context, closed afterwards (the VALU
  gradient sums with atomics and is compared at 1e-12, the bound test_sparse_lml_vs_oracle uses);
* with the CPU oracle at tests.helpers.TOL, unchanged (1e-6 fp64, 1e-3 fp32).  A tree with a Matern
  leaf, which the oracle does not know, is compared with the same quantities from numpy.

The table is plain data: the CPU test walks it without a GPU (conditioning of every step, a numpy
context with planted defects, the clearing plan replayed on a mask).
"""
import os

import numpy as np

from oracle import oracle as O
from tests import matern_ref
from tests.helpers import make_data, relerr, TOL
from tests.lifecycle_ref import C3, G, GW, INDEF, RQ

PP = "SumKernel(PeriodicKernel(0.3,2.2,0.7,),PeriodicKernel(0.1,3.141592653589793,1,))"
MAT = "Matern52Kernel(0.8,1.1,)"
G2 = "GaussianKernel(0.9,1.1,)"  # G's tree with other parameters
VALU = (GW, PP)  # a White leaf / two periodic leaves: the VALU build and the atomically summed gradient

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
ERR_NONFINITE, ERR_NOT_SPD, ERR_ARG = 1, 2, 8
CHUNK_ENV = "GPRX_SPARSE_CHUNK"


# ---------------------------------------------------------------------------------------
# the step table
# ---------------------------------------------------------------------------------------
def _defaults(op, dtype, sigma, jitter):
    """fp64: sigma 0.5, jitter 1e-2; fp32: the suite's fp32 configuration (test_gpu_sparse.py,
    test_gpu_sparse_lml.py CASES: G, jitter 0.5, sigma 5.0 for the fit and 2.0 for the LML)."""
    if np.dtype(dtype) == F64:
        return (0.5 if sigma is None else sigma), (1e-2 if jitter is None else jitter)
    return ((5.0 if op == "fit" else 2.0) if sigma is None else sigma), (0.5 if jitter is None else jitter)


def fit(n, d, M, m, ks, dtype=F64, sigma=None, jitter=None, chunk=None, seed=0, device=False):
    """device: X, Y and the three results as DeviceArrays (resident in HBM)."""
    sigma, jitter = _defaults("fit", dtype, sigma, jitter)
    return dict(op="fit", n=n, d=d, M=M, m=m, ks=ks, dtype=np.dtype(dtype), sigma=sigma, jitter=jitter, chunk=chunk,
                seed=seed, device=device, raises=None, nan_row=None)


def lml(n, d, M, ks, dtype=F64, sigma=None, jitter=None, chunk=None, seed=0, grad=True, compat=False):
    sigma, jitter = _defaults("lml", dtype, sigma, jitter)
    return dict(op="lml", n=n, d=d, M=M, m=1, ks=ks, dtype=np.dtype(dtype), sigma=sigma, jitter=jitter, chunk=chunk,
                seed=seed, grad=grad, compat=compat, raises=None, nan_row=None)


def fails(status, step, nan_row=None):
    """The call `step` must raise GprxError with that status; nan_row: that row of X gets one NaN."""
    return dict(step, raises=status, nan_row=nan_row)


def _fits(Ms, ks, n=600, d=8, m=1, chunk=None, **kw):
    return [fit(n, d, Mi, m, ks, chunk=chunk, seed=i, **kw) for i, Mi in enumerate(Ms)]


SCENARIOS = {
    # shrink: fewer inducing points on the same 128-padded layout, and back (rows [M, Mp) of the
    # block keep the earlier call's K(Z, x) unless they are cleared)
    "shrink_g": _fits((140, 130, 140, 128, 129), G),                 # MFMA build, K Y fused
    "shrink_gw": _fits((140, 130, 140, 128, 129), GW, chunk=256),    # VALU build, three chunks
    "shrink_small": _fits((40, 33, 40), C3, d=3),                    # below one tile
    "shrink_lml": [fit(600, 8, 140, 1, G, seed=0), lml(600, 8, 130, G, seed=1), lml(600, 8, 140, G, seed=2),
                   fit(600, 8, 130, 1, G, seed=3), lml(600, 8, 129, GW, seed=4), fit(600, 8, 128, 1, GW, seed=5)],
    # rows: a longer chunk, then a shorter one (n 600 -> 1300 -> 600: split-K partials and a ragged
    # second chunk at 1300), the chunk size changing on identical data, the same layout at two n
    "rows": [fit(600, 8, 130, 1, G, chunk=1024, seed=0), fit(1300, 8, 130, 1, G, chunk=1024, seed=1),
             fit(600, 8, 130, 1, G, chunk=1024, seed=2),
             fit(600, 8, 130, 1, G, chunk=256, seed=3), fit(600, 8, 130, 1, G, seed=3),
             fit(600, 8, 130, 1, G, chunk=256, seed=3),
             fit(1300, 8, 130, 3, GW, chunk=256, seed=4), fit(600, 8, 130, 3, GW, chunk=256, seed=5)],
    # labels: the fused K Y epilogue <-> label rows in the block; then label rows written where the
    # fused call left the old ones
    "labels": [fit(600, 8, 130, 1, G, seed=0), fit(600, 8, 130, 3, G, seed=1), fit(600, 8, 130, 1, G, seed=2),
               fit(600, 8, 130, 1, GW, seed=3), fit(600, 8, 130, 3, GW, seed=4), fit(600, 8, 130, 1, C3, seed=5)],
    # kernels: other feature columns, MFMA <-> VALU builds, the tree uploaded when it changes (at
    # last the same tree with new parameters)
    "kernels": [fit(600, 8, 130, 1, ks, seed=i) for i, ks in enumerate((G, C3, PP, RQ, MAT, GW, G, G2))],
    "dims": [fit(600, 8, 130, 1, C3, seed=0), fit(600, 33, 130, 1, C3, seed=1), fit(600, 3, 130, 1, C3, seed=2),
             fit(600, 33, 130, 1, PP, seed=3), fit(600, 3, 40, 1, PP, seed=4)],
    # types: the two states are separate; the tile engine, the stream and the scratch are shared
    "types": [fit(600, 8, 140, 1, G, seed=0), fit(600, 8, 130, 1, G, F32, seed=1), fit(600, 8, 130, 1, G, seed=2),
              fit(600, 8, 140, 1, G, F32, seed=3), lml(600, 8, 130, G, F32, seed=4), lml(600, 8, 140, G, seed=5),
              fit(600, 8, 128, 3, G, F32, seed=6)],
    # modes: fit, the likelihood with and without its gradient, the compat value, device-resident
    # inputs and outputs between host-array calls, at two M
    "modes": [fit(600, 8, 140, 1, C3, seed=0), lml(600, 8, 130, C3, seed=1), lml(600, 8, 140, C3, seed=2, grad=False),
              lml(600, 8, 130, C3, seed=3, compat=True), fit(600, 8, 140, 1, C3, seed=4, device=True),
              fit(600, 8, 130, 1, C3, seed=5), lml(600, 8, 140, GW, seed=6), fit(600, 8, 130, 3, C3, seed=7, device=True)],
    # failures: a call that raises (the library's ordinary error returns), then good calls at the
    # same shapes and at a smaller M.  sigma = 0 raises before anything is touched; a NaN in X
    # raises after the block has been dirtied with NaNs.  (lifecycle_ref's indefinite INDEF kernel
    # leaves S positive definite at these shapes -- sigma^-2 Kmn Knm dominates, smallest eigenvalue
    # = the jitter; test_sparse_reuse_cpu.py -- so there is no NOT_SPD step.)
    "failures": [fit(600, 8, 140, 1, G, seed=0),
                 fails(ERR_ARG, fit(600, 8, 140, 1, G, sigma=0.0, seed=1)),
                 fit(600, 8, 140, 1, G, seed=1),
                 fails(ERR_NONFINITE, fit(600, 8, 140, 1, G, seed=2), nan_row=77),
                 fit(600, 8, 140, 1, G, seed=3), fit(600, 8, 130, 1, G, seed=4),
                 fit(600, 8, 129, 1, GW, seed=5)],
}


def all_steps():
    return [(name, i, st) for name, steps in SCENARIOS.items() for i, st in enumerate(steps)]


# ---------------------------------------------------------------------------------------
# inputs and references (computed once per distinct step, read-only)
# ---------------------------------------------------------------------------------------
_inputs, _refs = {}, {}


def inputs(st):
    """(X, Y, Xm) of a step in its dtype: make_data(n, d, m) shifted by 1e-3 * seed, inducing points
    X[:: n // M][:M] (taken before the NaN of a failing step is planted)."""
    key = (st["n"], st["d"], st["M"], st["m"], st["dtype"].name, st["seed"], st["nan_row"])
    if key not in _inputs:
        n, M = st["n"], st["M"]
        X, Y = make_data(n, st["d"], st["m"])
        X = X + 1e-3 * st["seed"]
        Xm = X[:: n // M][:M].copy()
        if st["nan_row"] is not None:
            assert st["nan_row"] % (n // M) != 0, "the NaN row must not be an inducing point"
            X[st["nan_row"], 1] = np.nan
        out = tuple(np.ascontiguousarray(a, st["dtype"]) for a in (X, Y, Xm))
        for a in out:
            a.setflags(write=False)
        _inputs[key] = out
    return _inputs[key]


def numpy_sparse_fit(ks, X, Y, Xm, sigma, jitter, hp=np.longdouble):
    """(Kinv, RV, RM, S, K) with S = Kmm + jitter I + sigma^-2 Kmn Knm assembled in `hp` from the fp64
    kernel values of tests/matern_ref.py, solved directly in fp64."""
    X, Y, Xm = (np.asarray(a, np.float64) for a in (X, Y, Xm))
    Kmn = matern_ref.cross(ks, Xm, X).astype(hp)
    K = matern_ref.cross(ks, Xm, Xm) + jitter * np.eye(Xm.shape[0])
    is2 = hp(1) / (hp(sigma) * hp(sigma))
    S = (K.astype(hp) + is2 * (Kmn @ Kmn.T)).astype(np.float64)
    b = (is2 * (Kmn @ Y.astype(hp))).astype(np.float64)
    return np.linalg.inv(K), np.linalg.solve(S, b), np.linalg.inv(S), S, K


def reference(st):
    """fit: (Kinv, RV, RM); lml: (value, grad, logdet) -- the oracle's, in the step's dtype."""
    key = (st["op"], st["n"], st["d"], st["M"], st["m"], st["ks"], st["dtype"].name, st["sigma"], st["jitter"],
           st["seed"])
    if key not in _refs:
        X, Y, Xm = inputs(st)
        if st["op"] == "fit":
            if "Matern" in st["ks"]:
                out = numpy_sparse_fit(st["ks"], X, Y, Xm, st["sigma"], st["jitter"])[:3]
            else:
                out = O.sparse_fit(st["ks"], X, Y, Xm, st["sigma"], st["jitter"], st["dtype"])
        else:
            v, g, _, ld = O.sparse_lml(st["ks"], X, Y[:, 0], Xm, st["sigma"], st["jitter"], st["dtype"])
            out = (float(v), np.asarray(g, np.float64), float(ld))
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


# ---------------------------------------------------------------------------------------
# the library's shapes, restated (gprx_sparse.cpp sparse_normal_eq)
# ---------------------------------------------------------------------------------------
def _up(x, a):
    return -(-x // a) * a


def shapes(n, M, m, mma, chunk_env=None, ncu=256):
    """What one call does to the streamed block: its layout (ld x acols, Mp), whether K Y is fused
    (no label rows), and per chunk (nc, rows the accumulation reads, columns it reads)."""
    Mp, mp = _up(M, 128), _up(m, 128)
    ld = Mp + mp
    cmax = 262144 if chunk_env is None else max(64, _up(int(chunk_env), 64))
    chunk = max(64, min(_up(max(n, 1), 64), cmax))
    fused = bool(mma) and m == 1
    ntiles = (Mp // 128) * (Mp // 128 + 1) // 2 + (0 if fused else (mp // 128) * (Mp // 128))
    slots, P, best = max(1, ncu), 1, 0.0
    for p in range(1, 17):
        if p > 1 and _up((_up(chunk, 16) + p - 1) // p, 16) < 256:
            break
        wg = ntiles * p
        eff = wg / (-(-wg // slots) * slots)
        if eff > best + 1e-9:
            best, P = eff, p
    chunks = []
    for off in range(0, n, chunk):
        nc = min(chunk, n - off)
        ncp = _up(nc, 16)
        kpart = _up((ncp + P - 1) // P, 16)
        Pc = (ncp + kpart - 1) // kpart
        chunks.append((nc, Mp if fused else ld, Pc * kpart))
    return dict(Mp=Mp, mp=mp, ld=ld, acols=chunk + 256, chunk=chunk, fused=fused, P=P, chunks=chunks)


# ---------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    def __init__(self, scenario, step, kind, what):
        super().__init__(f"scenario {scenario!r}, step {step}: {kind}: {what}")
        self.scenario, self.step, self.kind = scenario, step, kind


def call(ctx, st):
    """One step's call on ctx -> fit: (Kinv, RV, RM); lml: (value, grad | None, logdet)."""
    X, Y, Xm = inputs(st)
    if st["op"] == "lml":
        return ctx.sparse_lml(st["ks"], X, Y[:, 0], Xm, st["sigma"], st["jitter"], st["dtype"], grad=st["grad"],
                              compat=st["compat"])
    if st["device"] and hasattr(ctx, "device_array"):
        import gpr_amd
        M, m = st["M"], st["m"]
        Xd, Yd = ctx.device_array(X), ctx.device_array(Y)
        outs = tuple(gpr_amd.DeviceArray.empty(ctx, shp, st["dtype"]) for shp in ((M, M), (M, m), (M, M)))
        try:
            ctx.sparse_fit(st["ks"], Xd, Yd, Xm, st["sigma"], st["jitter"], st["dtype"], out=outs)
            return tuple(o.numpy() for o in outs)
        finally:
            for a in (Xd, Yd) + outs:
                a.free()
    return ctx.sparse_fit(st["ks"], X, Y, Xm, st["sigma"], st["jitter"], st["dtype"])


def _attempt(ctx, st):
    """(result, None) or (None, status of the error the call raised)."""
    try:
        return call(ctx, st), None
    except Exception as e:  # GprxError, or the numpy context's error of the same shape
        if not hasattr(e, "status"):
            raise
        return None, e.status


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def compare_twin(st, got, twin):
    """The names of what differs between a call's results on the reused and on the fresh context."""
    bad = []
    if st["op"] == "fit":
        bad = [k for k, a, b in zip(("Kinv", "RV", "RM"), got, twin) if not _same(np.asarray(a), np.asarray(b))]
    else:
        (v, g, ld), (tv, tg, tld) = got, twin
        bad = [k for k, a, b in (("value", v, tv), ("logdet", ld, tld)) if not a == b]
        if st["grad"]:
            g, tg = np.asarray(g), np.asarray(tg)
            if st["ks"] in VALU:  # summed with atomics: last-bit differences between any two runs
                ok = g.shape == tg.shape and relerr(g, tg) <= 1e-12
            else:
                ok = _same(g, tg)
            if not ok:
                bad.append("grad")
        elif g is not None or tg is not None:
            bad.append("grad")
    return bad


def compare_reference(st, got):
    """(name, figure, bound) of every comparison with the oracle that misses tests.helpers.TOL."""
    tol = TOL[st["dtype"]]
    ref = reference(st)
    bad = []
    if st["op"] == "fit":
        for k, a, r in zip(("Kinv", "RV", "RM"), got, ref):
            e = relerr(a, r)
            if not e <= tol:
                bad.append((k, e, tol))
    else:
        (v, g, ld), (vr, gr, ldr) = got, ref
        for k, a, r in (("value", v, vr), ("logdet", ld, ldr)):
            if not abs(a - r) <= tol * max(1.0, abs(r)):
                bad.append((k, abs(a - r), tol * max(1.0, abs(r))))
        if st["grad"]:
            e = relerr(g, gr) if np.shape(g) == np.shape(gr) else np.inf
            if not e <= tol:
                bad.append(("grad", e, tol))
    return bad


def collect(ctx, names):
    """{"<scenario>/<step>/<read>": array} of the named scenarios' calls, made on ctx in order with
    nothing compared (tests/poison_ref.py: a reused sparse state under GPRX_POISON)."""
    saved = os.environ.get(CHUNK_ENV)
    out = {}
    try:
        for name in names:
            for i, st in enumerate(SCENARIOS[name]):
                assert st["raises"] is None
                if st["chunk"] is None:
                    os.environ.pop(CHUNK_ENV, None)
                else:
                    os.environ[CHUNK_ENV] = str(st["chunk"])
                got = call(ctx, st)
                if st["op"] == "lml":
                    got = (np.asarray([got[0], got[2]]),) + ((np.asarray(got[1]),) if st["grad"] else ())
                for k, a in enumerate(got):
                    out[f"{name}/{i}/{k}"] = np.asarray(a)
    finally:
        if saved is None:
            os.environ.pop(CHUNK_ENV, None)
        else:
            os.environ[CHUNK_ENV] = saved
    return out


def run(name, factory, steps=None, verbose=False):
    """Drive one context from factory() through the scenario; after every step compare the call's
    results with a twin's (the same call on a fresh factory() context, closed afterwards) and with
    the oracle.  Raises Mismatch at the first step that differs.  GPRX_SPARSE_CHUNK is set or
    removed per step and restored at the end."""
    steps = SCENARIOS[name] if steps is None else steps
    saved = os.environ.get(CHUNK_ENV)
    shared = factory()
    try:
        for i, st in enumerate(steps):
            if st["chunk"] is None:
                os.environ.pop(CHUNK_ENV, None)
            else:
                os.environ[CHUNK_ENV] = str(st["chunk"])
            got, err = _attempt(shared, st)
            fresh = factory()
            try:
                twin, terr = _attempt(fresh, st)
            finally:
                fresh.close()
            if st["raises"] is not None:
                if err != st["raises"]:
                    raise Mismatch(name, i, "status", f"the reused context gave {err}, not {st['raises']}")
                if terr != st["raises"]:
                    raise Mismatch(name, i, "status", f"the fresh context gave {terr}, not {st['raises']}")
                continue
            if terr is not None:
                raise Mismatch(name, i, "twin", f"the call fails on a fresh context (status {terr})")
            if err is not None:
                raise Mismatch(name, i, "twin", f"the call fails on the reused context alone (status {err})")
            bad = compare_twin(st, got, twin)
            if bad:
                raise Mismatch(name, i, "twin", f"{bad} differ from the fresh context's bits")
            bad = compare_reference(st, got)
            if verbose or bad:
                print(f"{name}[{i}] {st['op']} M={st['M']} n={st['n']}: misses {bad}")
            if bad:
                raise Mismatch(name, i, "oracle", str(bad))
    finally:
        shared.close()
        if saved is None:
            os.environ.pop(CHUNK_ENV, None)
        else:
            os.environ[CHUNK_ENV] = saved
