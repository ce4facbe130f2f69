"""Timings that go with the Matern leaf kernels; prints one JSON line per leg.

  predict   the C3 tree's mean prediction at Q = 65536 (predict_mma_kernel<double, 1, true>, which
            must not move: the Matern branches live in the _m kernel forms only).  Device ms of
            the predict class from the library's own event timing, and host wall ms.
  build     the stand-alone MFMA build at N = 16384, d = 32 (build_time, path 1) for Matern 3/2,
            Matern 5/2 and a RationalQuadratic leaf with alpha != 1, the nearest existing leaf.
  fit       the fit at C2's shape (N = 4096, d = 16) with the Matern-3/2 device leaf, against the
            same kernel through the caller-evaluated route (numpy K included in the wall time).

python scripts/matern_perf.py [legs...]   (default: all three)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gpr_amd  # noqa: E402
from gpr_amd.synth import C2, C3, make_data, make_queries  # noqa: E402


def _model(ctx, kernel, X, Y, sigma):
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X, Y)
    M.set_kernel(kernel)
    M.set_noise(sigma)
    return M


def leg_predict(ctx, reps=7):
    X, Y = make_data(C3["n"], C3["d"], C3["m"])
    Xq = make_queries(65536, C3["d"])
    M = _model(ctx, C3["kernel"], X, Y, C3["sigma"])
    M.fit()
    M.predict(Xq)
    M.predict(Xq)
    wall, dev = [], []
    for _ in range(reps):
        ctx.set_stats(True)
        t = time.perf_counter()
        M.predict(Xq)
        wall.append(1e3 * (time.perf_counter() - t))
        st = ctx.stats()
        ctx.set_stats(False)
        dev.append(sum(v["ms"] for k, v in st.items() if "predict" in k.lower()))
    M.close()
    return dict(leg="predict", tree="C3", q=65536, n=C3["n"], device_ms=[round(v, 4) for v in dev],
                wall_ms=[round(v, 3) for v in wall], device_ms_min=round(min(dev), 4), wall_ms_min=round(min(wall), 3))


def leg_build(ctx):
    X, _ = make_data(16384, 32)
    out = {}
    for name, ks in [("m32", "Matern32Kernel(2,1,)"), ("m52", "Matern52Kernel(2,1,)"),
                     ("rq_alpha1.5", "RationalQuadraticKernel(1,2,1.5,)"), ("gauss", "GaussianKernel(2,1,)")]:
        ctx.build_time(ks, X, 1.0, path=1, iters=2)
        out[name] = [round(ctx.build_time(ks, X, 1.0, path=1, iters=5), 4) for _ in range(3)]
    return dict(leg="build", n=16384, d=32, path=1, ms=out)


class HostMatern32:
    """Matern 3/2 evaluated by the caller in numpy (the route before the device leaf)."""

    def __init__(self, l, s):
        self.l, self.s = l, s

    def __call__(self, A, B):
        r2 = np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * A @ B.T, 0.0)
        a = np.sqrt(3.0 * r2) / self.l
        return self.s ** 2 * (1 + a) * np.exp(-a)


def leg_fit(ctx, reps=3):
    X, Y = make_data(C2["n"], C2["d"], C2["m"])
    out = {}
    for name, k in [("device_leaf", "Matern32Kernel(1,1,)"), ("host_route", HostMatern32(1.0, 1.0))]:
        try:
            ts = []
            for _ in range(reps + 1):
                t = time.perf_counter()
                M = _model(ctx, k, X, Y, C2["sigma"])
                M.fit()
                a = M.alpha()
                ts.append(1e3 * (time.perf_counter() - t))
                M.close()
            out[name] = dict(wall_ms=[round(v, 2) for v in ts[1:]], alpha_absmax=float(np.max(np.abs(a))))
        except Exception as e:  # (the device leaf does not exist in a library from before it)
            out[name] = dict(error=str(e)[:80])
    return dict(leg="fit", n=C2["n"], d=C2["d"], **out)


def main():
    legs = sys.argv[1:] or ["predict", "build", "fit"]
    ctx = gpr_amd.Context(0)
    try:
        for leg in legs:
            print(json.dumps({"predict": leg_predict, "build": leg_build, "fit": leg_fit}[leg](ctx)), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
