"""Leave-one-out cross-validation (gprx_model_loo) beside the fit and the LML gradient, at C3 and
C2 (BASELINE.json configs[2], [1]).  One JSON line: per case the median of `--reps` calls after
`--warmup` warm-ups of the wall time of the call (host clock around a call that ends in a device
synchronise and the download of its results).

  a  fit() of N samples
  b  loo() on the model a left fitted: V = L^{-T}, its rows' squared norms, the vectors
  c  loo() on an unfitted model: the fit, then b
  d  loo(grad=True) on an unfitted model: the fit with the inverse riding along, B, H = B B^T,
     the two-vector gradient pass
  e  loo(grad=True) again on the model d left: C is there, no fit
  f  lml(grad=True), which always refits

python scripts/loo_time.py [--reps 10] [--warmup 2] [--out FILE] [--configs C3,C2]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import gpr_amd
from gpr_amd.synth import C2, C3, make_data


def measure(ctx, cfg, reps, warmup):
    N, d, m = cfg["n"], cfg["d"], cfg["m"]
    dtype = np.float64 if cfg["dtype"] == "f64" else np.float32
    X, Y = make_data(N, d, m, dtype=dtype)
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X, Y)
    M.set_kernel(cfg["kernel"])

    def run(call, unfit):
        wall = []
        for it in range(warmup + reps):
            if unfit:
                M.set_noise(cfg["sigma"])  # drops the fit
            t0 = time.perf_counter()
            out = call()
            t1 = time.perf_counter()
            if it >= warmup:
                wall.append(1e3 * (t1 - t0))
        return {"wall_ms": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
                "wall_ms_max": round(max(wall), 4)}, out

    res = {}
    res["a_fit"], _ = run(M.fit, True)
    res["b_loo_values_fitted"], vals = run(M.loo, False)
    res["c_loo_values_with_fit"], _ = run(M.loo, True)
    res["d_loo_grad_with_fit"], grd = run(lambda: M.loo(grad=True), True)
    res["e_loo_grad_fitted"], _ = run(lambda: M.loo(grad=True), False)
    res["f_lml_grad"], _ = run(lambda: M.lml(grad=True), True)
    res["value_relerr_values_vs_grad_call"] = float(abs(vals[0] - grd[0]) / max(1.0, abs(grd[0])))
    res["values_fitted_cheaper_than_lml_grad"] = bool(res["b_loo_values_fitted"]["wall_ms"] < res["f_lml_grad"]["wall_ms"])
    res["loo_grad_over_lml_grad"] = round(res["d_loo_grad_with_fit"]["wall_ms"] / res["f_lml_grad"]["wall_ms"], 3)
    M.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="C3,C2")
    args = ap.parse_args()
    ctx = gpr_amd.Context(0)
    out = {"reps": args.reps, "warmup": args.warmup}
    for name in args.configs.split(","):
        cfg = {"C3": C3, "C2": C2}[name]
        out[name] = dict(n=cfg["n"], d=cfg["d"], dtype=cfg["dtype"], **measure(ctx, cfg, args.reps, args.warmup))
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
