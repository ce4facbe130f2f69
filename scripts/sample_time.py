"""The joint posterior and posterior sampling (gprx_model_posterior, gprx_model_sample) at C3
(BASELINE.json configs[2]: N = 16384, d = 32, f64) for Q query points, beside the variance call
posterior_cov(Xq, Xq) at the same Q, which runs the same cross build and row solve.  One JSON line:
per Q the median over `--reps` calls after `--warmup` warm-ups of

  wall_ms     the host clock around each call (it ends in a device synchronise and the download
              of its results);
  phases_ms   the device time of sample()'s phases, HIP events on the call's stream, recorded
              while the context's statistics are on (gprx_dev_sample_phases): cross build
              K(Xq, X), row solve R = K L^{-T}, K(Xq, Xq) and the rank update - R R^T, the
              factorisation, the normals (generator and staging), the transform (zeroing the
              upper part, the product, the mean and the output layout), for `--draws` draws.

python scripts/sample_time.py [--q 1024,4096] [--draws 64] [--reps 5] [--warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import gpr_amd
from gpr_amd.synth import C3, make_data, make_queries


def timed(call, reps, warmup, after=None):
    wall, extra = [], []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if it >= warmup:
            wall.append(1e3 * (t1 - t0))
            if after:
                extra.append(after())
    return round(statistics.median(wall), 4), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", default="1024,4096")
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=C3["n"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, d = args.n, C3["d"]
    ctx = gpr_amd.Context(0)
    X, Y = make_data(N, d, 1)
    M = gpr_amd.Model(ctx, np.float64)
    M.set_data(X, Y)
    M.set_kernel(C3["kernel"])
    M.set_noise(C3["sigma"])
    t0 = time.perf_counter()
    M.fit()
    out = {"n": N, "d": d, "dtype": "f64", "draws": args.draws, "reps": args.reps, "warmup": args.warmup,
           "fit_wall_ms": round(1e3 * (time.perf_counter() - t0), 3), "q": {}}
    for Q in (int(v) for v in args.q.split(",")):
        Xq = make_queries(Q, d)
        res = {}
        res["variance_wall_ms"], _ = timed(lambda: M.posterior_cov(Xq, Xq), args.reps, args.warmup)
        res["posterior_wall_ms"], _ = timed(lambda: M.posterior(Xq), args.reps, args.warmup)
        res["sample_wall_ms"], _ = timed(lambda: M.sample(Xq, n=args.draws, seed=1), args.reps, args.warmup)
        ctx.set_stats(True)
        jit = []
        _, ph = timed(lambda: jit.append(M.sample(Xq, n=args.draws, seed=1)[1]), args.reps, args.warmup, M.sample_phases)
        ctx.set_stats(False)
        res["phases_ms"] = {k: round(statistics.median(p[k] for p in ph), 4) for k in ph[0]}
        res["phases_total_ms"] = round(sum(res["phases_ms"].values()), 4)
        res["jitter"] = jit[-1]
        res["joint_over_variance_wall"] = round(res["posterior_wall_ms"] / res["variance_wall_ms"], 3)
        out["q"][str(Q)] = res
    M.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
