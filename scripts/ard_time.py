"""The length-scale gradient (gprx_model_lml_scale_grad) beside the LML call it rides on, on an
r2-only tree at N = 16384, d = 32 (C3's Gaussian leaf and noise) and at C2's shape (BASELINE.json
configs[1]).  One JSON line: per case the median of `--reps` calls after `--warmup` warm-ups of the
wall time of the call (host clock around a call that ends in a device synchronise and the download
of its results).

  a  lml(grad=True), no length scales set: today's path (the one case a library without length
     scales can run: on such a checkout the script measures it alone)
  b  lml(grad=True) with length scales set: the same call on the scaled copy
  c  lml(grad=True, scales=True): b, then the length-scale gradient from the same fit
  d  lml_scale_grad() alone on the model c left fitted (C resident, no fit)

python scripts/ard_time.py [--reps 10] [--warmup 2] [--out FILE] [--configs R16K,C2]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import gpr_amd
from gpr_amd.synth import C2, SEED, make_data, uniform

R16K = dict(n=16384, d=32, m=1, sigma=1.0, kernel="GaussianKernel(2,0.15,)", dtype="f64")


def measure(ctx, cfg, reps, warmup):
    N, d, m = cfg["n"], cfg["d"], cfg["m"]
    dtype = np.float64 if cfg["dtype"] == "f64" else np.float32
    X, Y = make_data(N, d, m, dtype=dtype)
    ell = np.exp(np.log(0.5) + uniform(SEED + 0xA4D, d) * np.log(4.0))  # log-uniform in [0.5, 2]
    M = gpr_amd.Model(ctx, dtype)
    M.set_data(X, Y)
    M.set_kernel(cfg["kernel"])
    M.set_noise(cfg["sigma"])

    def run(call):
        wall = []
        for it in range(warmup + reps):
            t0 = time.perf_counter()
            out = call()
            t1 = time.perf_counter()
            if it >= warmup:
                wall.append(1e3 * (t1 - t0))
        return {"wall_ms": round(statistics.median(wall), 4), "wall_ms_min": round(min(wall), 4),
                "wall_ms_max": round(max(wall), 4)}, out

    res = {}
    res["a_lml_grad_no_scales"], _ = run(lambda: M.lml(grad=True))
    if hasattr(M, "set_length_scales"):
        M.set_length_scales(ell)
        res["b_lml_grad_scales_set"], _ = run(lambda: M.lml(grad=True))
        res["c_lml_grad_and_scale_grad"], both = run(lambda: M.lml(grad=True, scales=True))
        res["d_scale_grad_fitted"], alone = run(M.lml_scale_grad)
        res["scale_grad_same_bits"] = bool(np.array_equal(both[3], alone))
        res["scale_grad_share_of_call"] = round(
            (res["c_lml_grad_and_scale_grad"]["wall_ms"] - res["b_lml_grad_scales_set"]["wall_ms"])
            / res["c_lml_grad_and_scale_grad"]["wall_ms"], 4)
    M.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="R16K,C2")
    args = ap.parse_args()
    ctx = gpr_amd.Context(0)
    out = {"reps": args.reps, "warmup": args.warmup}
    for name in args.configs.split(","):
        cfg = {"R16K": R16K, "C2": C2}[name]
        out[name] = dict(n=cfg["n"], d=cfg["d"], dtype=cfg["dtype"], **measure(ctx, cfg, args.reps, args.warmup))
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
