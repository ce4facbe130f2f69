"""Removing samples from a fitted model (gprx_model_remove) against the full refit, at C3 and C2
(BASELINE.json configs[2], [1]).  One JSON line: per case the median of 20 calls after 3
warm-ups of the wall time of the call (host clock around a call that ends in a device
synchronise) and of its device time (the call's HIP events: build = the copied column blocks,
factor = the rotation kernel, solve = the labels' forward and back substitution).

  a  fit() of N samples
  b  remove(0, 1): every block of the factor is rotated
  c  remove(N / 2, 1): half the rows, a quarter of the triangle
  d  remove(0, 16): one pass of the widest kernel
  e  remove(0, 32), remove(0, 64), remove(0, 128): 2, 4 and 8 passes (the cut-over's candidates)
  f  one sliding-window step on N - 1 samples: append(1) + remove(0, 1)

Every call starts from a model refitted to the same size, so the sizes match from call to call.
python scripts/remove_time.py [--reps 20] [--warmup 3] [--out FILE]"""
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


def device_ms(info):
    return info.ms_build + info.ms_factor + info.ms_solve + info.ms_refine


def measure(ctx, cfg, reps, warmup):
    N, d, m = cfg["n"], cfg["d"], cfg["m"]
    dtype = np.float64 if cfg["dtype"] == "f64" else np.float32
    X, Y = make_data(N, d, m, dtype=dtype)
    M = gpr_amd.Model(ctx, dtype)
    M.set_kernel(cfg["kernel"])
    M.set_noise(cfg["sigma"])

    def run(n0, first, count, append=0):
        """medians of: fit n0 samples (untimed unless count = 0), [append], remove(first, count)."""
        wall, dev, ph = [], [], []
        for it in range(warmup + reps):
            M.set_data(X[:n0], Y[:n0])
            t0 = time.perf_counter()
            info = M.fit()
            t1 = time.perf_counter()
            dms, p = device_ms(info), (info.ms_build, info.ms_factor, info.ms_solve)
            if count:
                dms = 0.0
                t0 = time.perf_counter()
                if append:
                    ia = M.append(X[n0:n0 + append], Y[n0:n0 + append])
                    assert ia.appended == append
                    dms += device_ms(ia)
                info = M.remove(first, count)
                t1 = time.perf_counter()
                assert info.appended == -count and info.method == 0, (info.appended, info.method)
                dms += device_ms(info)
                p = (info.ms_build, info.ms_factor, info.ms_solve)
            if it >= warmup:
                wall.append(1e3 * (t1 - t0))
                dev.append(dms)
                ph.append(p)
        return {"build_factor_solve_ms": [round(statistics.median(q[i] for q in ph), 4) for i in range(3)],
                "wall_ms": round(statistics.median(wall), 4), "device_ms": round(statistics.median(dev), 4),
                "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}

    res = {
        "a_fit": run(N, 0, 0),
        "b_remove1_first": run(N, 0, 1),
        "c_remove1_middle": run(N, N // 2, 1),
        "d_remove16": run(N, 0, 16),
        "e_remove32": run(N, 0, 32),
        "e_remove64": run(N, 0, 64),
        "e_remove128": run(N, 0, 128),
        "f_slide_append1_remove1": run(N - 1, 0, 1, append=1),
    }
    # the reduced model against the refitted one, at the size timed
    M.set_data(X, Y)
    M.fit()
    M.remove(0, 1)
    a_rem = M.alpha()
    M.set_data(X[1:], Y[1:])
    M.fit()
    a_fit = M.alpha()
    res["alpha_relerr_remove_vs_fit"] = float(np.max(np.abs(a_rem - a_fit)) / np.max(np.abs(a_fit)))
    fit = res["a_fit"]["wall_ms"]
    res["fit_over_remove1"] = round(fit / res["b_remove1_first"]["wall_ms"], 2)
    res["chain_step_us_per_block"] = round(1e3 * res["b_remove1_first"]["build_factor_solve_ms"][1] / (N // 128), 3)
    res["remove1_beats_fit"] = bool(res["b_remove1_first"]["wall_ms"] < fit)
    beats = [c for c, k in [(1, "b_remove1_first"), (16, "d_remove16"), (32, "e_remove32"), (64, "e_remove64"),
                            (128, "e_remove128")] if res[k]["wall_ms"] < fit]
    res["largest_count_that_beats_fit"] = max(beats) if beats else 0
    M.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
