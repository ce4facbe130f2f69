"""Appending samples to a fitted model (gprx_model_append) against the full refit, at C3 and C2
(BASELINE.json configs[2], [1]).  One JSON line: per case the median of 20 calls after 3
warm-ups of the wall time of the call (host clock around a call that ends in a device
synchronise) and of its device time (the call's HIP events: build + factor + solve).

  a  fit() of N samples
  b  append of 1 sample to N - 1 fitted samples (inside the factor's padding: nothing moves)
  c  append of 1 sample to N fitted samples (N a multiple of 128: the factor is re-laid)
  d  append of 128 samples to N - 128 fitted samples (a new block: re-laid as well)
  e, f  b and d with APPEND_SOLVE_GEMM (panel solves through trsm_rows)

Every append starts from a model refitted to the same size, so the sizes match from call to
call and the result of a, b and d is a model of the same N samples.
python scripts/append_time.py [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import gpr_amd
from gpr_amd import gprx
from gpr_amd.synth import C2, C3, make_data


def device_ms(info):
    return info.ms_build + info.ms_factor + info.ms_solve + info.ms_refine


def measure(ctx, cfg, reps, warmup):
    N, d, m = cfg["n"], cfg["d"], cfg["m"]
    dtype = np.float64 if cfg["dtype"] == "f64" else np.float32
    X, Y = make_data(N + 1, d, m, dtype=dtype)
    M = gpr_amd.Model(ctx, dtype)
    M.set_kernel(cfg["kernel"])
    M.set_noise(cfg["sigma"])

    def run(n0, k, flags):
        """(wall ms, device ms) medians of: fit n0 samples (untimed unless k = 0), append k."""
        wall, dev, ph = [], [], []
        for it in range(warmup + reps):
            M.set_data(X[:n0], Y[:n0])
            t0 = time.perf_counter()
            info = M.fit()
            t1 = time.perf_counter()
            if k:
                t0 = time.perf_counter()
                info = M.append(X[n0:n0 + k], Y[n0:n0 + k], flags)
                t1 = time.perf_counter()
                assert info.appended == k and info.method == 0, (info.appended, info.method)
            if it >= warmup:
                wall.append(1e3 * (t1 - t0))
                dev.append(device_ms(info))
                ph.append((info.ms_build, info.ms_factor, info.ms_solve))
        return {"build_factor_solve_ms": [round(statistics.median(p[i] for p in ph), 4) for i in range(3)],
                "wall_ms": round(statistics.median(wall), 4), "device_ms": round(statistics.median(dev), 4),
                "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4)}

    G = gprx.APPEND_SOLVE_GEMM
    res = {
        "a_fit": run(N, 0, 0),
        "b_append1": run(N - 1, 1, 0),
        "c_append1_relayout": run(N, 1, 0),
        "d_append128": run(N - 128, 128, 0),
        "e_append1_gemm": run(N - 1, 1, G),
        "f_append128_gemm": run(N - 128, 128, G),
    }
    # the appended model against the refitted one, at the size timed
    M.set_data(X[:N - 1], Y[:N - 1])
    M.fit()
    M.append(X[N - 1:N], Y[N - 1:N])
    a_app = M.alpha()
    M.set_data(X[:N], Y[:N])
    M.fit()
    a_fit = M.alpha()
    res["alpha_relerr_append_vs_fit"] = float(np.max(np.abs(a_app - a_fit)) / np.max(np.abs(a_fit)))
    res["fit_over_append1"] = round(res["a_fit"]["wall_ms"] / res["b_append1"]["wall_ms"], 2)
    if cfg is C3:  # the acceptance figure of the append path
        res["accept_b_le_a_over_5"] = bool(res["b_append1"]["wall_ms"] <= res["a_fit"]["wall_ms"] / 5)
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
