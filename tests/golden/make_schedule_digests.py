#!/usr/bin/env python3
"""Regenerate tests/golden/schedule_digests.json: the frozen ticket lists of the tile schedule
planner (gpr_amd/csrc/pt_sched.cpp), read through the debug exports gprx_dev_schedule /
gprx_dev_schedule_list (single GPU) and gprx_dev_dist_schedule / gprx_dev_dist_schedule_list
(sharded).

For each case the fixture holds the task count, the SHA-256 of the int32 ticket array (one per rank
for the sharded cases), the chunk width W (sharded) and the simulated makespan as repr(float).  It
pins the CURRENT cost model and chunk rules: tests/test_schedule_frozen.py recomputes the same
cases and compares lists and counts exactly, the makespan to 1e-12 relative.  A change that moves
planner code must leave the file untouched; a change that retunes the cost model, a chunk rule or a
pairing rule regenerates it on purpose:

    python tests/golden/make_schedule_digests.py      # rewrites tests/golden/schedule_digests.json

The planner reads its environment once per process, so the cases are computed in a child process
whose environment has every GPRX_PT_*, GPRX_DIST_* and GPRX_TP_* variable removed (compute()).
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "schedule_digests.json")

HEADER = ("Frozen ticket lists of the tile schedule planner under its default parameters: this file pins the "
          "current cost model, chunk rules and pairing rules.  Regenerate it (tests/golden/"
          "make_schedule_digests.py) only in a change that retunes them on purpose.")

BUILD, IDENT, NARROW, F32 = 1, 2, 4, 8
INV = 2  # (sharded flags: LML mode)


def _sel(ratio=None, pair=None):
    """ratio / pair: None = the simulation's choice / the precision's default rule."""
    return (0 if ratio is None else (ratio + 1) << 8) | (0 if pair is None else (pair + 1) << 16)


# (nc, nr, P, flags): the smallest shapes that reach each branch of the single-GPU planner
SINGLE = [
    (1, 1, 256, 0), (1, 2, 256, 0), (2, 3, 256, 0),                  # smallest shapes
    (9, 10, 256, _sel(0, 0)),                                        # fixed chunk rule, no pairs
    (9, 10, 7, _sel(0, 0)),                                          # fewer workers than parts: split off
    (33, 34, 256, BUILD | _sel(2, 2)),                               # capped chunk rule with pairs
    (40, 81, 256, IDENT | _sel(0, 4)),                               # identity rows in pairs (ident_even)
    (40, 81, 256, IDENT | _sel(0, 0)),                               # identity rows single
    (70, 73, 256, BUILD | _sel(2, 4)),                               # three label row blocks
    (65, 66, 256, BUILD), (65, 66, 256, BUILD | NARROW),             # near = 0, a 64-chunk
    (32, 33, 256, BUILD),                                            # C2
    (128, 129, 256, BUILD), (128, 129, 256, BUILD | NARROW),         # C3
]
SINGLE = [c[:3] + (c[3] | f,) for c in SINGLE for f in (0, F32)]

# (nc, P, g, gb, ww, flags)
DIST = []
for _ratio in (0, 2):
    DIST += [(24, 30, g, 2, ww, BUILD | _sel(_ratio)) for g in (2, 3, 5) for ww in (2, 3, 8)]
    DIST += [(16, 30, 3, 1, 4, BUILD | INV | _sel(_ratio))]
DIST += [
    (32, 120, 2, 2, 16, BUILD | _sel(0)), (32, 120, 2, 2, 16, BUILD | _sel(2)),
    (48, 64, 2, 2, 16, BUILD | _sel(0)), (48, 64, 2, 2, 16, BUILD | INV | _sel(0)),
    (128, 256, 1, 1, 128, BUILD | _sel(0)),
    (128, 256, 8, 2, 32, BUILD | _sel(0)),
    (24, 30, 3, 2, 8, BUILD | F32 | _sel(0)), (128, 256, 8, 2, 32, BUILD | F32 | _sel(0)),
]


def _key(case):
    return ",".join(str(v) for v in case)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def _compute_here():
    """Every case through the library of this process (its environment as it is)."""
    sys.path.insert(0, ROOT)
    from gpr_amd import gprx
    L = ctypes.CDLL(gprx.LIB_PATH)
    i32, i64, dbl = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    L.gprx_dev_schedule.argtypes = [i32] * 4 + [ctypes.POINTER(dbl), ctypes.POINTER(i64)]
    L.gprx_dev_schedule_list.argtypes = [i32] * 4 + [ctypes.c_void_p, i64]
    L.gprx_dev_schedule_list.restype = i64
    L.gprx_dev_dist_schedule.argtypes = [i32] * 6 + [ctypes.POINTER(dbl), ctypes.POINTER(i32), ctypes.POINTER(i64)]
    L.gprx_dev_dist_schedule_list.argtypes = [i32] * 7 + [ctypes.c_void_p, i64]
    L.gprx_dev_dist_schedule_list.restype = i64
    single, dist = {}, {}
    for case in SINGLE:
        est, n = dbl(), i64()
        st = L.gprx_dev_schedule(*case, ctypes.byref(est), ctypes.byref(n))
        assert st == 0, (case, st)
        out = np.zeros((n.value, 4), np.int32)
        assert L.gprx_dev_schedule_list(*case, out.ctypes.data, n.value) == n.value, case
        single[_key(case)] = {"ntasks": n.value, "sha256": _digest(out), "est_us": repr(est.value)}
    for case in DIST:
        nc, P, g, gb, ww, flags = case
        est, w, n = dbl(), i32(), i64()
        st = L.gprx_dev_dist_schedule(nc, P, g, gb, ww, flags, ctypes.byref(est), ctypes.byref(w), ctypes.byref(n))
        assert st == 0, (case, st)
        counts, shas = [], []
        out = np.zeros((n.value, 4), np.int32)
        for rank in range(g):
            k = L.gprx_dev_dist_schedule_list(nc, P, g, gb, ww, flags, rank, out.ctypes.data, n.value)
            assert 0 <= k <= n.value, (case, rank, k)
            counts.append(k)
            shas.append(_digest(out[:k]))
        assert sum(counts) == n.value, case
        dist[_key(case)] = {"ntasks": n.value, "rank_ntasks": counts, "rank_sha256": shas, "W": w.value,
                            "est_us": repr(est.value)}
    return {"single": single, "dist": dist}


def compute():
    """The same, in a child process with the planner's environment variables removed."""
    env = {k: v for k, v in os.environ.items() if not k.startswith(("GPRX_PT_", "GPRX_DIST_", "GPRX_TP_"))}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--compute"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if sys.argv[1:] == ["--compute"]:
        print(json.dumps(_compute_here()))
        return
    doc = {"_header": HEADER}
    doc.update(compute())
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(doc["single"]), "single-GPU and", len(doc["dist"]), "sharded cases to", FIXTURE)


if __name__ == "__main__":
    main()
