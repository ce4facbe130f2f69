"""The C++ host API (include/gpr/*.h, gpr_amd/host/) — GaussianProcess<T>, Kernel<T>,
KernelFactory<T>, Likelihood<T>, MatrixIO — driven through its two test executables
(tests/cpp/*.cpp, built by `make cpptests`).

* host_cpu_test: kernels / factory / file format on the host, and that a GaussianProcess
  throws when no GPU is visible (no CPU fallback).
* gp_host_test (-m gpu): the reference's GaussianProcessTest 1-7 and IOTest 1-3 with the
  reference's thresholds, plus a likelihood gradient consistency check, the sparse GP and
  PosteriorProcessTest 1-2 (Predict / operator() from 8 threads at once, on a fresh and on a
  loaded GP), and a user Kernel<T> subclass with no device form (host-evaluated through its
  virtual operator(), factored on the device), all running their fits on the GPU.
* pt_sched_test: not the host API but built and run the same way -- the tile schedule planner
  (gpr_amd/csrc/pt_sched.cpp) linked alone, no libgprx and no HIP runtime."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpr_amd", "lib")


def _run(exe, *args, timeout=600):
    path = os.path.join(LIB, exe)
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", ROOT, "cpptests"], check=True, timeout=900)
    r = subprocess.run([path, *args], capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("PASS", "FAIL"))]
    return r.returncode, lines, r.stdout + r.stderr


def _gpu_visible():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


def test_host_cpu():
    args = [] if _gpu_visible() else ["--no-device"]
    rc, lines, out = _run("host_cpu_test", *args)
    assert rc == 0, out
    assert len(lines) == 5 + len(args), out


def test_schedule_planner_standalone():
    """Every schedule of the frozen grid (tests/golden/make_schedule_digests.py), both precisions and
    the sharded shapes: non-empty lists, a positive makespan, sharded tickets on row blocks their rank
    owns, the split step's parts in their order (tests/cpp/pt_sched_test.cpp) -- and the figures it
    prints equal the frozen ones."""
    rc, lines, out = _run("pt_sched_test")
    assert rc == 0, out
    assert lines == ["PASS single-GPU schedules", "PASS sharded schedules"], out
    # the program is built by the host compiler, the library by hipcc: the same planner source must
    # give the frozen schedules under both (task counts and chunk width exactly, the makespan to
    # 1e-12 relative, as tests/test_schedule_frozen.py)
    import json
    from tests.golden import make_schedule_digests as G
    with open(G.FIXTURE) as f:
        frozen = json.load(f)
    got = {"single": {}, "sharded": {}}
    for l in out.splitlines():
        w = l.split()
        if w and w[0] in got:
            got[w[0]][w[1]] = w[2:]
    assert sorted(got["single"]) == sorted(frozen["single"]) and sorted(got["sharded"]) == sorted(frozen["dist"])
    for key, want in frozen["single"].items():
        n, est = got["single"][key]
        assert int(n) == want["ntasks"], key
        assert abs(float(est) - float(want["est_us"])) <= 1e-12 * float(want["est_us"]), (key, est, want["est_us"])
    for key, want in frozen["dist"].items():
        n, w, est, *ranks = got["sharded"][key]
        assert (int(n), int(w), [int(r) for r in ranks]) == (want["ntasks"], want["W"], want["rank_ntasks"]), key
        assert abs(float(est) - float(want["est_us"])) <= 1e-12 * float(want["est_us"]), (key, est, want["est_us"])


@pytest.mark.gpu
def test_host_gpu_reference_scenarios():
    rc, lines, out = _run("gp_host_test")
    assert rc == 0, out
    assert len(lines) == 21 and all(l.startswith("PASS") for l in lines), out
