"""The tile schedule planner (gpr_amd/csrc/pt_sched.cpp) against its frozen record
(tests/golden/schedule_digests.json, written by tests/golden/make_schedule_digests.py): under the
default parameters every ticket list of the recorded single-GPU and sharded cases, f64 and f32, is
reproduced exactly -- task counts and the SHA-256 of each int32 ticket array, per rank for the
sharded cases, and the chunk width -- and the simulated makespan to 1e-12 relative (a sum of at
most ~1e5 doubles in an unchanged order: the slack only covers a compiler contracting one
multiply-add differently).  The persistent kernel's deadlock-freedom argument rests on the ticket
order, so a change that only moves or restructures planner code must keep this passing with the
fixture untouched.  No device needed."""
import json

import pytest

from tests.golden import make_schedule_digests as G


@pytest.fixture(scope="module")
def frozen():
    with open(G.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    return G.compute()  # one child process, its environment cleaned of the planner's variables


def _same_est(a, b):
    a, b = float(a), float(b)
    return a > 0 and abs(a - b) <= 1e-12 * abs(b)


def test_fixture_covers_the_grid(frozen):
    assert "pins the current cost model" in frozen["_header"]
    assert sorted(frozen["single"]) == sorted(G._key(c) for c in G.SINGLE)
    assert sorted(frozen["dist"]) == sorted(G._key(c) for c in G.DIST)


@pytest.mark.parametrize("case", G.SINGLE, ids=G._key)
def test_single_gpu_schedule_frozen(case, frozen, computed):
    want, got = frozen["single"][G._key(case)], computed["single"][G._key(case)]
    assert got["ntasks"] == want["ntasks"]
    assert got["sha256"] == want["sha256"]
    assert _same_est(got["est_us"], want["est_us"]), (got["est_us"], want["est_us"])


@pytest.mark.parametrize("case", G.DIST, ids=G._key)
def test_sharded_schedule_frozen(case, frozen, computed):
    want, got = frozen["dist"][G._key(case)], computed["dist"][G._key(case)]
    assert got["ntasks"] == want["ntasks"] and got["W"] == want["W"]
    assert got["rank_ntasks"] == want["rank_ntasks"]
    assert got["rank_sha256"] == want["rank_sha256"]
    assert _same_est(got["est_us"], want["est_us"]), (got["est_us"], want["est_us"])
