"""A reused model against a fresh one, across shapes, kernel trees, layouts and modes.

Every real caller keeps one gprx_model alive: a hyperparameter loop repeats set_kernel -> lml,
then fits and predicts; AddSample appends; new data re-initialise.  The model's ~50 grow-only
device buffers change layout from call to call (ld = np + mp, + np with the LML's inverse; the
label block with m; the sin/cos tables with nper; the features with d and the tree; the query
workspace with the last batch), everything is padded to 128, and a dozen flags carry state.  A
stale row or flag gives plausible, slightly wrong numbers that a 1e-6 parity test on a fresh
model cannot see.

tests/lifecycle_ref.py drives one model through each scenario and, after every step that leaves
it fitted, requires its reads (alpha, FitInfo, predict on both paths at q = 61 and 1, the
posterior covariance of 40 equal and 40 reversed pairs, the core matrix) to be BIT-EQUAL to those
of a twin -- a fresh model given only the current data, kernel, noise and the last refitting call
(plus the appends after it) -- and to meet the oracle at the suite's tolerances.  Every scenario
also runs in a child process with GPRX_POISON=1 (every fresh device allocation holds finite
garbage instead of the zeros a new allocation usually has) and must give the same bits.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lifecycle_ref as L

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def _models(ctx):
    import gpr_amd
    return lambda dtype: gpr_amd.Model(ctx, dtype)


def _run(name, ctx, dtype, **kw):
    r = L.run_scenario(name, _models(ctx), dtype, **kw)
    print(r.summary(name))
    assert not r.report, L.format_report(r.report, L.SCENARIOS[name])
    return r


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_hyperparameter_loop(ctx, dtype):
    """Noise only; the same tree with new parameters (the resident tree's byte comparison); the LML
    layout growing by the identity rows and shrinking back; nper 1 -> 0 -> 1; the VALU gradient."""
    _run("a", ctx, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_b_shrink_and_grow(ctx, dtype):
    """6 tiles -> 2 -> 2 -> 6 -> 3 -> 3, d across 32 in both directions, label blocks 5 -> 1 -> 17 -> 2
    wide, an LML and a plain fit at the large shape in between."""
    _run("b", ctx, dtype)


def test_c_factor_method_changes_and_failures(ctx):
    """Cholesky -> LU fallback -> Cholesky, a refused indefinite fit and a NaN sample (after either
    nothing may answer from the previous fit), a forced LU, then a smaller problem."""
    _run("c", ctx, np.float64)


def test_d_query_workspace(ctx):
    """pvRa / pvRb / pvFq and the predict scratch reused at a smaller qp, again after a refit at a
    smaller n; every query is compared with a twin that makes only that query."""
    _run("d", ctx, np.float64)


@pytest.mark.parametrize("m", [2, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_e_append_then_something_else(ctx, dtype, m):
    """An append inside the padding, one that re-lays the factor, an LML (m = 1), new data at
    n = 129 and an append again.  The twin makes the same prefix fit and the same appends."""
    _run(f"e{m}", ctx, dtype)


def test_f_kernel_route_changes(ctx):
    """Device tree -> caller-evaluated K -> device tree; an installed alpha predicts like the twin
    it came from while posterior_cov refuses; a sparse GP's W, then a new kernel and a dense fit:
    posterior_cov must answer from that fit, not from W."""
    _run("f", ctx, np.float64)


def test_g_f32_refinement_state(ctx):
    """fp32: a refined fit at (517, 8, 3), the direct-refine branch at a smaller n, an unrefined
    fit, a refined one, an LML, a fit."""
    _run("g", ctx, np.float32)


def test_h_sharded_engine_reuse():
    """One model on a two-virtual-rank context refitted at n = 700, 260, 1536; the twin is a
    fresh model on the same context."""
    import gpr_amd
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        _run("h", vctx, np.float64, reads=L.SHARDED_READS)
    finally:
        vctx.close()


def test_i_two_models_interleaved(ctx):
    """Two models share the context's scratch (ticket and counter words, cached schedules):
    fit M1, fit M2, observe M1, LML on M2 (its labels narrowed to one column first: the
    likelihood takes m = 1), observe M1, observe M2 (lifecycle_ref.run_interleaved)."""
    r1, r2 = L.run_interleaved(_models(ctx), np.float64)
    print(r1.summary("i/M1"))
    print(r2.summary("i/M2"))
    assert not r1.report, L.format_report(r1.report)
    assert not r2.report, L.format_report(r2.report)


# argv: repository root, output file, "plain" | "sharded"
_POISON_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpr_amd
from tests import lifecycle_ref as L
if sys.argv[3] == "sharded":
    ctx = gpr_amd.Context(0, virtual=2)
    out = L.collect_reused(["h"], lambda dtype: gpr_amd.Model(ctx, dtype), reads=L.SHARDED_READS)
else:
    ctx = gpr_amd.Context(0)
    out = L.collect_reused(L.UNSHARDED, lambda dtype: gpr_amd.Model(ctx, dtype))
np.savez(sys.argv[2], **out)
ctx.close()
"""

# Limits of the two children: the whole child (Python start, code-object load, schedule planning,
# the scenarios) run unpoisoned takes 0.80 s (scenarios a-g, i) and 0.52 s (scenario h), measured on
# an MI355X with the library of the commit before these tests; times four for a shared machine
# (3.2 s, 2.1 s), rounded up to half a minute (the start of a process on a busy machine varies by seconds).
POISON_CHILD_TIMEOUT_S = 30
POISON_SHARDED_CHILD_TIMEOUT_S = 30


def _digest(a):
    import hashlib
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:10]


def _poisoned_child_equals(mine, mode, tmp_path, limit):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = tmp_path / f"poisoned_{mode}.npz"
    r = subprocess.run([sys.executable, "-c", _POISON_CHILD, root, str(f), mode], env=dict(os.environ, GPRX_POISON="1"),
                       capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(f) as theirs:
        assert sorted(theirs.files) == sorted(mine)
        bad = [(k, f"relerr {L.relerr(mine[k], theirs[k]):.2e}", _digest(mine[k]), _digest(theirs[k]))
               for k in sorted(mine) if not np.array_equal(mine[k], theirs[k])]
    assert not bad, (f"{len(bad)} of {len(mine)} observations differ under GPRX_POISON "
                     f"(read, error, digest here, digest poisoned): {bad[:12]}")


def test_poisoned_buffers_give_the_same_bits(ctx, tmp_path):
    """Scenarios a to g and i (each in the scalar types of its own test above) in a child process
    with GPRX_POISON=1 (read once per process): every fresh device allocation of the library holds
    bytes 0x41 -- finite garbage, as reused memory does -- where a new allocation is usually
    zero-filled, which is what hides a read of never-written padding from the twin comparison.
    Every observation must equal this process's unpoisoned run bit for bit.
    The control words are poisoned with everything else (gprx_alloc.h): Exec::scratch_ints, the
    tile engine's counter block and the sharded engine's ctr / sctl / info / flag start as
    0x41414141, and no launch may read one before its own initialisation wrote it.  DESIGN.md 3
    ("Control words") lists, per buffer, the call that does: a memset or an init kernel on the
    launch's stream ahead of every launch, never the allocation; every wait is the bounded
    wait_until."""
    import gpr_amd
    mine = L.collect_reused(L.UNSHARDED, lambda dtype: gpr_amd.Model(ctx, dtype))
    _poisoned_child_equals(mine, "plain", tmp_path, POISON_CHILD_TIMEOUT_S)


def test_poisoned_sharded_engine_gives_the_same_bits(tmp_path):
    """Scenario h (two virtual ranks, refits at n = 700, 260, 1536; alpha, predict and the sharded
    posterior_cov) in a child of its own under GPRX_POISON=1: the ranks' storage, windows, mailboxes,
    counter and flag words and the posterior solve's partial sums all start as bytes 0x41."""
    import gpr_amd
    vctx = gpr_amd.Context(0, virtual=2)
    try:
        mine = L.collect_reused(["h"], lambda dtype: gpr_amd.Model(vctx, dtype), reads=L.SHARDED_READS)
    finally:
        vctx.close()
    _poisoned_child_equals(mine, "sharded", tmp_path, POISON_SHARDED_CHILD_TIMEOUT_S)
