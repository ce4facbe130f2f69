"""The narrow label row of the single-GPU tile factorisation (k_mma.h tile_mma_rows16, k_pt_ops.h
tile_gemm_rows16): with at most 16 labels the label row block's updates multiply its first 16
rows only, and the row leaves the paired updates.  Per element the narrow product runs the MFMA
steps of the full tile in the same k order before the same subtraction, so against the full-tile
form (GPRX_PT_LABEL=0) the fit's results keep their bits wherever the schedule forms the same
sums -- with the pairs off (GPRX_PT_PAIR=0).  With pairs, row nc - 1 and the label row leave the
pairs they formed (a pair subtracts C inside its accumulators, a single tile after the product:
another rounding), so there the results are compared with the oracle and against the rounding the
pairing itself introduces.

The environment is read once per process, so each form runs in a child process; the four
children run once per session and every test reads their saved results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpr_amd.synth import C3_KERNEL
from tests.helpers import make_data, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSS = "GaussianKernel(1.3,1,)"
D = 4

# (name, dtype, N, m, kernel, sigma, what) -- what: "fit", "fit32" (FIT_F32_NO_REFINE: the factor's
# own z), "lml" (value, gradient, log det), "fit3" (three fits of one model)
# f64: chunks of 1, 2 and 4 panels (N = 256, 384, 1152), a ragged last block (300), one 64-panel
# chunk plus the binary tail (8448: 66 column blocks); m = 16 is the widest narrow row, m = 17 and
# m = 130 (two label blocks) keep the full tile
UNPAIRED = ([(f"f64_{n}_{m}", "f64", n, m, C3_KERNEL, 1.0, "fit") for n in (256, 384, 1152, 300, 8448) for m in (1, 3)]
            + [(f"f64_1152_{m}", "f64", 1152, m, C3_KERNEL, 1.0, "fit") for m in (16, 17, 130)]
            + [("f64_2560_1", "f64", 2560, 1, C3_KERNEL, 1.0, "fit")]
            + [(f"f32_{n}_1", "f32", n, 1, GAUSS, 0.5, "fit32") for n in (1152, 4224)]
            + [("lml_1152", "f64", 1152, 1, C3_KERNEL, 1.0, "lml")])
PAIRED = [("f64_1152_1", "f64", 1152, 1, C3_KERNEL, 1.0, "fit"), ("f64_2560_1", "f64", 2560, 1, C3_KERNEL, 1.0, "fit3")]
# the f64 defaults pair nothing below 33 column blocks: every chunk pairs, from row j + 1, in every column
PAIR_ON = {"GPRX_PT_PAIR": "1", "GPRX_PT_PAIR_NBMIN": "1", "GPRX_PT_PAIR_TAIL": "0"}
PAIR_OFF = {"GPRX_PT_PAIR": "0"}

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpr_amd
from gpr_amd.gprx import FIT_DEFAULT, FIT_F32_NO_REFINE
from gpr_amd.synth import make_data
cases = json.loads(sys.argv[3])
ctx = gpr_amd.Context(0)
out = {}
for name, dt, n, m, ks, sigma, what in cases:
    X, Y = make_data(n, 4, m)
    M = gpr_amd.Model(ctx, np.float64 if dt == "f64" else np.float32)
    M.set_data(X, Y)
    M.set_kernel(ks)
    M.set_noise(sigma)
    if what == "lml":
        v, g, ld = M.lml(grad=True)
        out[name + ".v"], out[name + ".g"], out[name + ".ld"] = np.float64(v), np.asarray(g), np.float64(ld)
    else:
        for rep in range(3 if what == "fit3" else 1):
            info = M.fit(FIT_F32_NO_REFINE if what == "fit32" else FIT_DEFAULT)
            assert info.info >= 0, (name, info.info)
            sfx = "" if rep == 0 else f".rep{rep}"
            out[name + ".alpha" + sfx] = M.alpha()
            out[name + ".logdet" + sfx] = np.float64(info.logdet)
            out[name + ".datafit" + sfx] = np.float64(info.datafit)
    M.close()
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """results[(paired, label)]: the saved arrays of one child process per form."""
    tmp = tmp_path_factory.mktemp("label_rows")
    res = {}
    for paired in (False, True):
        for label in (1, 0):
            f = tmp / f"p{int(paired)}_l{label}.npz"
            env = dict(os.environ, GPRX_PT_LABEL=str(label), **(PAIR_ON if paired else PAIR_OFF))
            r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(f), json.dumps(PAIRED if paired else UNPAIRED)],
                               env=env, capture_output=True, text=True, timeout=240)
            assert r.returncode == 0, r.stderr[-2000:]
            res[(paired, label)] = dict(np.load(f))
    return res


@pytest.mark.parametrize("name", [c[0] for c in UNPAIRED if c[6] in ("fit", "fit32")])
def test_narrow_row_keeps_the_bits_unpaired(runs, name):
    a, b = runs[(False, 1)], runs[(False, 0)]
    for k in ("alpha", "logdet", "datafit"):
        assert np.array_equal(a[f"{name}.{k}"], b[f"{name}.{k}"]), k
    assert np.all(np.isfinite(a[name + ".alpha"]))


def test_lml_rides_on_the_same_launch(runs):
    a, b = runs[(False, 1)], runs[(False, 0)]
    for k in ("v", "g", "ld"):
        assert np.array_equal(a["lml_1152." + k], b["lml_1152." + k]), k
    assert np.isfinite(a["lml_1152.v"]) and np.all(np.isfinite(a["lml_1152.g"]))


@pytest.mark.parametrize("n", [1152, 2560])
def test_narrow_row_with_pairs(runs, n):
    """Every chunk paired: the narrow build's alpha against the oracle (the 1e-6 of
    test_gpu_configs.py), and its distance from the full-tile form no larger than the rounding the
    pairing introduces in the full-tile form itself (paired against unpaired, measured here)."""
    from oracle import oracle as O
    key = f"f64_{n}_1.alpha"
    narrow, full = runs[(True, 1)][key], runs[(True, 0)][key]
    full_unpaired = runs[(False, 0)][key]
    X, Y = make_data(n, D, 1)
    a_ref, _ = O.fit(C3_KERNEL, X, Y, 1.0, want_core=False)
    err = relerr(narrow, a_ref)
    delta = float(np.max(np.abs(narrow - full)))
    yard = float(np.max(np.abs(full - full_unpaired)))
    print(f"N={n}: alpha vs oracle {err:.3e}, |narrow - full| {delta:.3e}, pairing yardstick {yard:.3e}")
    assert err <= 1e-6
    assert delta <= yard


def test_paired_fit_repeatable(runs):
    a = runs[(True, 1)]
    for rep in (1, 2):
        for k in ("alpha", "logdet", "datafit"):
            assert np.array_equal(a[f"f64_2560_1.{k}"], a[f"f64_2560_1.{k}.rep{rep}"]), (k, rep)
