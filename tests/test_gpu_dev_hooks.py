"""gprx_dev_bench (include/gprx_dev.h): the case numbers that remain and the retired ones.

Scripts and recorded profiles refer to the cases by number.  The GEMM (1, 2), the per-block and
chained back substitutions (5, 10) and the tile factorisation (9) must still run; the numbers that
timed the removed stream-based Cholesky (0, 3, 4, 6, 7, 8) must answer GPRX_ERR_ARG like any
unknown case.  Nothing here is about speed.
"""
import ctypes
import math

import pytest

pytestmark = pytest.mark.gpu

GPRX_OK, GPRX_ERR_ARG = 0, 8
F32, F64 = 0, 1


def _bench(ctx, dt, what, M, N=0, K=0, iters=2):
    from gpr_amd.gprx import lib
    L = lib()
    L.gprx_dev_bench.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                 ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]
    ms = ctypes.c_double(float("nan"))
    st = L.gprx_dev_bench(ctx.h, dt, what, M, N, K, iters, ctypes.byref(ms))
    return st, ms.value


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("what,sizes", [(1, (256, 256, 128)), (2, (256, 256, 128)), (5, (512,)), (9, (512,)),
                                        (10, (512,))])
def test_dev_bench_live_cases(ctx, dt, what, sizes):
    st, ms = _bench(ctx, dt, what, *sizes)
    assert st == GPRX_OK
    assert math.isfinite(ms) and ms > 0


@pytest.mark.parametrize("dt", [F64, F32])
@pytest.mark.parametrize("what", [0, 3, 4, 6, 7, 8])
def test_dev_bench_retired_cases(ctx, dt, what):
    st, _ = _bench(ctx, dt, what, 512)
    assert st == GPRX_ERR_ARG
