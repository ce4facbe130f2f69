"""Host-side checks of the narrow label row in the tile-dataflow schedule (pt_sched.cpp
make_schedule `narrow`, flag bit 2 of gprx_dev_schedule / gprx_dev_schedule_list): the label row
block nc updates as a 16-row product, so it is never the bottom of a paired update -- row nc - 1
runs single in the columns where it was the label row's top.  Task types, the meaning of a ticket
and the deadlock-freedom argument are unchanged; with the bit clear the lists are the ones the
schedule produced before the narrow row existed.  No device needed."""
import ctypes
import hashlib

import numpy as np
import pytest

from gpr_amd.gprx import lib

NARROW = 4  # flag bit 2


def _flags(ident, ratio, pair, narrow):
    return (1 | (2 if ident else 0) | (NARROW if narrow else 0) | (0 if ratio is None else (ratio + 1) << 8)
            | (0 if pair is None else (pair + 1) << 16))


def _valid(nc, nr, flags):
    L = lib()
    L.gprx_dev_schedule.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_double),
                                                           ctypes.POINTER(ctypes.c_int64)]
    est, n = ctypes.c_double(), ctypes.c_int64()
    st = L.gprx_dev_schedule(nc, nr, 256, flags, ctypes.byref(est), ctypes.byref(n))
    return st, n.value


def _list(nc, nr, flags):
    L = lib()
    L.gprx_dev_schedule_list.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_void_p, ctypes.c_int64]
    L.gprx_dev_schedule_list.restype = ctypes.c_int64
    n = L.gprx_dev_schedule_list(nc, nr, 256, flags, None, 0)
    assert n > 0
    out = np.zeros((n, 4), np.int32)
    assert L.gprx_dev_schedule_list(nc, nr, 256, flags, out.ctypes.data, n) == n
    return out


# (nc, nr, identity rows); the rules: the fixed chunk rule with every chunk paired from row j + 1
# and from row j + 4 (the label row is then in a pair in about half the columns), and the rule and
# pairing potrf_tiles picks by itself (ratio None, pair None)
SHAPES = [(2, 3, False), (9, 10, False), (40, 41, False), (128, 129, False), (9, 19, True), (40, 81, True)]
RULES = [(0, 1), (0, 4), (None, None)]


@pytest.mark.parametrize("ratio,pair", RULES)
@pytest.mark.parametrize("nc,nr,ident", SHAPES)
def test_narrow_label_row_schedule(nc, nr, ident, ratio, pair):
    nr0 = nc + 1  # matrix rows, then the one label row block; the identity rows follow
    fl = _flags(ident, ratio, pair, True)
    st, n = _valid(nc, nr, fl)
    assert st == 0  # every producer holds an earlier ticket than its consumers
    L = _list(nc, nr, fl)
    assert len(L) == n
    typ, nb = L[:, 0] & 0xFF, L[:, 0] >> 8
    ii, jj, b0 = L[:, 1], L[:, 2], L[:, 3]
    # the label row is in no pair (the identity rows below it pair among themselves)
    p5 = typ == 5
    assert not np.any(p5 & (ii < nr0) & (ii + 1 >= nc))
    assert np.all((ii[p5] < nc - 1) | (ii[p5] >= nr0))
    # label updates stay type 2, label TRSMs type 1, one per column block
    assert {int(j) for j in jj[(typ == 1) & (ii == nc)]} == set(range(nc))
    # replay: every tile's panels exactly once, in order
    applied = {}
    for q in np.where((typ == 2) | p5)[0]:
        for r in ([ii[q]] if typ[q] == 2 else [ii[q], ii[q] + 1]):
            applied.setdefault((int(r), int(jj[q])), []).append((int(b0[q]), int(nb[q])))
    # (identity rows go in pairs (E_2s, E_2s+1), both from panel 2s)
    start = lambda r: 0 if r < nr0 else (r - nr0) - ((r - nr0) & 1)  # noqa: E731
    for (r, j), ch in applied.items():
        e = j - 1 if r == j else j
        pos = start(r)
        for b, k in ch:
            assert b == pos, (r, j, ch)
            pos += k
        assert pos == e, (r, j, ch)
    for j in range(1, nc):  # no tile is left out: matrix rows, and the label row over all j panels
        assert (nc, j) in applied
        for r in range(j, nc):
            assert ((r, j) in applied) == ((j - 1 if r == j else j) > 0)
    # ... by tickets after the producers of their operands
    final = {}
    for q in range(len(L)):
        if typ[q] == 1:
            final[(int(ii[q]), int(jj[q]))] = q
        elif typ[q] == 0:
            final[(int(ii[q]), int(ii[q]))] = q
    for q in np.where((typ == 2) | p5)[0]:
        rows = (ii[q], jj[q]) if typ[q] == 2 else (ii[q], ii[q] + 1, jj[q])
        for b in range(b0[q], b0[q] + nb[q]):
            for r in rows:
                if r >= nr0 and b < r - nr0:
                    continue  # the zero tile left of a paired odd identity row's own block
                if r < nc and b == r:
                    continue  # a diagonal tile's own panel is never an operand
                p = final.get((int(r), int(b)))
                if p is None and r == b + 1:
                    p = final.get((int(r), int(r)))  # L_{b+1,b}: published by DIAGX(b + 1)
                assert p is not None and p < q, (q, r, b)
    if ratio is not None:
        # the same chunk rule without the flag: one more ticket per pair that held the label row
        L0 = _list(nc, nr, _flags(ident, ratio, pair, False))
        t0, i0 = L0[:, 0] & 0xFF, L0[:, 1]
        held = int(((t0 == 5) & (i0 + 1 == nc)).sum())
        assert len(L) == len(L0) + held
        if nc >= 9:
            assert held > 0
        # and nothing else changed: apart from the updates of rows nc - 1 and nc the tasks are the same set

        def others(A):
            t, i = A[:, 0] & 0xFF, A[:, 1]
            drop = ((t == 5) & (i + 1 == nc)) | ((t == 2) & (i >= nc - 1) & (i <= nc))
            return sorted(map(tuple, A[~drop].tolist()))

        assert others(L) == others(L0)


# Ticket count and SHA-256 of the int32 ticket list with the flag clear, taken from the build before
# the narrow label row existed (flags: fused build, the rule below, P = 256)
PARENT = {
    (2, 3, False, 0, 1): (16, "9fcfabb3a888350a6833f49f2e4560181a6c5949b88dc1f5faa785792f674d8b"),
    (2, 3, False, 0, 4): (16, "9fcfabb3a888350a6833f49f2e4560181a6c5949b88dc1f5faa785792f674d8b"),
    (2, 3, False, None, None): (16, "9fcfabb3a888350a6833f49f2e4560181a6c5949b88dc1f5faa785792f674d8b"),
    (9, 10, False, 0, 1): (215, "baf383b1468e5774686962e3e2de625f9377bf27e6a3e6f9519f226ba4b8c114"),
    (9, 10, False, 0, 4): (236, "51448a026b7090ed503782df3af2ca66f5116c2c55f4c993c420358270ef6c65"),
    (9, 10, False, None, None): (252, "0e95329dd3f918cb88675d283654fb19ff0ab8488356adf12453539c919f8d35"),
    (40, 41, False, 0, 1): (3348, "2f2213e85091802c15904d1911b9df1662ec54e688ea0ef639f9f90698cb42d9"),
    (40, 41, False, 0, 4): (3550, "23b619799793779b30296b93e0398f792fe79a3ab2466edd0a7ce8116438a669"),
    (40, 41, False, None, None): (5145, "eba53bb2520a56d7b6ebd5565de2a0e4dfe70b692dde360d17002843e5e1c922"),
    (128, 129, False, 0, 1): (30514, "366e65782be69811235536961d61a75a1f94621151d0beae8fd0ae2b4cfde8b5"),
    (128, 129, False, 0, 4): (31141, "aa5a190338a01621960f78dc4858ae8b02d62fd42870d869b3bf4d5aae4e7ed5"),
    (128, 129, False, None, None): (36007, "497379f842f0ee8e544e7e157155efc44e57da022cc0ab237f80db374c6fe19e"),
    (9, 19, True, 0, 1): (304, "2f60418fe4b3391cca98ad54c46ee874fdbcdfe4164dcff9319c800959188bbc"),
    (9, 19, True, 0, 4): (325, "0071e4719e2aada59b10b655632264ba909fff7452170b8ff7c3575712e3c5b7"),
    (9, 19, True, None, None): (385, "a86d218c2572ff894d22867075c0365e787fcacaca2f2aad2b668af9db0c7d6f"),
    (40, 81, True, 0, 1): (5432, "a08627c9df7b538f5dd433a407ddd4675bcf2efcf8ef3ecf163f8d42a08a6f8f"),
    (40, 81, True, 0, 4): (5634, "2e542e3dc2edaf2ba892a914afa1800ff7ee91d9ad5c83ed00e634ba11e1bb3f"),
    (40, 81, True, None, None): (8071, "62c55dc17b0f9be52551007b93c6bb32c6655b283ff683c2612d0abc90dd595c"),
}


@pytest.mark.parametrize("ratio,pair", RULES)
@pytest.mark.parametrize("nc,nr,ident", SHAPES)
def test_flag_clear_reproduces_earlier_lists(nc, nr, ident, ratio, pair):
    L = _list(nc, nr, _flags(ident, ratio, pair, False))
    n, h = PARENT[(nc, nr, ident, ratio, pair)]
    assert len(L) == n
    assert hashlib.sha256(np.ascontiguousarray(L, np.int32).tobytes()).hexdigest() == h
