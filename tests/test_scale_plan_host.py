"""The launch plan of the scale() kernels (ppls_scale.hip: ppls_scale_plan) against the resident
layout (CPU only).

The column kernels address X + row * ld + unit * VE for the 16-byte units [0, units) of the rows of
their row block, and part + block * ldc + unit * VE.  Checked over a grid of shapes, from the plan the
library itself returns: every unit lies inside a row of ld_of(cols) elements (so no load or store
reaches the next row, let alone the slack), the partials' index stays below nblocks * ldc, the grid
covers every unit and row block, and the even split tiles [0, n) in order without gaps.
"""
import ctypes as ct
import itertools


class PplsScalePlan(ct.Structure):   # ppls_scale.h
    _fields_ = [("units", ct.c_int), ("ldc", ct.c_int), ("tx", ct.c_int), ("ty", ct.c_int), ("grid_x", ct.c_int),
                ("grid_y", ct.c_int), ("nblocks", ct.c_int64)]


def ld_of(p, f32, pad=1):   # ppls_capi.cpp: ld_of
    es = 4 if f32 else 8
    b = p * es
    if not pad or b < 1024 or (not f32 and p <= 2048):
        return (p + 3) & ~3 if f32 else (p + 1) & ~1
    al = 4096 if b >= 16384 else 128
    return ((b + al - 1) // al * al) // es


def _plan():
    from ppls_amd import _lib
    fn = _lib.lib().ppls_scale_plan
    fn.restype = PplsScalePlan
    fn.argtypes = [ct.c_int64, ct.c_int, ct.c_int, ct.c_int]
    return fn


def test_scale_plan_stays_inside_the_layout():
    plan = _plan()
    checked = 0
    ns = (0, 1, 2, 15, 16, 17, 40, 67, 1031, 100_000, 1_000_000, 3_000_000_000)
    cols = (1, 2, 3, 4, 5, 19, 37, 127, 128, 129, 255, 256, 257, 301, 511, 512, 513, 1023, 1025, 2000, 2100, 10_000, 100_000)
    for n, c, f32, cus in itertools.product(ns, cols, (0, 1), (0, 1, 64, 256, 304)):
        pl = plan(n, c, f32, cus)
        ve = 4 if f32 else 2
        key = (n, c, f32, cus)
        assert pl.units == (c + ve - 1) // ve and pl.ldc == pl.units * ve, key
        assert pl.ldc <= ld_of(c, f32) and pl.ldc <= ld_of(c, f32, pad=0), key     # the last unit ends inside the row
        assert c > pl.ldc - ve, key                                                 # ... and holds a real column
        assert pl.tx * pl.ty == 256 and pl.tx & (pl.tx - 1) == 0, key
        assert pl.grid_x * pl.tx >= pl.units > (pl.grid_x - 1) * pl.tx, key
        assert 1 <= pl.nblocks <= 2048 and pl.nblocks <= max(1, (n + 15) // 16), key
        assert pl.grid_y * pl.ty >= pl.nblocks > (pl.grid_y - 1) * pl.ty and pl.grid_y <= 65535, key
        prev = 0
        for b in range(pl.nblocks):                                                 # the even split
            r0, r1 = b * n // pl.nblocks, (b + 1) * n // pl.nblocks
            assert r0 == prev and r1 >= r0, key
            prev = r1
        assert prev == n, key
        again = plan(n, c, f32, cus)
        assert [getattr(again, f) for f, _ in PplsScalePlan._fields_] == [getattr(pl, f) for f, _ in PplsScalePlan._fields_]
        checked += 1
    assert checked > 2000


def test_scale_plan_of_the_benchmark_shapes():
    plan = _plan()
    c3 = plan(1_000_000, 2000, 0, 256)
    assert (c3.units, c3.tx, c3.ty, c3.grid_x, c3.nblocks) == (1000, 256, 1, 4, 512)      # 2048 workgroups
    narrow = plan(1031, 5, 0, 256)
    assert (narrow.units, narrow.tx, narrow.ty, narrow.grid_y, narrow.nblocks) == (3, 4, 64, 2, 65)   # a ragged last workgroup
