"""The cross-product statistics pass without a GPU: plain fp64 numpy lies inside every bar of
tests/xprod_bar.py at the shapes of tests/test_gpu_xprod_matrix.py, each seeded defect falls outside the bar
of every quantity it touches (and stays inside the others), the exact case is exact in fp64, the prefix
property holds, and the launch rules restated in xprod_bar are the library's."""
import functools

import numpy as np
import pytest

import xprod_bar as xb

SHAPES = {"matrix": (301, 39, 48), "nt": (5100, 2, 64)}      # p, q, rows of D: (a) and (c) of the GPU module


@functools.lru_cache(maxsize=None)
def _case(name):
    """(padded S, W, C, coef, reference) of a shape, computed once and left unchanged."""
    p, q, rows = SHAPES[name]
    S, W, C, coef = xb.problem(p, q, rows, seed=p + q)
    ref = xb.XprodReference(S, p, q, W, C, coef)
    Sp, Wp, Cp = xb.padded(S, W, C, p, q)
    for A in (Sp, Wp, Cp, coef):
        A.setflags(write=False)
    return Sp, Wp, Cp, coef, ref


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_plain_fp64_numpy_lies_inside_every_bar(name):
    Sp, Wp, Cp, coef, ref = _case(name)
    r = ref.ratios(*xb.model(Sp, Wp, Cp, coef, ref.ldx))
    print(name, r)
    assert max(r.values()) <= 1.0, r
    assert min(r.values()) > 0.0                      # a bar, not a blanket: fp64 does err against long double
    for k in (1, 5, 8):                               # an R-form is held to the first R columns
        rk = ref.ratios(*xb.model(Sp, Wp[:, :k], Cp[:, :k], coef[:, :k], ref.ldx))
        assert max(rk.values()) <= 1.0, (k, rk)


# defect -> the quantities whose bar it must break, and those it does not reach (G sums M's rows: one
# broken row of M may or may not carry G outside, so G is in neither set there)
BREAKS = {
    "drop_pair": {"M", "SX"}, "y_offset": {"M", "SX", "SY", "G"}, "row_past_P": {"M", "SY"}, "swap_ab": {"SX"},
    "gram_wrong_side": {"G"}, "scatter_off_by_one": {"M", "SX"},
}
INSIDE = {
    "drop_pair": {"SY"}, "y_offset": set(), "row_past_P": {"SX"}, "swap_ab": {"M", "SY", "G"},
    "gram_wrong_side": {"M", "SX", "SY"}, "scatter_off_by_one": {"SY"},
}


@pytest.mark.parametrize("defect", xb.DEFECTS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_seeded_defects_lie_outside(name, defect):
    Sp, Wp, Cp, coef, ref = _case(name)
    r = ref.ratios(*xb.model(Sp, Wp, Cp, coef, ref.ldx, defect))
    print(name, defect, r)
    for k in BREAKS[defect]:
        assert r[k] > 1.0, (defect, k, r)
    for k in INSIDE[defect]:
        assert r[k] <= 1.0, (defect, k, r)


def test_exact_case_is_exact_in_fp64_and_defects_show():
    p, q = 301, 39
    S, W, C, coef = xb.exact_problem(p, q, seed=3)
    assert np.array_equal(S, S.T) and np.abs(S).max() <= 8 and np.abs(W).max() <= 4
    ldx, ldy, live = xb.layout(p, q)
    assert float((np.abs(S[:, :p]) @ np.abs(W)).max()) < 2 ** 13     # every partial sum far below 2^53
    Sp, Wp, Cp = xb.padded(S, W, C, p, q)
    for r in (1, 6, 16):
        Wr, Cr, cr = xb.first(r, Wp, Cp, coef)
        want = xb.exact_reference(S, *xb.first(r, W, C, coef), p, q)
        got = xb.model(Sp, Wr, Cr, cr, ldx)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        bad = xb.model(Sp, Wr, Cr, cr, ldx, "scatter_off_by_one")
        assert not np.array_equal(bad[0], want[0])


def test_prefix_property():
    """Column t of every output depends on column t of W, C and the coefficients only."""
    p, q, rows = SHAPES["matrix"]
    S, W, C, coef = xb.problem(p, q, rows, seed=p + q)
    ref = _case("matrix")[4]
    for r in (1, 7):
        sub = xb.XprodReference(S, p, q, *xb.first(r, W, C, coef))
        c = np.r_[np.arange(r), xb.RMAX + np.arange(r)]
        pairs = [(sub.M, ref.M[:, c]), (sub.bar_M, ref.bar_M[:, c]), (sub.SX, ref.SX[:, :r]), (sub.bar_SX, ref.bar_SX[:, :r]),
                 (sub.SY, ref.SY[:, :r]), (sub.bar_SY, ref.bar_SY[:, :r]), (sub.G, ref.G[np.ix_(c, c)]),
                 (sub.bar_G, ref.bar_G[np.ix_(c, c)])]
        for a, b in pairs:      # the long-double sums may be blocked differently by width: equal to 2^-60
            assert a.shape == b.shape and np.all(np.abs(a - b) <= 2.0 ** -60 * np.abs(b))


def test_forms_and_shape_properties():
    """The 56 forms, and the five properties the matrix shape (301, 39) was chosen for."""
    assert len(xb.FORMS) == 56 and len(set(xb.FORMS)) == 56
    assert all((r, 8) in xb.FORMS for r in range(1, 9)) and (9, 8) not in xb.FORMS
    ldx, ldy, _ = xb.layout(301, 39)
    P = ldx + ldy
    assert (ldx, ldy, P) == (302, 40, 342)
    assert ldx % 256 == 46 and ldx % 128 == 46 and ldx > 256          # a partial last X tile in both geometries
    assert ldy < 128                                                   # the Y phase is one partial tile
    for rw in (4, 8):                                                  # a wave with rows on both sides of the seam
        assert ldx % rw != 0
    assert P % 4 == 2 and P % 8 == 6                                   # the last live wave has rows past P
    for waves in (4, 8):                                               # the last workgroup has whole waves past P
        for rw in (1, 2, 4, 8):
            blocks = -(-P // (waves * rw))
            assert blocks * waves * rw - P >= rw, (waves, rw)


def test_launch_rules_are_the_librarys():
    from ppls_amd import _lib
    lib = _lib.lib()                                                   # loads without a device
    assert lib.ppls_xprod_tile_nt(5120) == 0 and lib.ppls_xprod_tile_nt(5122) == 1
    for P in (4, 342, 5118, 5120, 5122, 16000, 46340):
        assert lib.ppls_xprod_tile_nt(P) == xb.tile_nt(P), P
    cus = 256                                                          # P / 8 against 2 x num_cus: the boundary is P = 4096
    assert lib.ppls_xprod_tile_rows(4096, 5, 0, cus) == 2 and lib.ppls_xprod_tile_rows(4095, 5, 0, cus) == 1
    assert lib.ppls_xprod_tile_rows(4103, 5, 0, cus) == 2 and lib.ppls_xprod_tile_rows(4088, 5, 0, cus) == 1
    for P in (4, 342, 4094, 4096, 4098, 5122):
        for r in (1, 8, 9, 16):
            for opt in (0, 1, 2, 3, 4, 8, 16):
                for n in (1, 64, 256, 304):
                    assert lib.ppls_xprod_tile_rows(P, r, opt, n) == xb.tile_rows(P, r, opt, n), (P, r, opt, n)
    assert lib.ppls_xprod_tile_rows(342, 8, 8, cus) == 8 and lib.ppls_xprod_tile_rows(342, 9, 8, cus) == 1


def test_entry_points_are_declared():
    import os
    from conftest import ROOT
    from ppls_amd import _lib
    from ppls_amd.api import Context
    with open(os.path.join(ROOT, "include", "ppls_debug.h")) as f:
        dbg = f.read()
    for decl in ("int ppls_xprod_pass(ppls_ctx* ctx, const double* S, int P, int ldx, const double* W, const double* C,",
                 "int ppls_xprod_tile_nt(int P);", "int ppls_xprod_tile_rows(int P, int r, int rw_opt, int num_cus);"):
        assert decl in dbg
    for name in ("ppls_xprod_pass", "ppls_xprod_tile_nt", "ppls_xprod_tile_rows"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ppls_xprod_pass"][1]) == 18
    assert callable(Context.xprod_pass)
