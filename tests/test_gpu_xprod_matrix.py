"""Every cross-product tile kernel instantiation against long double (tests/xprod_bar.py).

``Context.xprod_pass`` runs ppls_xprod_tile_kernel<R, RW, NT> (and ppls_xprod_gram_kernel) alone through
ppls_launch_xprod_tile, the launcher xprod_stats() calls, on a caller's S, W, C and alpha..delta, with every
output between checked NaN guards.  Every case asserts the (rw, nt) that ran, holds M = S B, X'mu_T, Y'mu_U
and the Gram entrywise to an a-priori bar (nothing in it is measured), requires exact zeros in the rows that
belong to padding columns of S, a bitwise symmetric Gram, and the same bits from a second identical call.

  (a) the matrix: all 56 (R, RW) forms, cached loads, at (p, q) = (301, 39): ldx = 302, ldy = 40, P = 342.
      The X phase ends in a partial tile in both geometries (256 + 46 with an empty second sub-tile for
      R <= 5, 128 + 128 + 46 for R >= 6), the Y phase is one partial tile, waves of RW = 4 and 8 hold rows on
      both sides of the X/Y seam at row 302, 342 = 4 x 85 + 2 = 8 x 42 + 6 so the last live wave has rows
      past P, and the last workgroup has whole waves past P for every waves x RW
      (test_xprod_bar_host.test_forms_and_shape_properties asserts all five).  The bar case and the exact
      integer case; on top, M is bit-identical across RW at fixed R, and column t of M is bit-identical
      across every R > t.
  (b) shape edges at R in {1, 5, 6, 8, 16}, every legal RW: p in {1, 2, 37, 127, 128, 129, 255, 256, 257,
      258} with q = 3 and transposed, p = q = 1 (P = 4, less than one wave's rows), and the Gram kernel's
      row counts ldx in {768, 770, 1024, 1026, 2050} (tail only, mixed, unrolled only, unrolled + tail,
      two unrolled rounds + tail) with q = 3 and transposed.
  (c) non-temporal loads: all 56 forms at P = 5122 (p = 5100, q = 2, 64 rows), S formed on the device and
      read back, one module-scoped long-double reference.
  (d) switches: with_gram = 0, stop = 1, and each refusal.
  (e) the tie to production: Context.xprod_stats' Gram is xprod_pass' bit for bit, and its SX, SY lie inside
      the bar with the oracle's alpha..delta.

Worst err / bar on the MI355X when this file was written (each family prints its own; they are a record,
not thresholds): matrix 0.060 (M; SX 0.0065, SY 0.0047, G 0.021), edges 0.41, Gram rows 0.41, NT 0.44,
production 0.070.  The narrow side sets the larger figures: with q = 3 (or 2) the bar is gamma_6 (gamma_4) on
three (two) terms.  The across-R bitwise check holds on the device.  Against a library with two seeded
in-bounds defects (the Gram kernel's fourth unrolled partial dropped; <7, 8> publishing its last component
one row off) exactly test_matrix[7], the across-R check and test_gram_rows[770, 1024, 1026, 2050] failed.
"""
import functools

import numpy as np
import pytest

import xprod_bar as xb
from sweep_bar import sweep_problem

pytestmark = pytest.mark.gpu

E_ARG = -1
MATRIX = (301, 39, 48)          # p, q, rows of D
NT = (5100, 2, 64)
EDGE_R = (1, 5, 6, 8, 16)
EDGE_P = (1, 2, 37, 127, 128, 129, 255, 256, 257, 258)
GRAM_LD = (768, 770, 1024, 1026, 2050)

WORST = {}                      # family -> worst err / bar
RAN = {}                        # (family, R, RW) -> (rw, nt) asserted
STARTED = {}                    # family -> the R whose case was started


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


class Case:
    """One shape's bar problem and exact problem in the padded layout, with their references."""

    def __init__(self, p, q, rows, seed, ldx=None, ldy=None, exact=True, fill=0.0):
        self.p, self.q = p, q
        S, W, C, self.coef = xb.problem(p, q, rows, seed)
        self.ref = xb.XprodReference(S, p, q, W, C, self.coef, ldx, ldy)
        self.ldx, self.ldy = self.ref.ldx, self.ref.ldy
        self.Sp, self.Wp, self.Cp = xb.padded(S, W, C, p, q, fill, ldx, ldy)
        self.exact = None
        if exact:
            S, W, C, coef = xb.exact_problem(p, q, seed + 1)
            self.exact = (coef,) + xb.padded(S, W, C, p, q, fill, ldx, ldy)
            self.exact_want = xb.exact_reference(S, W, C, coef, p, q, ldx, ldy)      # all 16 columns, once

    def exact_for(self, r):
        """The int64 result of the exact problem's first r columns (the prefix property)."""
        M, SX, SY, G = self.exact_want
        c = np.r_[np.arange(r), xb.RMAX + np.arange(r)]
        return M[:, c], SX[:, :r], SY[:, :r], G[np.ix_(c, c)]


@functools.lru_cache(maxsize=None)
def _matrix_case():
    p, q, rows = MATRIX
    return Case(p, q, rows, seed=p + q)


def _bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("M", "SX", "SY", "G"))


def _run(ctx, case, r, rw, family, nt=0, S="host"):
    """One form on one case: the bar problem (twice) and the exact problem.  Returns the bar problem's M."""
    P = case.ldx + case.ldy
    W, C, cf = xb.first(r, case.Wp, case.Cp, case.coef)
    Sarg = case.Sp if S == "host" else None
    out = ctx.xprod_pass(W, C, cf, Sarg, rw=rw)
    assert (out["rw"], out["nt"]) == (rw, nt) and nt == xb.tile_nt(P), (r, rw, out["rw"], out["nt"])
    rat = case.ref.ratios(out["M"], out["SX"], out["SY"], out["G"])
    assert max(rat.values()) <= 1.0, (family, case.p, case.q, r, rw, rat)       # (a padding row that is not 0 reads inf)
    assert np.array_equal(out["G"], out["G"].T), (r, rw)
    again = ctx.xprod_pass(W, C, cf, Sarg, rw=rw)
    assert _bits(out, again), (family, r, rw, "a second identical call differs")
    if case.exact is not None:
        c0, Sp, Wp, Cp = case.exact
        got = ctx.xprod_pass(*xb.first(r, Wp, Cp, c0), Sp, rw=rw)
        for k, w in zip(("M", "SX", "SY", "G"), case.exact_for(r)):
            assert np.array_equal(got[k], w), (family, case.p, case.q, r, rw, k, "the exact case is not exact")
    WORST[family] = max(WORST.get(family, 0.0), *rat.values())
    RAN[(family, r, rw)] = (out["rw"], out["nt"])
    return out["M"], rat


# ------------------------------------------------------------------------------------ (a) the matrix
MATRIX_M = {}     # (R, RW) -> M of the bar problem


@pytest.mark.parametrize("r", range(1, xb.RMAX + 1))
def test_matrix(ctx, r):
    case = _matrix_case()
    STARTED.setdefault("matrix", set()).add(r)
    worst = {}
    for rw in xb.legal_rw(r):
        MATRIX_M[(r, rw)], rat = _run(ctx, case, r, rw, "matrix")
        worst = {k: max(worst.get(k, 0.0), v) for k, v in rat.items()}
        # every form sums a row of M in the same column order
        assert np.array_equal(MATRIX_M[(r, rw)], MATRIX_M[(r, 1)]), (r, rw, "M differs from the RW = 1 form's")
    print(f"matrix r={r}: worst err/bar {worst}")


def test_matrix_columns_do_not_depend_on_r(ctx):
    """Column t of M = S B is bit-identical for every R > t and every RW: a lane's fma chain runs over its
    own two columns of each 128-column sub-tile in column order whatever R, RW and the sub-tiles per barrier
    are, and the six butterfly levels add the same lane pairs in the same order wherever the value sits."""
    case = _matrix_case()
    for r, rw in xb.FORMS:
        if (r, rw) not in MATRIX_M:                 # (a -k selection: run what the matrix did not)
            W, C, cf = xb.first(r, case.Wp, case.Cp, case.coef)
            MATRIX_M[(r, rw)] = ctx.xprod_pass(W, C, cf, case.Sp, rw=rw)["M"]
    full = MATRIX_M[(xb.RMAX, 1)]
    bad = []
    for (r, rw), M in sorted(MATRIX_M.items()):
        for t in range(r):
            if not (np.array_equal(M[:, t], full[:, t]) and np.array_equal(M[:, r + t], full[:, xb.RMAX + t])):
                bad.append((r, rw, t))
    assert not bad, bad


# --------------------------------------------------------------------------------- (b) shape edges
def _edge(ctx, p, q, family, ldx=None, ldy=None, rows=40):
    case = Case(p, q, rows, seed=1000 * p + q, ldx=ldx, ldy=ldy, fill=1.0)   # the padding rows of W, C must not matter
    worst = 0.0
    for r in EDGE_R:
        for rw in xb.legal_rw(r):
            worst = max(worst, *_run(ctx, case, r, rw, family)[1].values())
    print(f"{family} p={p} q={q} ldx={case.ldx} ldy={case.ldy}: worst err/bar {worst:.3g}")


@pytest.mark.parametrize("p", EDGE_P)
def test_edges(ctx, p):
    _edge(ctx, p, 3, "edges")
    _edge(ctx, 3, p, "edges")


def test_edge_smaller_than_a_wave(ctx):
    _edge(ctx, 1, 1, "edges")                       # P = 4


@pytest.mark.parametrize("ld", GRAM_LD)
def test_gram_rows(ctx, ld):
    """The Gram kernel's 4-way unrolled loop takes more than 768 rows: ld rows on the X side, then on the Y
    side (the columns are all real here: p = ld)."""
    _edge(ctx, ld, 3, "gram rows", ldx=ld)
    _edge(ctx, 3, ld, "gram rows", ldy=ld)


# ------------------------------------------------------------------------------- (c) non-temporal
@pytest.fixture(scope="module")
def nt_case():
    """S of 64 rows at P = 5122 formed on the device, read back, and its long-double reference (once)."""
    from ppls_amd import Context
    from ppls_amd._lib import lib
    p, q, rows = NT
    D, W, C, coef = xb.data(p, q, rows, seed=p + q)
    c = Context(0)
    c.set_data(D[:, :p], D[:, p:])
    c.xprod_prepare()
    Sp, ldx = c.xprod_matrix(padded=True)
    P = Sp.shape[0]
    assert (ldx, P) == (5120, 5122)
    assert lib().ppls_xprod_tile_nt(5122) == 1 and lib().ppls_xprod_tile_nt(5120) == 0
    live = np.r_[np.arange(p), ldx + np.arange(q)]
    pad = np.setdiff1d(np.arange(P), live)
    assert not Sp[pad].any() and not Sp[:, pad].any()
    case = Case.__new__(Case)
    case.p, case.q, case.coef, case.exact = p, q, coef, None
    case.ref = xb.XprodReference(Sp[np.ix_(live, live)], p, q, W, C, coef)
    case.ldx, case.ldy = case.ref.ldx, case.ref.ldy
    case.Sp, case.Wp, case.Cp = xb.padded(Sp[np.ix_(live, live)], W, C, p, q)
    assert np.array_equal(case.Sp, Sp)
    yield c, case
    c.close()


@pytest.mark.parametrize("r", range(1, xb.RMAX + 1))
def test_nontemporal(nt_case, r):
    c, case = nt_case
    STARTED.setdefault("nt", set()).add(r)
    worst = 0.0
    for rw in xb.legal_rw(r):
        worst = max(worst, *_run(c, case, r, rw, "nt", nt=1, S=None)[1].values())
    print(f"nt r={r}: worst err/bar {worst:.3g}")


# ------------------------------------------------------------------------------------ (d) switches
def test_without_gram_and_stopped(ctx):
    case = _matrix_case()
    for r in (3, 8, 12):
        W, C, cf = xb.first(r, case.Wp, case.Cp, case.coef)
        full = ctx.xprod_pass(W, C, cf, case.Sp, rw=2)
        out = ctx.xprod_pass(W, C, cf, case.Sp, rw=2, with_gram=False)
        assert np.all(np.isnan(out["G"]))                                  # the Gram slot: still the fill
        assert all(np.array_equal(out[k], full[k]) for k in ("M", "SX", "SY"))
        out = ctx.xprod_pass(W, C, cf, case.Sp, rw=2, stop=True)
        assert all(np.all(np.isnan(out[k])) for k in ("M", "SX", "SY", "G"))
        assert (out["rw"], out["nt"]) == (2, 0)


def test_refusals(ctx):
    from ppls_amd import PplsError
    rng = np.random.default_rng(0)

    def call(ldx, ldy, r, rw):
        P = ldx + ldy
        with pytest.raises(PplsError) as e:
            ctx.xprod_pass(rng.standard_normal((ldx, r)), rng.standard_normal((ldy, r)), np.ones((4, r)), np.eye(P), rw=rw)
        assert e.value.code == E_ARG, (ldx, ldy, r, rw)

    call(7, 4, 2, 1)        # ldx odd
    call(6, 5, 2, 1)        # ldy odd
    call(0, 4, 2, 1)        # ldx below 2
    call(6, 0, 2, 1)        # ldy below 2
    call(6, 4, 17, 1)       # r outside 1..16
    call(6, 4, 2, 3)        # rw = 3
    call(6, 4, 9, 8)        # rw = 8 with r = 9
    import ctypes as ct
    from ppls_amd._lib import dptr
    W, C, S, cf, M, st = np.zeros((6, 1)), np.zeros((4, 1)), np.eye(10), np.ones(1), np.zeros(20), np.zeros(14)
    rc = ctx._L.ppls_xprod_pass(ctx.h, dptr(S), 10, 6, dptr(W), dptr(C), dptr(cf), dptr(cf), dptr(cf), dptr(cf), 0, 1, 1, 0,
                                dptr(M), dptr(st), None, None)
    assert rc == E_ARG      # r = 0
    ok = ctx.xprod_pass(np.ones((6, 8)), np.ones((4, 8)), np.ones((4, 8)), np.eye(10), rw=8)     # and r = 8 takes rw = 8
    assert ok["rw"] == 8 and np.array_equal(ok["M"][:6, :8], np.ones((6, 8)))


# ---------------------------------------------------------------------- (e) the tie to production
@pytest.mark.parametrize("n,p,q,r", [(120, 70, 37, 5), (90, 129, 31, 10)])
def test_production_statistics_are_the_pass(n, p, q, r):
    """Context.xprod_stats (theta uploaded, the library's alpha..delta) against xprod_pass on the same S with
    the same padded W, C and rows per wave: the Gram does not depend on the coefficients, so it is the same
    bits; SX and SY lie inside the bar with the oracle's alpha..delta at sweep_bar's well-conditioned theta."""
    from ppls_amd import Context, Theta
    from sweep_bar import coefficients
    X, Y, thd = sweep_problem(n, p, q, r, seed=n + p + q + r)
    coef = np.array(coefficients(thd))
    with Context(0) as c:
        c.set_data(X, Y)
        c.xprod_prepare()
        Sp, ldx = c.xprod_matrix(padded=True)
        SX, SY, G = c.xprod_stats(Theta(**thd))
        live = np.r_[np.arange(p), ldx + np.arange(q)]
        ref = xb.XprodReference(Sp[np.ix_(live, live)], p, q, thd["W"], thd["C"], coef)
        _, Wp, Cp = xb.padded(Sp[np.ix_(live, live)], thd["W"], thd["C"], p, q)
        out = c.xprod_pass(Wp, Cp, coef, None, rw=0)
        assert out["rw"] == c.xprod_info(r)["rows_per_wave"] and out["nt"] == 0
    assert np.array_equal(G, out["G"])
    SXp, SYp = np.zeros((ref.ldx, r)), np.zeros((ref.ldy, r))
    SXp[:p], SYp[:q] = SX, SY
    rat = ref.ratios(out["M"], SXp, SYp, G)
    print(f"production n={n} p={p} q={q} r={r}: err/bar {rat}")
    assert max(rat.values()) <= 1.0, rat
    rat2 = ref.ratios(out["M"], out["SX"], out["SY"], out["G"])
    assert max(rat2.values()) <= 1.0, rat2
    WORST["production"] = max(WORST.get("production", 0.0), *rat.values())


# -------------------------------------------------------------------------------------- the record
def test_every_form_ran():
    """All 56 cached and all 56 non-temporal forms ran and asserted their own (rw, nt) (this test follows them
    in the file: run the module as a whole; a -k selection leaves only the printout)."""
    for fam in ("matrix", "nt"):
        ran = {(r, rw): v for (f, r, rw), v in RAN.items() if f == fam}
        if STARTED.get(fam) == set(range(1, xb.RMAX + 1)):
            assert set(ran) == set(xb.FORMS) and len(ran) == 56, sorted(set(xb.FORMS) - set(ran))
            assert all(v == (rw, int(fam == "nt")) for (r, rw), v in ran.items())
    for fam in sorted(WORST):
        print(f"{fam}: worst err/bar {WORST[fam]:.3g}")
