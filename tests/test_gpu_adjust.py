"""Covariate adjustment on the device: ppls_adjust_data / ppls_get_adjustment /
ppls_xprod_adjust and their debug entries, Context.adjust_data, adjust_data, adjust_new,
stream_data(covariates=True), predict_PPLS(Znew=) and diagnostics_PPLS(Z=).

References are long double (tests/adjust_bar.py); every bar is the a-priori one derived there.  For fp32
storage the reference is applied to what the device holds, ``X.astype(float32).astype(float64)``.  Fits are
compared at the project's 1e-8 (README, "Parity"), shards at its 1e-12.
"""
import ctypes as ct
import functools
import threading

import numpy as np
import pytest

import adjust_bar as ab
from adjust_bar import L
from conftest import make_problem
from oracle import ppls_oracle as o
from oracle.r_rng import r_scale

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
K1S = (1, 2, 4, 5, 8, 9, 16)


def _ctx(dtype=0, xprod=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", xprod)
    return c


def _held(A, dtype):
    return A.astype(np.float32).astype(np.float64) if dtype else np.asarray(A, dtype=np.float64)


def _data(n, p, q, k, seed=0):
    """X, Y with a covariate share, and Z (k columns of unequal scale and offset)."""
    rng = np.random.default_rng([seed, n, p, q, k])
    Z = rng.standard_normal((n, k)) * (1.0 + np.arange(k) % 3) + (np.arange(k) % 4 - 1.5)

    def block(m):
        j = np.arange(m)
        return (Z @ rng.standard_normal((k, m)) * 0.7 + rng.standard_normal((n, m)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7)
    return block(p), block(q), Z


def _relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _theta(th):
    from ppls_amd import Theta
    return Theta(th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])


# ------------------------------------------------------------------------------ 1. the coefficient pass alone
COEF_SHAPES = [(1, 1), (5, 3), (514, 2), (1030, 6)]


@functools.lru_cache(maxsize=None)
def _coef_case(n, p, q, dtype):
    """Data, a 16-column Q (any values serve: the pass does not need orthonormal columns) and Q'D in long
    double, once per shape; the k1 leading columns serve every smaller k1."""
    rng = np.random.default_rng([n, p, q, dtype])
    X = rng.standard_normal((n, p)) * (0.5 + np.arange(p) % 7) + (np.arange(p) % 5 - 2)
    Y = rng.standard_normal((n, q)) * (0.5 + np.arange(q) % 3)
    Q = rng.standard_normal((n, 16)) / np.sqrt(n)
    D = np.hstack([_held(X, dtype), _held(Y, dtype)])
    ref = Q.T.astype(L) @ D.astype(L)
    for a in (X, Y, Q, D, ref):
        a.setflags(write=False)
    return X, Y, Q, D, ref


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("p,q", COEF_SHAPES, ids=[f"p{p}q{q}" for p, q in COEF_SHAPES])
@pytest.mark.parametrize("n", [1, 7, 257, 4099])
def test_coefficient_pass(n, p, q, dtype):
    X, Y, Q, D, ref = _coef_case(n, p, q, dtype)
    with _ctx(dtype) as c:
        c.set_data(X, Y)
        before = c.get_data()
        for k1 in K1S:
            info = c.adjust_info(k1)
            assert info["kt"] == ab.kt_of(k1)                       # the instantiation, by name
            px, py = ab.scale_plan(n, p, dtype), ab.scale_plan(n, q, dtype)
            for side, pl in (("X", px), ("Y", py)):
                assert info[side] == {k: pl[k] for k in ("tx", "ty", "grid_x", "grid_y", "nblocks")}
            if (p, dtype) in ((514, 0), (1030, 1)):
                assert info["X"]["grid_x"] > 1                      # crosses one column tile of tx = 256 units
            Qk = np.ascontiguousarray(Q[:, :k1])
            P = p + q
            buf = np.full(k1 * P + 8, np.nan)                       # NaN guards behind G
            rc = c._L.ppls_adjust_coef(c.h, Qk.ctypes.data_as(ct.POINTER(ct.c_double)), k1,
                                       buf.ctypes.data_as(ct.POINTER(ct.c_double)))
            assert rc == 0 and np.all(np.isnan(buf[k1 * P:])) and np.all(np.isfinite(buf[: k1 * P]))
            G = buf[: k1 * P].reshape(k1, P)
            bar = np.hstack([ab.coef_bar(Qk, D[:, :p], px["nblocks"]), ab.coef_bar(Qk, D[:, p:], py["nblocks"])])
            r = ab.inside(G, ref[:k1], bar)
            print(f"n={n} p={p} q={q} {'fp32' if dtype else 'fp64'} k1={k1} KT={info['kt']}: G err/bar {r:.3g}")
            assert r <= 1.0
            assert np.array_equal(c.adjust_coef(Qk), G)             # the same bits on a second call
        after = c.get_data()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ------------------------------------------------------------------------------ 2. adjust_data: values
ADJ_SHAPES = {
    "odd_p": (67, 37, 19, 3),
    "row_blocks": (1031, 5, 3, 8),
    "ld320": (40, 301, 19, 15),      # fp32 rows padded to 128 B; k1 = 16 of n = 40
    "tiny": (4, 1, 1, 1),
}


def _check_residuals(tag, c, X, Y, Z, dtype, intercept=True, ranks=1, rows=None):
    """The context's rows against the long-double residuals of what the device held."""
    n, p = X.shape
    D = np.hstack([_held(X, dtype), _held(Y, dtype)])
    exact, Qld = ab.ld_resid(Z, D, intercept)
    gX, gY = rows if rows is not None else c.get_data()
    got = np.hstack([gX, gY])
    q = ab.design_q(Z, intercept)
    Q = q["Q"]
    G = np.asarray(ab.ld_coef(Q, D), dtype=np.float64)
    gbar = np.hstack([ab.coef_bar(Q, D[:, :p], ab.scale_plan(n, p, dtype)["nblocks"], ranks),
                      ab.coef_bar(Q, D[:, p:], ab.scale_plan(n, Y.shape[1], dtype)["nblocks"], ranks)])
    bar = (ab.resid_bar(Q, G, D, gbar, dtype, np.asarray(exact, dtype=np.float64))
           + ab.design_terms(Q, G, D, ab.design_kappa(Z, intercept)))
    r = ab.inside(got, exact, bar)
    # Q'D of the result is zero within the bar carried through |q|
    back = np.abs(np.asarray(Qld.T @ got.astype(L), dtype=np.float64))
    rz = float(np.max(back / (np.abs(np.asarray(Qld, dtype=np.float64)).T @ bar)))
    print(f"{tag}: residual err/bar {r:.3g} (max err {np.abs(got - np.asarray(exact, dtype=float)).max():.3g}), Q'R / bar {rz:.3g}")
    assert got.shape == exact.shape and r <= 1.0 and rz <= 1.0
    return exact


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", list(ADJ_SHAPES))
def test_adjust_data_matches_lm_residuals(shape, dtype):
    n, p, q, k = ADJ_SHAPES[shape]
    X, Y, Z = _data(n, p, q, k)
    with _ctx(dtype) as c, _ctx(dtype) as fresh:
        c.set_data(X, Y)
        c.adjust_data(Z)
        gX, gY = c.get_data()
        rX, rY = c.get_data_rows()
        assert np.array_equal(rX, gX) and np.array_equal(rY, gY)
        _check_residuals(f"{shape} {'fp32' if dtype else 'fp64'}", c, X, Y, Z, dtype)
        fresh.set_data(gX, gY)                      # ||X||^2, ||Y||^2 (summed over whole rows: the padding is still zero)
        assert c.ssq() == fresh.ssq()
        ad, sc = c.adjustment(), c.scaling()
    D = np.hstack([_held(X, dtype), _held(Y, dtype)])
    gam = np.hstack([ad["coefX"], ad["coefY"]])
    lst = np.linalg.lstsq(np.hstack([np.ones((n, 1)), Z]), D, rcond=None)[0]
    gbar = ab.gamma_bar(Z, D)
    rg = ab.inside(gam, ab.ld_gamma(Z, D), gbar)
    print(f"{shape}: Gamma err/bar {rg:.3g}; lstsq {ab.inside(lst[1:], ab.ld_gamma(Z, D), gbar):.3g}")
    assert ad["k"] == k and rg <= 1.0 and ab.inside(gam, lst[1:], 2 * gbar) <= 1.0
    assert np.abs(ad["zcenter"] - Z.mean(axis=0)).max() <= 1e-13 * max(1.0, np.abs(Z).max())
    cen = np.hstack([sc["centerX"], sc["centerY"]])
    assert np.abs(cen - D.mean(axis=0)).max() <= 1e-12 * np.abs(D).max()
    assert np.all(sc["scaleX"] == 1) and np.all(sc["scaleY"] == 1)


def test_padding_stays_zero_and_fit_reads_it():
    """ld2560 / fp64 takes the panel sweep, which reads the padding columns of every row."""
    n, p, q, k, r = 40, 2100, 5, 2, 2
    X, Y, Z = _data(n, p, q, k)
    th0 = make_problem(n, p, q, r, seed=3)[2]
    with _ctx() as c, _ctx() as fresh:
        c.set_data(X, Y)
        c.adjust_data(Z)
        fresh.set_data(*c.get_data())
        assert c.ssq() == fresh.ssq()
        est, ll, _, _ = c.em_run(_theta(th0), 3, -1.0)
        est_f, ll_f, _, _ = fresh.em_run(_theta(th0), 3, -1.0)
    assert np.array_equal(ll, ll_f) and np.array_equal(est.W, est_f.W)


def test_module_adjust_data_and_intercept_only():
    from ppls_amd import adjust_data
    n, p, q, k = ADJ_SHAPES["odd_p"]
    X, Y, Z = _data(n, p, q, k)
    with _ctx() as c, _ctx() as s:
        out = adjust_data(X, Y, Z, ctx=c)
        assert set(out) == {"coefX", "coefY", "zcenter", "centerX", "centerY", "ss_explainedX", "ss_explainedY"}
        D = np.hstack([X, Y])
        exact, _ = ab.ld_resid(Z, D)
        ss = np.asarray((D.astype(L) ** 2).sum(axis=0) - (exact ** 2).sum(axis=0), dtype=float)   # Pythagoras
        assert _relerr(np.hstack([out["ss_explainedX"], out["ss_explainedY"]]), ss) < 1e-11
        # without an intercept: centres 0
        c.set_data(X, Y)
        out0 = adjust_data(None, None, Z, intercept=False, ctx=c)
        assert not out0["centerX"].any() and not out0["zcenter"].any()
        _check_residuals("no intercept", c, X, Y, Z, 0, intercept=False)
        # a design of the intercept alone (Z = a column that the intercept does not alias: the residual is
        # the centred data once Z's own share is out) -- here: centring = adjusting for nothing else
        s.set_data(X, Y)
        s.scale_data(True, False)
        cX, cY = s.get_data()
        c.set_data(X, Y)
        c.adjust_data(np.ones((n, 1)), intercept=False)             # Z = 1: centring is this special case
        gX, gY = c.get_data()
        xmax = np.abs(D).max(axis=0)
        # sum of both bars: scale_data's 2 (n + 4) u (max|x| + |z|) and the residual bar with q = 1 / sqrt(n)
        Q1 = np.full((n, 1), 1.0 / np.sqrt(n))
        G1 = np.asarray(ab.ld_coef(Q1, D), dtype=float)
        bar = (2 * (n + 4) * ab.U * (xmax + np.abs(np.hstack([cX, cY])))
               + ab.resid_bar(Q1, G1, D, ab.coef_bar(Q1, D, ab.scale_plan(n, p, 0)["nblocks"]))
               + ab.design_terms(Q1, G1, D, 1.0))
        r = ab.inside(np.hstack([gX, gY]), np.hstack([cX, cY]), bar)
        print(f"intercept-only design against scale_data(center): err/bar {r:.3g}")
        assert r <= 1.0


# ------------------------------------------------------------------------------ 3. context state, composition
def test_state_after_adjusting_and_composition():
    from ppls_amd import PplsError, adjust_new
    n, p, q, k = ADJ_SHAPES["odd_p"]
    X, Y, Z = _data(n, p, q, k)
    th0 = make_problem(n, p, q, 2, seed=4)[2]
    with _ctx(0, 1) as c, _ctx(0, 1) as fresh, _ctx() as t:
        c.set_data(X, Y)
        c.xprod_prepare()                          # S of the raw data: must not survive
        assert c.xprod_info(2)["ready"]
        c.adjust_data(Z)
        assert not c.xprod_info(2)["ready"]
        fresh.set_data(*c.get_data())
        est, ll, _, _ = c.em_run(_theta(th0), 5, -1.0)          # ... and the next fit forms it anew
        est_f, ll_f, _, _ = fresh.em_run(_theta(th0), 5, -1.0)
        assert c.xprod_info(2)["ready"] and np.array_equal(ll, ll_f) and np.array_equal(est.W, est_f.W)
        c.em_begin(_theta(th0))
        c.em_iterate(1)
        c.set_data(X, Y)
        c.em_begin(_theta(th0))
        c.em_iterate(1)
        c.adjust_data(Z)                           # an ppls_em_begin session ends with the data change
        with pytest.raises(PplsError) as ei:
            c.em_iterate(1)
        assert ei.value.code == E_STATE
        # scale_data afterwards composes: the two records reproduce the loaded rows
        c.scale_data()
        gX, gY = c.get_data()
        sc, ad = c.scaling(), c.adjustment()
        back = np.hstack([gX * sc["scaleX"] + sc["centerX"], gY * sc["scaleY"] + sc["centerY"]]) \
            + (Z - ad["zcenter"]) @ np.hstack([ad["coefX"], ad["coefY"]])
        assert np.abs(back - np.hstack([X, Y])).max() <= 1e-11 * np.abs(np.hstack([X, Y])).max()
        aX, aY = adjust_new(c, X, Y, Z)
        assert np.abs(aX - gX).max() <= 1e-11 and np.abs(aY - gY).max() <= 1e-11
        # = R's scale(resid(lm(.)))
        exact, _ = ab.ld_resid(Z, np.hstack([X, Y]))
        want = r_scale(np.asarray(exact, dtype=float))
        assert np.abs(np.hstack([gX, gY]) - want).max() <= 1e-11
        # set_data_from copies the record; cv_PPLS runs on an adjusted context
        t.set_data_from(c, np.arange(0, n, 2))
        assert t.adjustment()["k"] == k and np.array_equal(t.adjustment()["coefX"], ad["coefX"])
        assert np.array_equal(t.scaling()["scaleY"], sc["scaleY"])
        from ppls_amd import cv_PPLS
        assert np.isfinite(cv_PPLS(None, None, 2, 3, ctx=c, EMsteps=5, atol=1e-4))
        c.set_data(X, Y)                           # new data clear it
        assert c.adjustment()["k"] == 0


def test_fits_on_adjusted_context_match_oracle_on_host_residuals():
    from ppls_amd import PPLS, PPLS_simult
    n, p, q, k, r = 150, 12, 9, 3, 3
    X0, Y0, th0 = make_problem(n, p, q, r, seed=12)
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((n, k)) + [0.5, -1.0, 2.0]
    X, Y = X0 + Z @ rng.standard_normal((k, p)), Y0 + Z @ rng.standard_normal((k, q))
    exact, _ = ab.ld_resid(Z, np.hstack([X, Y]))
    H = r_scale(np.asarray(exact, dtype=float))     # host: resid(), then scale()
    Xh, Yh = H[:, :p], H[:, p:]
    with _ctx() as c:
        c.set_data(X, Y)
        c.adjust_data(Z)
        c.scale_data()
        fit = PPLS(None, None, r, 30, -1.0, "equal", ctx=c)
        sim = PPLS_simult(None, None, r, 10, -np.inf, init=th0, ctx=c)
    ref = o.ppls(Xh, Yh, r, 30, -1.0, theta0s=[o.initial_guess(p, q, "equal")] * r)
    sref = o.ppls_simult(Xh, Yh, r, EMsteps=10, atol=-np.inf, theta0=th0)
    print(f"PPLS W err {np.abs(fit['W'] - ref['W']).max():.3g}, PPLS_simult W err "
          f"{np.abs(sim['estimates']['W'] - sref['estimates']['W']).max():.3g}")
    assert np.abs(fit["W"] - ref["W"]).max() < 1e-8 and np.abs(fit["C"] - ref["C"]).max() < 1e-8
    assert np.abs(sim["estimates"]["W"] - sref["estimates"]["W"]).max() < 1e-8
    assert np.abs(sim["estimates"]["C"] - sref["estimates"]["C"]).max() < 1e-8


# ------------------------------------------------------------------------------ 4. shards
class ThreadAllReduce:
    """Sum over k host threads in rank order: every rank gets the bitwise-same result; a bounded
    barrier, so a rank that misses a collective fails the test instead of hanging it."""

    def __init__(self, k):
        self.k = k
        self.bar = threading.Barrier(k, timeout=60)
        self.bufs = [None] * k
        self.calls = 0

    def fn(self, rank):
        def reduce(buf):
            self.bufs[rank] = buf.copy()
            self.bar.wait()
            tot = self.bufs[0].copy()
            for b in self.bufs[1:]:
                tot += b
            self.bar.wait()
            if rank == 0:
                self.calls += 1
            buf[:] = tot
        return reduce


def _run_ranks(X, Y, bounds, work):
    """work(ctx, rank, lo, hi) on len(bounds) - 1 contexts of GPU 0 that hold the row ranges of X, Y."""
    n, nr = X.shape[0], len(bounds) - 1
    red = ThreadAllReduce(nr)
    out, errs = [None] * nr, []

    def body(rank):
        try:
            lo, hi = bounds[rank], bounds[rank + 1]
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.set_data(X[lo:hi], Y[lo:hi], n_total=n)
                out[rank] = work(c, rank, lo, hi)
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(nr)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
    if errs:
        raise errs[0]
    return out, red


@pytest.mark.parametrize("bounds", [[0, 30, 67], [0, 30, 67, 67], [0, 0, 67]], ids=["2ranks", "3ranks_last_empty", "2ranks_first_empty"])
def test_sharded_adjustment_equals_unsharded(bounds):
    n, p, q, k = ADJ_SHAPES["odd_p"]
    X, Y, Z = _data(n, p, q, k)
    with _ctx() as c:
        c.set_data(X, Y)
        c.adjust_data(Z)
        uX, uY = c.get_data()
        uad, usc, ussq = c.adjustment(), c.scaling(), c.ssq()

    def work(c, rank, lo, hi):
        c.adjust_data(Z[lo:hi])                     # a zero-row rank joins and returns PPLS_OK
        return c.adjustment(), c.scaling(), c.get_data(), c.ssq()

    out, red = _run_ranks(X, Y, bounds, work)
    assert red.calls > 0
    for ad, sc, _, ssq in out[1:]:
        assert np.array_equal(ad["coefX"], out[0][0]["coefX"]) and np.array_equal(sc["centerY"], out[0][1]["centerY"])
        assert ssq == out[0][3]
    gX = np.vstack([o_[2][0] for o_ in out])
    gY = np.vstack([o_[2][1] for o_ in out])
    scaleX, scaleY = np.abs(X).max(), np.abs(Y).max()
    print(f"shards {bounds}: rows {np.abs(gX - uX).max():.3g}, Gamma {np.abs(out[0][0]['coefX'] - uad['coefX']).max():.3g}")
    assert np.abs(gX - uX).max() <= 1e-12 * scaleX and np.abs(gY - uY).max() <= 1e-12 * scaleY
    assert _relerr(out[0][0]["coefX"], uad["coefX"]) <= 1e-12 and _relerr(out[0][0]["coefY"], uad["coefY"]) <= 1e-12
    assert _relerr(out[0][1]["centerX"], usc["centerX"]) <= 1e-12 and _relerr(out[0][3], ussq) <= 1e-12
    _check_residuals(f"sharded {bounds}", None, X, Y, Z, 0, ranks=len(bounds) - 1, rows=(gX, gY))


def test_sharded_refusal_is_the_same_on_every_rank():
    from ppls_amd import PplsError
    n, p, q, k = ADJ_SHAPES["odd_p"]
    X, Y, Z = _data(n, p, q, k)
    Zbad = Z.copy()
    Zbad[50, 1] = np.nan                            # one rank's rows hold it

    def work(c, rank, lo, hi):
        before = c.get_data()
        try:
            c.adjust_data(Zbad[lo:hi])
        except PplsError as e:
            after = c.get_data()
            return e.code, np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), c.adjustment()["k"]
        return 0, False, -1

    out, _ = _run_ranks(X, Y, [0, 30, 67, 67], work)
    assert all(o_ == (E_ARG, True, 0) for o_ in out)


# ------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_rows_and_record_untouched():
    from ppls_amd import PplsError
    n, p, q, k = ADJ_SHAPES["odd_p"]
    X, Y, Z = _data(n, p, q, k)

    def refused(c, code, match, call):
        before, rec = c.get_data(), (c.adjustment(), c.scaling())
        with pytest.raises(PplsError, match=match) as ei:
            call()
        assert ei.value.code == code
        after = c.get_data()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert c.adjustment()["k"] == rec[0]["k"] and np.array_equal(c.scaling()["centerX"], rec[1]["centerX"])

    dp = ct.POINTER(ct.c_double)
    with _ctx() as c:
        with pytest.raises(PplsError) as ei:        # no data
            c._chk(c._L.ppls_adjust_data(c.h, None, 1, 1, 1))
        assert ei.value.code == E_STATE
        c.set_data(X, Y)
        zp = np.ascontiguousarray(Z).ctypes.data_as(dp)
        refused(c, E_ARG, "NULL", lambda: c._chk(c._L.ppls_adjust_data(c.h, None, k, 1, 1)))
        refused(c, E_ARG, "covariates", lambda: c._chk(c._L.ppls_adjust_data(c.h, zp, 0, 1, 1)))
        Zw = np.random.default_rng(1).standard_normal((n, 16))
        refused(c, E_ARG, "covariates", lambda: c.adjust_data(Zw))                    # k1 = 17
        c.adjust_data(Zw[:, :15])                                                      # k1 = 16 is served
        c.set_data(X, Y)
        c.adjust_data(Zw, intercept=False)                                             # so is k = 16 without one
        c.set_data(X, Y)
        for bad in (np.nan, np.inf):
            Zb = Z.copy()
            Zb[n - 1, k - 1] = bad
            refused(c, E_ARG, "NaN or Inf", lambda: c.adjust_data(Zb))
        Zd = np.hstack([Z, Z[:, :1] * 2.0 + Z[:, 1:2]])                                # aliased: names the column
        refused(c, E_ARG, f"column {k + 1} is aliased", lambda: c.adjust_data(Zd))
        Zc = Z.copy()
        Zc[:, 1] = 3.0                                                                 # constant beside the intercept
        refused(c, E_ARG, "column 2 is constant", lambda: c.adjust_data(Zc))
        c.set_data(X[:4], Y[:4])
        refused(c, E_ARG, "degrees of freedom", lambda: c.adjust_data(Z[:4]))          # n_total <= k1
        c.set_data(X, Y)
        c.scale_data()
        refused(c, E_STATE, "adjust before scaling", lambda: c.adjust_data(Z))
        c.set_data(X, Y)
        c.adjust_data(Z)
        refused(c, E_STATE, "already adjusted", lambda: c.adjust_data(Z))
        # streamed, and an open stream
        c.stream_begin(p, q)
        with pytest.raises(PplsError) as ei:
            c.adjust_data(np.zeros((0, k)))
        assert ei.value.code == E_STATE
        c.stream_rows(X, Y)
        c.stream_end()
        with pytest.raises(PplsError) as ei:
            c._chk(c._L.ppls_adjust_data(c.h, None, k, 1, 1))
        assert ei.value.code == E_STATE


# ------------------------------------------------------------------------------ 6. the Schur kernel alone
def _schur_input(p, q, k, ldx, ldy_src, seed=0, n=80):
    rng = np.random.default_rng([seed, p, q, k])
    M = np.zeros((n, ldx + ldy_src))
    Z = rng.standard_normal((n, k))
    M[:, :p] = rng.standard_normal((n, p)) + Z @ rng.standard_normal((k, p)) * 0.5
    M[:, ldx:ldx + q] = rng.standard_normal((n, q)) + Z @ rng.standard_normal((k, q)) * 0.5
    M[:, ldx + q:ldx + q + k] = Z
    return M.T @ M


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("P_dst", [4, 66, 130])
def test_schur_kernel(P_dst, k):
    # padded ldx and ldy: one padding column each in dst
    ldx = P_dst // 2 if (P_dst // 2) % 2 == 0 else P_dst // 2 + 1
    ldy = P_dst - ldx
    p, q = ldx - 1, ldy - 1
    ldy_src = (q + k + 1) & ~1
    ldy_src += 2                                    # and more in src
    S = _schur_input(p, q, k, ldx, ldy_src)
    live = ab.joint_live(p, ldx, q, ldy)
    f, piv = ab.schur_f(S, ldx + q, k, live)
    assert piv == 0
    ref = ab.ld_schur(S, ldx + q, k, live)
    bar = ab.schur_bar(S, f, live)
    with _ctx() as c:
        got = c.xadjust_matrix(S, p, ldx, q + k, ldy_src, k, ldy)       # (NaN around the output: checked inside)
        got_s = c.xadjust_matrix(S, p, ldx, q + k, ldy_src, k, ldy, scale=True)
        assert c.adjust_timing()["schur"] > 0
    r = ab.inside(got, ref, bar)
    Rs, sbar = ab.schur_scaled(ref, bar, live)
    rs = ab.inside(got_s, Rs, sbar)
    print(f"P_dst={P_dst} k={k}: Schur err/bar {r:.3g}, scaled {rs:.3g}, kappa(C) {f['kappa']:.3g}")
    assert got.shape == (P_dst, P_dst) and np.all(np.isfinite(got)) and r <= 1.0 and rs <= 1.0
    for g in (got, got_s):
        assert np.array_equal(g, g.T)                                    # exact symmetry
        assert not g[~np.outer(live, live)].any()                        # zero padding
    assert np.abs(np.diag(got_s)[live] - 1.0).max() <= 8 * ab.U          # scale = 1: a unit diagonal


def test_schur_kernel_refusals():
    from ppls_amd import PplsError
    p, q, k, ldx, ldy_src, ldy = 3, 3, 2, 4, 6, 4
    S = _schur_input(p, q, k, ldx, ldy_src)
    z0 = ldx + q
    with _ctx() as c:
        Sd = S.copy()
        Sd[z0 + 1], Sd[:, z0 + 1] = Sd[z0], Sd[:, z0]                    # a duplicated covariate
        Sd[z0 + 1, z0 + 1] = Sd[z0, z0]
        with pytest.raises(PplsError, match="column 2 is aliased") as ei:
            c.xadjust_matrix(Sd, p, ldx, q + k, ldy_src, k, ldy)
        assert ei.value.code == E_ARG
        S0 = S.copy()
        S0[z0], S0[:, z0] = 0.0, 0.0
        with pytest.raises(PplsError, match="singular") as ei:
            c.xadjust_matrix(S0, p, ldx, q + k, ldy_src, k, ldy)
        assert ei.value.code == E_ARG
        with pytest.raises(PplsError) as ei:
            c.xadjust_matrix(S, p, ldx, q + k, ldy_src, q + k, ldy)      # k >= q_src
        assert ei.value.code == E_ARG


# ------------------------------------------------------------------------------ 7. xprod_adjust, stream_data
def _joint(S, p, ldx, q):
    """The live (p + q)^2 part of a joint-layout matrix."""
    idx = np.r_[np.arange(p), ldx + np.arange(q)]
    return S[np.ix_(idx, idx)]


def _xprod_pair(scale=True, n=120, p=11, q=7, k=3, seed=2):
    """(dst from a centred stream of [Y Z], the resident context adjusted and scaled the same way, data)."""
    X, Y, Z = _data(n, p, q, k, seed)
    src, dst, res = _ctx(), _ctx(), _ctx(0, 1)
    src.stream_begin(p, q + k, True, False)
    for lo in range(0, n, 50):
        src.stream_rows(X[lo:lo + 50], np.hstack([Y, Z])[lo:lo + 50])
    src.stream_end()
    dst.xprod_adjust(src, k, scale)
    res.set_data(X, Y)
    res.adjust_data(Z)
    res.scale_data(True, scale)
    return src, dst, res, (X, Y, Z)


def test_xprod_adjust_matches_resident_adjustment():
    from ppls_amd import PPLS_simult, variances_PPLS_simult
    src, dst, res, (X, Y, Z) = _xprod_pair()
    n, p, q, k = X.shape[0], X.shape[1], Y.shape[1], Z.shape[1]
    with src, dst, res:
        assert dst.stream_info()["state"] == "streamed" and dst.n_total == n and (dst.p, dst.q) == (p, q)
        assert dst.stream_info()["n_total"] == n
        S, ldx = dst.xprod_matrix(padded=True)
        P = S.shape[0]
        res.xprod_prepare()
        Sr, ldxr = res.xprod_matrix(padded=True)
        assert (P, ldx) == (Sr.shape[0], ldxr) and np.array_equal(S, S.T)
        # the sum of the two bars: the Schur bar of the unscaled complement brought to the scaled units, and the
        # resident Gram of n unit-variance rows (gamma(n + 2) |R|'|R| <= gamma(n + 2) (n - 1) by Cauchy-Schwarz),
        # with the residual bar's share: 2 |r| bar(r) summed over the rows <= 2 (n - 1) max relative bar(r)
        Ssrc, _ = src.xprod_matrix(padded=True)
        live = ab.joint_live(p, ldx, q, P - ldx)
        f, piv = ab.schur_f(Ssrc, ldx + q, k, live)
        assert piv == 0
        ubar = ab.schur_bar(Ssrc, f, live)
        ref = ab.ld_schur(Ssrc, ldx + q, k, live)
        d = np.sqrt(np.where(live, np.diag(np.asarray(ref, dtype=float)), 1.0) / (n - 1))
        _, sbar = ab.schur_scaled(ref / L(n - 1), ubar / (n - 1), live)
        sbar = sbar * (n - 1)
        rel_r = 64 * (n + 16) * ab.U * 16            # a residual's bar relative to its column's sd, generously: (k1 + 1) u (|x| + ...) / sd
        bar = sbar + (ab.gamma(n + 2) + 2 * rel_r) * (n - 1)
        r = ab.inside(S, Sr, bar)
        print(f"xprod_adjust against the resident S: max diff {np.abs(S - Sr).max():.3g}, diff/bar {r:.3g}")
        assert r <= 1.0
        assert np.abs(np.diag(_joint(S, p, ldx, q)) - (n - 1)).max() <= 1e-9
        sx, sy = dst.ssq()
        assert abs(sx - p * (n - 1)) <= 1e-8 and abs(sy - q * (n - 1)) <= 1e-8
        # both records
        sc, ad, rsc, rad = dst.scaling(), dst.adjustment(), res.scaling(), res.adjustment()
        for key in ("centerX", "centerY", "scaleX", "scaleY"):
            assert _relerr(sc[key], rsc[key]) <= 1e-10
        assert ad["k"] == k and _relerr(ad["coefX"], rad["coefX"]) <= 1e-9 and _relerr(ad["coefY"], rad["coefY"]) <= 1e-9
        assert np.abs(ad["zcenter"] - rad["zcenter"]).max() <= 1e-12
        # a repeated call reuses S
        dst.xprod_adjust(src, k, True)
        assert np.array_equal(S, dst.xprod_matrix(padded=True)[0]) and dst.stream_info()["state"] == "streamed"
        # a fit from dst equals the resident adjusted fit
        th0 = make_problem(n, p, q, 2, seed=6)[2]
        fit = PPLS_simult(None, None, 2, 10, -np.inf, init=th0, ctx=dst)
        rfit = PPLS_simult(None, None, 2, 10, -np.inf, init=th0, ctx=res)
        assert np.abs(fit["estimates"]["W"] - rfit["estimates"]["W"]).max() < 1e-8
        assert np.abs(fit["estimates"]["C"] - rfit["estimates"]["C"]).max() < 1e-8
        v = variances_PPLS_simult(fit, None, "X", ctx=dst, from_xprod=True)
        assert np.all(np.isfinite(v["seLoad"]))


def test_xprod_adjust_from_resident_source_and_refusals():
    from ppls_amd import PplsError
    n, p, q, k = 90, 6, 5, 2
    X, Y, Z = _data(n, p, q, k, seed=4)
    Xc, YZc = X - X.mean(axis=0), np.hstack([Y, Z]) - np.hstack([Y, Z]).mean(axis=0)
    with _ctx() as src, _ctx() as dst, _ctx() as res, _ctx() as empty:
        src.set_data(Xc, YZc)                      # resident: S is formed and kept
        dst.xprod_adjust(src, k, False)
        assert src.xprod_info(1)["ready"]
        res.set_data(X, Y)
        res.adjust_data(Z)
        res.xprod_prepare()
        S, ldx = dst.xprod_matrix(padded=True)
        Sr, _ = res.xprod_matrix(padded=True)
        assert np.abs(S - Sr).max() <= 1e-10 * np.abs(Sr).max()
        before = (S.copy(), dst.adjustment(), dst.stream_info())

        def refused(code, call):
            with pytest.raises(PplsError) as ei:
                call()
            assert ei.value.code == code
            S1, _ = dst.xprod_matrix(padded=True)
            assert np.array_equal(S1, before[0]) and dst.adjustment()["k"] == k and dst.stream_info() == before[2]

        for bad in (0, q + k, 17):
            refused(E_ARG, lambda: dst._chk(dst._L.ppls_xprod_adjust(dst.h, src.h, bad, 0)))
        refused(E_ARG, lambda: dst._chk(dst._L.ppls_xprod_adjust(dst.h, dst.h, 1, 0)))
        refused(E_STATE, lambda: dst._chk(dst._L.ppls_xprod_adjust(dst.h, empty.h, 1, 0)))
        empty.stream_begin(p, q + k)
        refused(E_STATE, lambda: dst._chk(dst._L.ppls_xprod_adjust(dst.h, empty.h, k, 0)))    # an open stream
        empty.stream_begin(p, q + k, True, False, nr_folds=2)
        empty.stream_rows(Xc, YZc, np.arange(n) % 2)
        empty.stream_end()
        refused(E_STATE, lambda: dst._chk(dst._L.ppls_xprod_adjust(dst.h, empty.h, k, 0)))    # a fold stream
        YZd = YZc.copy()
        YZd[:, q + 1] = YZd[:, q]                                                               # singular S_zz
        empty.set_data(Xc, YZd)
        refused(E_ARG, lambda: dst._chk(dst._L.ppls_xprod_adjust(dst.h, empty.h, k, 0)))
        YZ0 = YZc.copy()
        YZ0[:, 0] = 0.0                            # a Y column without spread: d_j = 0 under scale = 1
        empty.set_data(Xc, YZ0)
        with pytest.raises(PplsError) as ei:
            dst.xprod_adjust(empty, k, True)
        assert ei.value.code == E_ARG


def test_derivations_chain_on_one_destination():
    """One destination through every call that leaves a derived S, adopting a new S where the
    shape changes and reusing its own where it does not: after each call it equals, bit for bit, a fresh
    context given that call alone, and an EM session opened before the call is over."""
    from ppls_amd import PplsError
    n, p, q, k = 300, 13, 11, 2
    X, Y, Z = _data(n, p, q, k, seed=5)
    rng = np.random.default_rng(9)
    count = rng.multinomial(n, np.full(n, 1.0 / n)).astype(np.int32)
    weight = rng.uniform(0.2, 2.0, n)
    perm1, perm2 = rng.permutation(n), rng.permutation(n)
    th0 = {qq: _theta(make_problem(n, p, qq, 2, seed=4)[2]) for qq in (q, q + k)}
    steps = [
        ("resample", q + k, lambda c, s: c.xprod_resample(s, count)),
        ("permute", q + k, lambda c, s: c.xprod_permute(s, perm1)),
        ("adjust", q, lambda c, s: c.xprod_adjust(s, k, True)),           # q changes: a new S on a streamed context
        ("weighted", q + k, lambda c, s: c.xprod_weighted(s, weight)),    # ... and back
        ("permute again", q + k, lambda c, s: c.xprod_permute(s, perm2)),
        ("adjust again", q, lambda c, s: c.xprod_adjust(s, k, False)),
        ("adjust, reusing S", q, lambda c, s: c.xprod_adjust(s, k, True)),
    ]

    def state(c):
        S, ldx = c.xprod_matrix(padded=True)
        return dict(S=S, ldx=ldx, ssq=c.ssq(), n_total=c.n_total, shape=(c.p, c.q), stream=c.stream_info(),
                    scaling=c.scaling(), adjustment=c.adjustment())

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[key], b[key]) for key in a)
        return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b

    with _ctx() as src, _ctx() as work:
        src.set_data(X, np.hstack([Y, Z]))
        for name, q_after, call in steps:
            if work.streamed:
                work.em_begin(th0[work.q])
                work.em_iterate(1)
            call(work, src)
            with pytest.raises(PplsError) as ei:
                work.em_iterate(1)
            assert ei.value.code == E_STATE, name
            with _ctx() as fresh:
                call(fresh, src)
                got, want = state(work), state(fresh)
            assert got["shape"] == (p, q_after) and got["stream"]["state"] == "streamed", name
            for key in want:
                assert same(got[key], want[key]), f"{name}: {key} differs from a fresh context's"


def test_stream_data_with_covariates():
    from ppls_amd import PPLS_simult, stream_data
    n, p, q, k = 130, 9, 6, 2
    X, Y, Z = _data(n, p, q, k, seed=8)
    chunks = [(X[lo:hi], Y[lo:hi], Z[lo:hi]) for lo, hi in ((0, 50), (50, 51), (51, n))]
    th0 = make_problem(n, p, q, 2, seed=6)[2]
    with _ctx() as c, _ctx() as res:
        out = stream_data(chunks, ctx=c, covariates=True)
        assert {"n", "centerX", "scaleX", "centerY", "scaleY", "coefX", "coefY", "zcenter"} <= set(out) and out["n"] == n
        res.set_data(X, Y)
        res.adjust_data(Z)
        res.scale_data()
        assert _relerr(out["coefX"], res.adjustment()["coefX"]) <= 1e-9 and _relerr(out["scaleY"], res.scaling()["scaleY"]) <= 1e-10
        fit = PPLS_simult(None, None, 2, 10, -np.inf, init=th0, ctx=c)
        rfit = PPLS_simult(None, None, 2, 10, -np.inf, init=th0, ctx=res)
        assert np.abs(fit["estimates"]["W"] - rfit["estimates"]["W"]).max() < 1e-8
        assert np.abs(fit["estimates"]["C"] - rfit["estimates"]["C"]).max() < 1e-8
        with pytest.raises(ValueError, match="nr_folds"):
            stream_data([(X, Y, Z)], ctx=c, covariates=True, nr_folds=2)


# ------------------------------------------------------------------------------ 8. new rows
def test_predict_and_diagnostics_on_new_raw_rows():
    from ppls_amd import PPLS_simult, adjust_new, diagnostics_PPLS, predict_PPLS
    n, p, q, k = 140, 10, 7, 2
    X, Y, Z = _data(n, p, q, k, seed=10)
    Xn, Yn, Zn = _data(9, p, q, k, seed=11)
    th0 = make_problem(n, p, q, 2, seed=6)[2]
    with _ctx() as c, _ctx() as plain:
        c.set_data(X, Y)
        c.adjust_data(Z)
        c.scale_data()
        fit = PPLS_simult(None, None, 2, 10, -np.inf, init=th0, ctx=c)
        aX, aY = adjust_new(c, Xn, Yn, Zn)          # the host-adjusted rows
        sc, ad = c.scaling(), c.adjustment()
        for xy, raw, adj, other in (("X", Xn, aX, "Y"), ("Y", Yn, aY, "X")):
            got = predict_PPLS(fit, raw, xy, ctx=c, rescale=True, Znew=Zn)
            want = predict_PPLS(fit, adj, xy, ctx=c) * sc["scale" + other] + sc["center" + other] \
                + (Zn - ad["zcenter"]) @ ad["coef" + other]
            assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
            with pytest.raises(ValueError, match="Z"):
                predict_PPLS(fit, raw, xy, ctx=c, rescale=True)
        got = diagnostics_PPLS(fit, Xn, Yn, ctx=c, new=True, rescale=True, Z=Zn)
        want = diagnostics_PPLS(fit, aX, aY, ctx=c, new=True)
        assert np.allclose(got["d2"], want["d2"], rtol=1e-12, atol=0) and np.array_equal(got["flag"]["d2"], want["flag"]["d2"])
        sub = diagnostics_PPLS(fit, Xn, Yn, ctx=c, new=True, rescale=True, Z=Zn, subset=[4, 1])
        assert np.allclose(sub["d2"], want["d2"][[4, 1]], rtol=1e-12, atol=0)
        with pytest.raises(ValueError, match="Z"):
            diagnostics_PPLS(fit, Xn, Yn, ctx=c, new=True, rescale=True)
        # a context that is not adjusted behaves as before
        plain.set_data(X, Y)
        plain.scale_data()
        a = predict_PPLS(fit, Xn, "X", ctx=plain, rescale=True)
        psc = plain.scaling()
        b = predict_PPLS(fit, (Xn - psc["centerX"]) / psc["scaleX"], "X", ctx=plain) * psc["scaleY"] + psc["centerY"]
        assert np.array_equal(a, b)
