"""PO2PLS row diagnostics and the t-model fit on the device: the kernel against long double inside
the a-priori bars of tests/po2_rowdiag_bar.py, its bitwise row-independence, consistency with ppls_po2_loglik,
scores_PO2PLS and ppls_row_diagnostics, the weights, robust_PO2PLS against the loop written out, planted
outliers, rows that are not resident, shards, an open EM session, and every refusal with the outputs untouched."""
import ctypes as ct
import functools
import threading

import numpy as np
import pytest

import po2_bar
import po2_rowdiag_bar as prb
import rowdiag_bar as rb

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
FIVE = ("odx2", "ody2", "sd2", "d2", "loglik")
L = prb.L


def _ctx(dtype=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", 0)
    return c


@functools.lru_cache(maxsize=None)
def _case(*case):
    X, Y, th = prb.make_case(*case)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, th


def _check(tag, got, ref, bar, keys=prb.OUTPUTS):
    for key in keys:
        ok, ratio = prb.inside(got[key], ref[key], bar[key])
        print(f"{tag} {key}: max error / bar = {ratio:.3g}")
        assert ok, (tag, key, ratio)


def _same_bits(a, b, keys=prb.OUTPUTS):
    for key in keys:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key


def _guards_intact(out):
    """Every returned array is a view of a buffer 8 doubles longer than the library was told, NaN before the
    call: what lies past the real extent is still NaN."""
    for key, v in out.items():
        base = v.base
        assert base is not None and base.ndim == 1 and base.shape[0] == v.size + 8, key
        assert np.all(np.isnan(base[v.size:])), key


def _untouched(ctx):
    for key, b in ctx._rowdiag_last.items():
        assert np.all(np.isnan(b)), key


# ------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", prb.cases(), ids=prb.case_id)
def test_kernel_against_long_double(case, dtype):
    n, p, q, r, rx, ry, _ = case
    kx, ky, k = r + rx, r + ry, 2 * r + rx + ry
    X, Y, th = _case(*case)
    T = prb.theta_of(th)
    f32 = bool(dtype)
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        info = ctx.po2_rowdiag_info(r, rx, ry, f32)
        assert info == dict(tile_x=prb.tile_of(kx), tile_y=prb.tile_of(ky), rows_per_wave=prb.rows_per_wave(kx, ky, p, q, f32))
        Xs, Ys = ctx.get_data()                                     # the rows as stored (fp32: rounded)
        assert np.array_equal(Xs, rb.stored(X, f32)) and np.array_equal(Ys, rb.stored(Y, f32))
        ref = prb.reference(Xs, Ys, th, f32)
        bar = prb.bars(Xs, Ys, th, f32, ref)
        full = ctx.po2_row_diagnostics(T, want_mu=True)
        assert full["odx2"].shape == (n,) and full["mu"].shape == (n, k)
        assert np.all(full["sd2"] >= 0)
        _check("mu", full, ref, bar)
        _guards_intact(full)
        nomu = ctx.po2_row_diagnostics(T)
        assert set(nomu) == set(FIVE)
        _same_bits(nomu, full, FIVE)
        _guards_intact(nomu)
        _same_bits(ctx.po2_row_diagnostics(T, want_mu=True), full)  # the same call, the same bits
        rows = np.array([n - 1, 0, n // 2, 0, n - 1, 1 % n, n // 2])  # a subset, out of order and with repeats
        sub = ctx.po2_row_diagnostics(T, rows=rows, want_mu=True)
        _same_bits(sub, {key: full[key][rows] for key in prb.OUTPUTS})
        _guards_intact(sub)
        assert ctx.po2_row_diagnostics(T, rows=[], want_mu=True)["mu"].shape == (0, k)
        # the same rows as new rows: staged in fp64 whatever the context stores
        new = ctx.po2_row_diagnostics_new(T, X, Y, want_mu=True)
        _guards_intact(new)
        _same_bits(ctx.po2_row_diagnostics_new(T, np.asfortranarray(X), np.asfortranarray(Y), want_mu=True), new)
        if f32:
            ref64 = prb.reference(X, Y, th)
            _check("new", new, ref64, prb.bars(X, Y, th, False, ref64))
        else:
            _same_bits(new, full)
    i0, i1 = n // 3, n - n // 4                                     # a context that holds only rows [i0, i1)
    with _ctx(dtype) as part:
        part.set_data(X[i0:i1], Y[i0:i1])
        _same_bits(part.po2_row_diagnostics(T, want_mu=True), {key: full[key][i0:i1] for key in prb.OUTPUTS})


# ------------------------------------------------------------------------------ 2. the existing entries
CONSISTENCY = [(37, 41, 37, 2, 2, 1, True), (37, 41, 37, 4, 4, 5, False), (67, 131, 9, 5, 3, 0, False), (33, 261, 130, 3, 5, 13, True)]


@pytest.mark.parametrize("case", CONSISTENCY, ids=prb.case_id)
def test_loglik_sum_and_scores_agree_with_the_existing_entries(case):
    from ppls_amd import scores_PO2PLS
    X, Y, th = _case(*case)
    T = prb.theta_of(th)
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        full = ctx.po2_row_diagnostics(T, want_mu=True)
        assert not ctx.xprod_info()["ready"]                        # no S was read and none was formed
        ll, total = ctx.po2_loglik(T), float(full["loglik"].sum())
        ref = prb.reference(X, Y, th)
        bar = prb.bars(X, Y, th, False, ref)
        llbar = prb.loglik_sum_bar(X, Y, th, False, ref, bar)
        print(f"sum loglik {total!r} ppls_po2_loglik {ll!r} |diff| / bar = {abs(total - ll) / llbar:.3g}")
        assert abs(total - ll) <= llbar
        # scores_PO2PLS: [X Gx | Y Gy] K with the K of ppls_po2_estep, whose own error is po2_bar's e_K
        e = ctx.po2_estep(T)
        sc = scores_PO2PLS(dict(estimates=T.as_dict(), Expectations=dict(K=e.K)), ctx=ctx)
        Z = np.hstack([X, Y]).astype(L)
        S = Z.T @ Z
        p, q = X.shape[1], Y.shape[1]
        sref = po2_bar.sform(th, S, X.shape[0], p, q)
        e_K = float(po2_bar.small_bars(sref, th, X.shape[0], p, q, np.trace(S[:p, :p]), np.trace(S[p:, p:]))["K"])
        Gx, Gy = po2_bar.loadings(th)
        A = np.hstack([np.abs(X) @ np.abs(Gx), np.abs(Y) @ np.abs(Gy)])          # |x|'|G|: the size of a raw score
        own = A.sum(axis=1, keepdims=True) * e_K + float(rb.gamma(max(p, q) + A.shape[1] + 2)) * (A @ np.abs(np.asarray(sref["K"], dtype=np.float64)))
        worst = float(np.max(np.abs(full["mu"] - sc) / (bar["mu"] + own)))
        print(f"mu vs scores_PO2PLS: {worst:.3g} of the summed bars")
        assert np.all(np.abs(full["mu"] - sc) <= bar["mu"] + own)


@pytest.mark.parametrize("shape", [(37, 41, 37, 5), (67, 131, 9, 9), (6, 2051, 3, 1)], ids=str)
def test_shared_only_agrees_with_row_diagnostics(shape):
    n, p, q, r = shape
    X, Y, th = rb.make_case(n, p, q, r)
    W, C, b, t, sE, sF, sH = rb.theta_parts(th)
    th2 = dict(W=W, Wo=W[:, :0], C=C, Co=C[:, :0], B=b, sigT=t, sigTo=np.zeros(0), sigUo=np.zeros(0), sigE=sE, sigF=sF, sigH=sH)
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        old = ctx.row_diagnostics(rb.theta_of(th), want_mu=True)
        new = ctx.po2_row_diagnostics(prb.theta_of(th2), want_mu=True)
    b_old, b_new = rb.bars(X, Y, th), prb.bars(X, Y, th2)
    for key in FIVE:
        assert np.all(np.abs(old[key] - new[key]) <= b_old[key] + b_new[key]), key
    mu_old, mb = np.hstack([old["mu_T"], old["mu_U"]]), np.hstack([b_old["mu_T"], b_old["mu_U"]])
    assert np.all(np.abs(mu_old - new["mu"]) <= mb + b_new["mu"])


# ------------------------------------------------------------------------------ 3. the weights
@pytest.mark.parametrize("m", [1, 16])
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", [(37, 41, 37, 2, 2, 1, True), (67, 131, 9, 5, 3, 0, False)], ids=prb.case_id)
def test_robust_weights(case, dtype, m):
    X, Y, th = _case(*case)
    T = prb.theta_of(th)
    n, p, q = X.shape[0], X.shape[1], Y.shape[1]
    nus = 4.0 if m == 1 else np.exp(np.linspace(0.0, np.log(50.0), 16))
    keep = 0 if m == 1 else 5
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        ll, sw = ctx.po2_robust_weights(T, nus, keep)
        w, d2 = ctx.robust_get()
        assert np.array_equal(d2, ctx.po2_row_diagnostics(T)["d2"])             # the bits the diagnostics report
        ref = prb.reference(X, Y, th, bool(dtype))
        bar = prb.bars(X, Y, th, bool(dtype), ref)
        rref, rbar = prb.robust_reference(ref, th, nus, keep, p, q, n), prb.robust_bars(ref, bar, th, nus, keep, p, q, n)
        ok_w, worst_w = prb.inside(w, rref["w"], rbar["w"])
        ok_l, worst_l = prb.inside(ll, rref["loglik_t"], rbar["loglik_t"])
        print(f"err / bar  w {worst_w:.3g}  l_t {worst_l:.3g}")
        assert ok_w and ok_l
        outs = []
        for grid in (0, 1, 7):                                                   # any grid of the row pass: the same bits
            ctx.set_option("robust_grid", grid)
            outs.append(ctx.po2_robust_weights(T, nus, keep) + ctx.robust_get())
        for o in outs:
            assert np.array_equal(o[0], ll) and o[1] == sw and np.array_equal(o[2], w) and np.array_equal(o[3], d2)
        # S_u from the kept weights, with no host round trip, is S_u from their host copies
        with _ctx(dtype) as a, _ctx(dtype) as b:
            a.xprod_weighted(ctx)
            b.xprod_weighted(ctx, w)
            assert np.array_equal(a.xprod_matrix(), b.xprod_matrix()) and a.stream_info() == b.stream_info()


def test_robust_weights_refusals_leave_everything_untouched():
    from ppls_amd import PplsError
    X, Y, th = _case(37, 41, 37, 2, 2, 1, True)
    T = prb.theta_of(th)
    with _ctx() as ctx, _ctx() as streamed:
        ctx.set_data(X, Y)
        ctx.po2_robust_weights(T, 4.0)
        w0, d0 = ctx.robust_get()

        def refused(code, fn):
            with pytest.raises(PplsError) as e:
                fn()
            assert e.value.code == code
            ll, sw = ctx._robust_last                               # NaN before the call: nothing was written
            assert np.all(np.isnan(ll)) and np.all(np.isnan(sw))
            w, d = ctx.robust_get()                                 # and the kept weights survive
            assert np.array_equal(w, w0) and np.array_equal(d, d0)

        for nus, keep in ((np.ones(17), 0), (np.ones(0), 0), ([4.0, np.nan], 0), ([4.0, np.inf], 0), ([0.0], 0), ([-1.0, 4.0], 0),
                          ([4.0, 5.0], 2), ([4.0, 5.0], -1)):
            refused(E_ARG, lambda: ctx.po2_robust_weights(T, nus, keep))
        for bad in _bad_fits(th):
            refused(E_ARG, lambda: ctx.po2_robust_weights(bad[1], 4.0))
        streamed.xprod_weighted(ctx, np.ones(X.shape[0]))
        with pytest.raises(PplsError, match="streamed") as e:
            streamed.po2_robust_weights(T, 4.0)
        assert e.value.code == E_STATE


# ------------------------------------------------------------------------------ 4., 5. robust_PO2PLS
@functools.lru_cache(maxsize=None)
def _contaminated(seed=11):
    X, Y, tr, bad = prb.contaminated(seed)
    s = po2_bar.HOST_SHAPE
    Z = np.hstack([X, Y])
    th = po2_bar.cast(tr, np.float64)
    for _ in range(200):                                            # the Gaussian fit of the host test
        th = po2_bar.ecm_update(th, po2_bar.sform(th, Z.T @ Z, s["N"], s["p"], s["q"], np.float64), s["p"], np.float64)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, tr, bad, th


def _distances(a, b):
    out = {key: po2_bar.projector_distance(a[key], b[key]) for key in ("W", "Wo", "C", "Co")}
    for key in ("B", "sigT", "sigTo", "sigUo", "sigE", "sigF", "sigH"):
        x, y = (np.ravel(np.diag(v) if np.ndim(v) == 2 else v).astype(np.float64) for v in (np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64)))
        out[key] = float(np.max(np.abs(x - y) / np.abs(y)))
    return out


def test_robust_fit_equals_the_written_out_loop():
    """3 outer x 2 inner forced steps at nu = 4 from the Gaussian fit of the contaminated problem (seed 11): the
    device loop against the long-double loop, every distance within po2_bar.SLACK times the yardstick, which is
    the largest distance of the plain fp64 numpy loop from the same long-double loop.  Measured on the MI355X:
    yardstick 2.75e-15 (the numpy loop's sigH; its projector distances 1.57e-15, 7.4e-16, 1.31e-15, 5.5e-16 for
    W, Wo, C, Co); the device loop's largest distance 1.34e-15 (W; Wo 7.1e-16, C 1.14e-15, Co 8.7e-16, the
    scalars at most 7.2e-16).  The figures are printed by this test."""
    from ppls_amd import robust_PO2PLS
    X, Y, tr, bad, g = _contaminated()
    init = {key: np.array(v) if np.ndim(v) else float(v) for key, v in g.items()}
    ref, _ = prb.robust_loop(X, Y, init, 4.0, 3, 2, L)
    own, _ = prb.robust_loop(X, Y, init, 4.0, 3, 2, np.float64)
    with _ctx() as ctx:
        out = robust_PO2PLS(X, Y, 2, 2, 1, nu=4.0, outer=3, inner=2, atol=-np.inf, init=init, ctx=ctx)
    assert out["steps"] == 3 and len(out["loglik"]) == 4 and out["gaussian"] is None
    refc = po2_bar.canonical({key: np.asarray(v, dtype=np.float64) if np.ndim(v) else float(v) for key, v in ref.items()})
    d_own, d_dev = _distances(po2_bar.canonical(own), refc), _distances(out["estimates"], refc)
    yard = max(d_own.values())
    print(f"yardstick (fp64 numpy loop, largest distance) {yard:.3g}")
    for key in d_dev:
        print(f"  {key}: device {d_dev[key]:.3g}  numpy {d_own[key]:.3g}")
    for key in d_dev:
        assert d_dev[key] <= float(po2_bar.SLACK) * yard, (key, d_dev[key], yard)


def test_robust_fit_default_run_recovers():
    from ppls_amd import robust_PO2PLS
    X, Y, tr, bad, _ = _contaminated()
    with _ctx() as ctx:
        out = robust_PO2PLS(X, Y, 2, 2, 1, ctx=ctx, rng=np.random.default_rng(5))
    e, w = out["estimates"], out["weights"]
    good = np.setdiff1d(np.arange(X.shape[0]), bad)
    dg, dr = po2_bar.projector_distance(out["gaussian"]["estimates"]["W"], tr["W"]), po2_bar.projector_distance(e["W"], tr["W"])
    print(f"gaussian {dg:.3f} robust {dr:.3f} sigE {e['sigE']:.4f} planted {w[bad].max():.3f} others {np.median(w[good]):.3f} "
          f"steps {out['steps']} converged {out['converged']}")
    assert dg >= 0.9 and dr <= 0.35 and 0.45 <= e["sigE"] <= 0.55
    assert np.all(w[bad] <= 0.1) and 0.9 <= np.median(w[good]) <= 1.1
    assert np.all(np.diff(out["loglik"])[:-1] > 0)


# ------------------------------------------------------------------------------ 6. planted outliers
def test_planted_outliers():
    from ppls_amd import diagnostics_PO2PLS
    X, Y, th, planted = prb.planted()
    n, p, q, kx, ky = 203, 37, 21, 4, 3
    with _ctx() as ctx:
        out = diagnostics_PO2PLS(dict(estimates=th), X, Y, ctx=ctx, alpha=0.01)
        bon = diagnostics_PO2PLS(th, ctx=ctx, alpha=0.01, adjust="bonferroni")
        sub = diagnostics_PO2PLS(prb.theta_of(th), ctx=ctx, subset=[150, 5], want_mu=True)
    ref = prb.reference(X, Y, th)
    _check("planted", out, ref, prb.bars(X, Y, th, False, ref), FIVE)
    assert out["df"] == dict(odx2=p - kx, ody2=q - ky, sd2=kx + ky, d2=p + q)
    for key, row in planted.items():
        pv = out["pvalue"][key]
        print(f"{key}: row {row} p = {pv[row]:.3g}, the nearest other row {np.delete(pv, row).min():.3g}")
        assert int(np.argmin(pv)) == row and pv[row] < 1e-8 and np.delete(pv, row).min() > 1e-6
        assert np.array_equal(out["flag"][key], pv < 0.01) and np.array_equal(bon["flag"][key], bon["pvalue"][key] < 0.01 / n)
    assert set(out["outliers"][:3]) == {5, 77, 150} and set(bon["outliers"][:3]) == {5, 77, 150}
    for key in FIVE:
        assert np.array_equal(sub[key], out[key][[150, 5]])
    assert sub["mu"].shape == (2, kx + ky)


# ------------------------------------------------------------------------------ 7. other contexts
def test_streamed_second_pass_and_state_refusal():
    from ppls_amd import PplsError, diagnostics_PO2PLS, stream_data
    case = (67, 41, 37, 4, 4, 5, False)
    X, Y, th = _case(*case)
    n, p, q = case[:3]
    T = prb.theta_of(th)
    Xr = X * (0.5 + np.arange(p) % 7) + (np.arange(p) % 5 - 2) * 0.7         # loaded units: scale and centre matter
    Yr = Y * (0.5 + np.arange(q) % 3) + (np.arange(q) % 4 - 1) * 1.3
    chunks = [(0, 30), (30, 31), (31, n)]
    with _ctx() as sc, _ctx() as res:
        stream_data([(Xr[lo:hi], Yr[lo:hi]) for lo, hi in chunks], center=True, scale=True, ctx=sc)
        res.set_data(Xr, Yr)
        res.scale_data()
        want = diagnostics_PO2PLS(T, ctx=res, want_mu=True)
        parts = [diagnostics_PO2PLS(T, Xr[lo:hi], Yr[lo:hi], ctx=sc, new=True, rescale=True, want_mu=True) for lo, hi in chunks]
        got = {key: np.concatenate([part[key] for part in parts]) for key in prb.OUTPUTS}
        Xs, Ys = res.get_data()
        s = sc.scaling()
        dX = rb.rescale_perturbation(Xr, s["centerX"], s["scaleX"], n)
        dY = rb.rescale_perturbation(Yr, s["centerY"], s["scaleY"], n)
        ref = prb.reference(Xs, Ys, th)
        bar0, bar1 = prb.bars(Xs, Ys, th, False, ref), prb.bars(Xs, Ys, th, False, ref, dX=dX, dY=dY)
        _check("resident, scaled", want, ref, bar0)
        _check("streamed context, host rescale", got, ref, bar1)
        for key in prb.OUTPUTS:
            assert np.all(np.abs(got[key] - want[key]) <= bar0[key] + bar1[key]), key
        with pytest.raises(PplsError, match="streamed") as e:      # the resident entry has no rows to read
            sc.po2_row_diagnostics(T, want_mu=True)
        assert e.value.code == E_STATE
        _untouched(sc)


def test_two_shards_are_slices_of_one_context():
    from test_gpu_stream import ThreadAllReduce
    case = (67, 131, 9, 5, 3, 0, False)
    X, Y, th = _case(*case)
    n = case[0]
    T = prb.theta_of(th)
    with _ctx() as one:
        one.set_data(X, Y)
        full = one.po2_row_diagnostics(T, want_mu=True)
    shares = [(0, 29), (29, n)]
    red = ThreadAllReduce(2)
    out, errs = [None] * 2, []

    def body(rank):
        try:
            lo, hi = shares[rank]
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.set_data(X[lo:hi], Y[lo:hi], n_total=n)
                out[rank] = c.po2_row_diagnostics(T, want_mu=True)  # no collective: each rank's own rows
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
    if errs:
        raise errs[0]
    for rank, (lo, hi) in enumerate(shares):
        _same_bits(out[rank], {key: full[key][lo:hi] for key in prb.OUTPUTS})


def test_an_open_em_session_continues_bitwise_and_no_s_is_formed():
    import ppls_amd as pa
    from conftest import make_problem
    X, Y, t0 = make_problem(300, 37, 12, 3, seed=5)
    th = pa.Theta(t0["W"], t0["C"], t0["B"], t0["sigE"], t0["sigF"], t0["sigH"], t0["sigT"])
    T = prb.theta_of(po2_bar.make_theta(np.random.default_rng(3), 37, 12, 2, 2, 1, orthonormal=False, scale=2.0))

    def state(c):
        est, ll = c.em_state()[:2]
        return [est.W.copy(), est.C.copy(), est.B.copy(), est.sigT.copy(), np.array([est.sigE, est.sigF, est.sigH]), np.array(ll)]

    with _ctx() as c:
        c.set_data(X, Y)
        c.em_begin(th)
        c.em_iterate(6)
        want = state(c)
    with _ctx() as c:
        c.set_data(X, Y)
        c.em_begin(th)
        c.em_iterate(3)
        before = c.get_data()
        c.po2_row_diagnostics(T, want_mu=True)
        c.po2_row_diagnostics_new(T, X[:7], Y[:7])
        c.po2_robust_weights(T, [3.0, 4.0], 1)
        assert not c.xprod_info()["ready"]                          # a context with no S still has none
        after = c.get_data()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        c.em_iterate(3)
        got = state(c)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------ 8. refusals
def _bad_fits(th):
    from ppls_amd import Po2Theta

    def theta(**kw):
        d = {key: np.array(v, dtype=np.float64, copy=True) for key, v in th.items()}
        d.update(kw)
        return Po2Theta.from_dict(d)

    p, q = th["W"].shape[0], th["C"].shape[0]
    rng = np.random.default_rng(1)
    nanW, infCo = th["W"].copy(), th["Co"].copy()
    nanW[3, 1], infCo[0, 0] = np.nan, np.inf
    dupWo = th["Wo"].copy()
    dupWo[:, 1] = th["W"][:, 0] * 2.0                               # [W Wo] has two parallel columns
    dupCo = th["C"][:, :1] - th["C"][:, 1:2]                        # Co in the span of C
    wide = Po2Theta(rng.standard_normal((p, 9)), rng.standard_normal((p, 8)), rng.standard_normal((q, 9)), np.zeros((q, 0)),
                    np.ones(9), np.ones(9), np.ones(8), (), 0.3, 0.4, 0.2)                   # r + rx = 17
    tiny = 1e-200
    return [("r + rx above 16", wide), ("NaN in W", theta(W=nanW)), ("Inf in Co", theta(Co=infCo)),
            ("NaN in B", theta(B=np.array([np.nan, 1.0]))), ("Inf in sigTo", theta(sigTo=np.array([np.inf, 1.0]))),
            ("sigE = 0", theta(sigE=0.0)), ("sigF < 0", theta(sigF=-0.4)), ("NaN sigH", theta(sigH=np.nan)),
            ("sigUo = 0", theta(sigUo=np.array([0.0]))), ("rank-deficient [W Wo]", theta(Wo=dupWo)),
            ("rank-deficient [C Co]", theta(Co=dupCo)),
            ("Sigma_c underflows to 0", theta(sigE=tiny, sigF=tiny, sigH=tiny, sigT=np.full(2, tiny), sigTo=np.full(2, tiny),
                                              sigUo=np.full(1, tiny)))]


def test_refusals_leave_the_outputs_untouched():
    from ppls_amd import PplsError, Po2Theta
    case = (37, 41, 37, 2, 2, 1, True)
    X, Y, th = _case(*case)
    n, p, q, r, rx, ry = case[:6]
    T = prb.theta_of(th)
    with _ctx() as ctx, _ctx() as narrow:
        ctx.set_data(X, Y)
        narrow.set_data(X[:, :5], Y[:, :3])
        for what, bad in _bad_fits(th):
            for call in (lambda: ctx.po2_row_diagnostics(bad, want_mu=True), lambda: ctx.po2_row_diagnostics_new(bad, X, Y, want_mu=True)):
                with pytest.raises(PplsError) as e:
                    call()
                assert e.value.code == E_ARG, what
                _untouched(ctx)
        few = Po2Theta(th["W"][:5], th["Wo"][:5], th["C"][:3], th["Co"][:3], th["B"], th["sigT"], th["sigTo"], th["sigUo"], 0.3, 0.4, 0.2)
        for call in (lambda: narrow.po2_row_diagnostics(few, want_mu=True),      # r + ry = 3 fits q = 3, r + rx = 4 fits p = 5 ..
                     lambda: narrow.po2_row_diagnostics_new(few, X[:, :5], Y[:, :3], want_mu=True)):
            call()                                                               # .. and is served
        narrow.set_data(X[:, :3], Y[:, :3])                                      # r + rx = 4 > p = 3
        few = Po2Theta(th["W"][:3], th["Wo"][:3], th["C"][:3], th["Co"][:3], th["B"], th["sigT"], th["sigTo"], th["sigUo"], 0.3, 0.4, 0.2)
        for call in (lambda: narrow.po2_row_diagnostics(few, want_mu=True),
                     lambda: narrow.po2_row_diagnostics_new(few, X[:, :3], Y[:, :3], want_mu=True)):
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_ARG
            _untouched(narrow)
        for rows in ([0, n], [-1], [3, 2, 10 ** 12]):
            with pytest.raises(PplsError, match="outside") as e:
                ctx.po2_row_diagnostics(T, rows=rows, want_mu=True)
            assert e.value.code == E_ARG
            _untouched(ctx)
        # NULL data with n > 0, a NULL theta or loading, a bad layout, sizes the theta does not have
        k = 2 * r + rx + ry
        bufs, s = ctx._po2_rowdiag_out(3, k, True)
        t = T.struct()
        Xc, Yc = np.ascontiguousarray(X), np.ascontiguousarray(Y)
        dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))   # noqa: E731
        new, res = ctx._L.ppls_po2_row_diagnostics_new, ctx._L.ppls_po2_row_diagnostics
        assert new(ctx.h, ct.byref(t), r, rx, ry, None, dp(Yc), 3, 1, ct.byref(s)) == E_ARG
        assert new(ctx.h, ct.byref(t), r, rx, ry, dp(Xc), None, 3, 1, ct.byref(s)) == E_ARG
        assert new(ctx.h, ct.byref(t), r, rx, ry, dp(Xc), dp(Yc), -1, 1, ct.byref(s)) == E_ARG
        assert new(ctx.h, ct.byref(t), r, rx, ry, dp(Xc), dp(Yc), 3, 2, ct.byref(s)) == E_ARG
        assert new(ctx.h, None, r, rx, ry, dp(Xc), dp(Yc), 3, 1, ct.byref(s)) == E_ARG
        assert res(ctx.h, None, r, rx, ry, None, 3, ct.byref(s)) == E_ARG
        assert res(ctx.h, ct.byref(t), 0, rx, ry, None, 3, ct.byref(s)) == E_ARG
        assert res(ctx.h, ct.byref(t), r, -1, ry, None, 3, ct.byref(s)) == E_ARG
        noWo = T.struct()
        noWo.Wo = None
        assert res(ctx.h, ct.byref(noWo), r, rx, ry, None, 3, ct.byref(s)) == E_ARG
        assert new(ctx.h, ct.byref(noWo), r, rx, ry, dp(Xc), dp(Yc), 3, 1, ct.byref(s)) == E_ARG
        _untouched(ctx)
        for blk, val in ((0, np.nan), (1, np.inf), (1, -np.inf)):               # non-finite new rows: the whole call
            Xb, Yb = X.copy(), Y.copy()
            (Yb if blk else Xb)[n - 1, 2] = val
            with pytest.raises(PplsError, match="NaN or Inf") as e:
                ctx.po2_row_diagnostics_new(T, Xb, Yb, want_mu=True)
            assert e.value.code == E_ARG
            _untouched(ctx)
        with pytest.raises(ValueError, match="columns"):
            ctx.po2_row_diagnostics_new(T, X[:, :-1], Y)
        info = ctx._L.ppls_po2_rowdiag_info
        assert info(p, q, 0, 9, 8, 0, None, None, None) == E_ARG and info(p, q, 0, 0, 0, 0, None, None, None) == E_ARG
        # and the context still works
        ref = prb.reference(X, Y, th)
        _check("after the refusals", ctx.po2_row_diagnostics(T, want_mu=True), ref, prb.bars(X, Y, th, False, ref))


def test_timing_entry():
    X, Y, th = _case(37, 41, 37, 2, 2, 1, True)
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        t = ctx.po2_rowdiag_timing(prb.theta_of(th), reps=2)
        assert t["ms"] > 0 and t["ms_mu"] > 0
