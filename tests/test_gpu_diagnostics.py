"""Row diagnostics on the device: the kernel against long double inside the a-priori bars of
tests/rowdiag_bar.py, its bitwise row-independence, consistency with ppls_loglik and ppls_estep, planted
outliers, rows that are not resident, shards, and every refusal with the outputs untouched."""
import ctypes as ct
import functools
import threading

import numpy as np
import pytest

import rowdiag_bar as rb

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
FIVE = ("odx2", "ody2", "sd2", "d2", "loglik")


def _ctx(dtype=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", 0)
    return c


@functools.lru_cache(maxsize=None)
def _case(n, p, q, r):
    X, Y, th = rb.make_case(n, p, q, r)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, th


def _check(tag, got, ref, bar, keys=rb.OUTPUTS):
    for key in keys:
        ok, ratio = rb.inside(got[key], ref[key], bar[key])
        print(f"{tag} {key}: max error / bar = {ratio:.3g}")
        assert ok, (tag, key, ratio)


def _same_bits(a, b, keys=rb.OUTPUTS):
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
@pytest.mark.parametrize("shape", rb.cases(), ids=lambda s: "n%d_p%d_q%d_r%d" % s)
def test_kernel_against_long_double(shape, dtype):
    n, p, q, r = shape
    X, Y, th = _case(*shape)
    T = rb.theta_of(th)
    f32 = bool(dtype)
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        Xs, Ys = ctx.get_data()                                     # the rows as stored (fp32: rounded)
        assert np.array_equal(Xs, rb.stored(X, f32)) and np.array_equal(Ys, rb.stored(Y, f32))
        ref, bar = rb.reference(Xs, Ys, th, f32), rb.bars(Xs, Ys, th, f32)
        full = ctx.row_diagnostics(T, want_mu=True)
        assert full["odx2"].shape == (n,) and full["mu_T"].shape == (n, r)
        _check("mu", full, ref, bar)
        _guards_intact(full)
        nomu = ctx.row_diagnostics(T)
        assert set(nomu) == set(FIVE)
        _check("no mu", nomu, ref, bar, FIVE)
        _guards_intact(nomu)
        _same_bits(ctx.row_diagnostics(T, want_mu=True), full)      # the same call, the same bits
        # a subset, out of order and with repeats: every row as in the full call
        rows = np.array([n - 1, 0, n // 2, 0, n - 1, 1 % n, n // 2])
        sub = ctx.row_diagnostics(T, rows=rows, want_mu=True)
        _same_bits(sub, {k: full[k][rows] for k in rb.OUTPUTS})
        _guards_intact(sub)
        _same_bits(ctx.row_diagnostics(T, rows=[n // 2]), {k: full[k][[n // 2]] for k in FIVE}, FIVE)
        assert ctx.row_diagnostics(T, rows=[], want_mu=True)["mu_U"].shape == (0, r)
        # consistency with the existing entries
        ll, total = ctx.loglik(T), float(full["loglik"].sum())
        llbar = rb.loglik_sum_bar(Xs, Ys, th, f32)
        print(f"sum loglik {total!r} ppls_loglik {ll!r} |diff| / bar = {abs(total - ll) / llbar:.3g}")
        assert abs(total - ll) <= llbar
        e = ctx.estep(T)
        bT, bU = rb.estep_mu_bar(Xs, Ys, th, f32)
        print(f"mu vs estep: {float((np.abs(full['mu_T'] - e.mu_T) / bT).max()):.3g} "
              f"{float((np.abs(full['mu_U'] - e.mu_U) / bU).max()):.3g} of the bar")
        assert np.all(np.abs(full["mu_T"] - e.mu_T) <= bT) and np.all(np.abs(full["mu_U"] - e.mu_U) <= bU)
        # the same rows as new rows: staged in fp64 whatever the context stores
        new = ctx.row_diagnostics_new(T, X, Y, want_mu=True)
        _guards_intact(new)
        newF = ctx.row_diagnostics_new(T, np.asfortranarray(X), np.asfortranarray(Y), want_mu=True)
        _same_bits(newF, new)                                       # either layout
        if f32:
            _check("new", new, rb.reference(X, Y, th), rb.bars(X, Y, th))
        else:
            _same_bits(new, full)
    # a context that holds only rows [i0, i1) of the same data
    i0, i1 = n // 3, n - n // 4
    with _ctx(dtype) as part:
        part.set_data(X[i0:i1], Y[i0:i1])
        _same_bits(part.row_diagnostics(T, want_mu=True), {k: full[k][i0:i1] for k in rb.OUTPUTS})


def test_no_local_rows():
    X, Y, th = _case(3, 5, 3, 1)
    T = rb.theta_of(th)
    with _ctx() as ctx:
        ctx.set_data(np.zeros((0, 5)), np.zeros((0, 3)))
        out = ctx.row_diagnostics(T, want_mu=True)
        assert all(out[k].shape == (0,) for k in FIVE) and out["mu_T"].shape == (0, 1) and out["mu_U"].shape == (0, 1)
        _guards_intact(out)
        # the shape alone serves new rows
        new = ctx.row_diagnostics_new(T, X, Y, want_mu=True)
        _check("new on an empty context", new, rb.reference(X, Y, th), rb.bars(X, Y, th))
        assert ctx.row_diagnostics_new(T, X[:0], Y[:0])["d2"].shape == (0,)


# ------------------------------------------------------------------------------ 2. planted outliers
def test_planted_outliers():
    from ppls_amd import diagnostics_PPLS
    from ppls_amd.api import diagnostics_summary
    X, Y, th, planted = rb.planted()
    n, p, q, r = 203, 37, 21, 3
    fit = dict(estimates=th)
    alpha = 0.01
    with _ctx() as ctx:
        out = diagnostics_PPLS(fit, X, Y, ctx=ctx, alpha=alpha)
        bon = diagnostics_PPLS(fit, ctx=ctx, alpha=alpha, adjust="bonferroni")
        sub = diagnostics_PPLS(fit, ctx=ctx, subset=[150, 5], want_mu=True)
    ref, bar = rb.reference(X, Y, th), rb.bars(X, Y, th)
    _check("planted", out, ref, bar, FIVE)
    f64 = {k: np.asarray(ref[k], dtype=np.float64) for k in ("odx2", "ody2", "sd2", "d2")}
    want = diagnostics_summary(f64, p, q, r, th["sigE"], th["sigF"], alpha=alpha)
    assert out["df"] == want["df"] == dict(odx2=p - r, ody2=q - r, sd2=2 * r, d2=p + q)
    scale = dict(odx2=th["sigE"] ** 2, ody2=th["sigF"] ** 2, sd2=1.0, d2=1.0)
    for key in ("odx2", "ody2", "sd2", "d2"):
        pv = out["pvalue"][key]
        assert pv.shape == (n,) and np.all(np.isfinite(pv)) and np.all((pv >= 0) & (pv <= 1))
        pbar = rb.pvalue_bar(f64[key] / scale[key], want["df"][key], bar[key] / scale[key])
        for level, got in ((alpha, out), (alpha / n, bon)):
            decided = np.abs(want["pvalue"][key] - level) > pbar
            print(f"{key} at {level:.3g}: {int(decided.sum())} of {n} rows decided, {int(got['flag'][key].sum())} flagged")
            assert decided.sum() >= n - 2
            assert np.array_equal(got["flag"][key][decided], (want["pvalue"][key] < level)[decided])
            assert np.array_equal(got["flag"][key], got["pvalue"][key] < level)
    for key, row in planted.items():
        pv = out["pvalue"][key]
        print(f"{key}: row {row} p = {pv[row]:.3g}, the nearest other row {np.delete(pv, row).min():.3g}")
        assert int(np.argmin(pv)) == row and pv[row] < 1e-12 and np.delete(pv, row).min() > 1e-6
    assert set(out["outliers"][:3]) == {5, 77, 150} and set(bon["outliers"][:3]) == {5, 77, 150}
    assert np.all(np.diff(out["pvalue"]["d2"][out["outliers"]]) >= 0) and np.all(out["flag"]["d2"][out["outliers"]])
    for key in FIVE:
        assert np.array_equal(sub[key], out[key][[150, 5]])
    assert sub["mu_T"].shape == (2, r) and list(sub["outliers"]) in ([0, 1], [1, 0])


# ------------------------------------------------------------------------------ 3. rows that are not resident
def test_streamed_second_pass_and_state_refusal():
    from ppls_amd import PplsError, diagnostics_PPLS, stream_data
    n, p, q, r = 67, 41, 37, 5
    X, Y, th = _case(n, p, q, r)
    T = rb.theta_of(th)
    Xr = X * (0.5 + np.arange(p) % 7) + (np.arange(p) % 5 - 2) * 0.7         # loaded units: scale and centre matter
    Yr = Y * (0.5 + np.arange(q) % 3) + (np.arange(q) % 4 - 1) * 1.3
    chunks = [(0, 30), (30, 31), (31, n)]
    with _ctx() as sc, _ctx() as res:
        stream_data([(Xr[lo:hi], Yr[lo:hi]) for lo, hi in chunks], center=True, scale=True, ctx=sc)
        res.set_data(Xr, Yr)
        res.scale_data()
        want = diagnostics_PPLS(T, ctx=res, want_mu=True)
        parts = [diagnostics_PPLS(T, Xr[lo:hi], Yr[lo:hi], ctx=sc, new=True, rescale=True, want_mu=True) for lo, hi in chunks]
        got = {k: np.concatenate([part[k] for part in parts]) for k in rb.OUTPUTS}
        assert parts[1]["d2"].shape == (1,) and sc.streamed
        Xs, Ys = res.get_data()                                     # the rows as the resident context holds them
        s = sc.scaling()
        dX = rb.rescale_perturbation(Xr, s["centerX"], s["scaleX"], n)
        dY = rb.rescale_perturbation(Yr, s["centerY"], s["scaleY"], n)
        ref, bar0, bar1 = rb.reference(Xs, Ys, th), rb.bars(Xs, Ys, th), rb.bars(Xs, Ys, th, dX=dX, dY=dY)
        _check("resident, scaled", want, ref, bar0)
        _check("streamed context, host rescale", got, ref, bar1)
        for key in rb.OUTPUTS:
            assert np.all(np.abs(got[key] - want[key]) <= bar0[key] + bar1[key]), key
        # the resident entry has no rows to read
        with pytest.raises(PplsError, match="streamed") as e:
            sc.row_diagnostics(T, want_mu=True)
        assert e.value.code == E_STATE
        _untouched(sc)
        with pytest.raises(PplsError) as e:
            diagnostics_PPLS(T, ctx=sc)
        assert e.value.code == E_STATE


# ------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_outputs_untouched():
    from ppls_amd import PplsError, Theta
    n, p, q, r = 37, 41, 37, 5
    X, Y, th = _case(n, p, q, r)

    def theta(**kw):
        d = {k: np.array(v, dtype=np.float64, copy=True) for k, v in th.items()}
        d.update(kw)
        return Theta(d["W"], d["C"], d["B"], d["sigE"], d["sigF"], d["sigH"], d["sigT"])

    def wide(k):                                           # k components: orthonormal columns, unit scalars
        rng = np.random.default_rng(k)
        return Theta(np.linalg.qr(rng.standard_normal((p, k)))[0], np.linalg.qr(rng.standard_normal((q, k)))[0],
                     np.ones(k), 0.3, 0.4, 0.2, np.ones(k))

    nanW, infC = th["W"].copy(), th["C"].copy()
    nanW[3, 1], infC[0, 0] = np.nan, np.inf
    nanB, infT = np.diag(th["B"]).copy(), np.diag(th["sigT"]).copy()
    nanB[2], infT[0] = np.nan, np.inf
    bad_fits = [("r above PPLS_RMAX", wide(17)), ("NaN in W", theta(W=nanW)), ("Inf in C", theta(C=infC)),
                ("NaN in B", theta(B=nanB)), ("Inf in sigT", theta(sigT=infT)), ("sigE = 0", theta(sigE=0.0)),
                ("sigF < 0", theta(sigF=-0.4)), ("NaN sigH", theta(sigH=np.nan)),
                ("det underflows to 0", theta(sigE=1e-200, sigF=1e-200, sigH=0.0, sigT=np.full(r, 1e-100)))]
    T = rb.theta_of(th)
    with _ctx() as ctx, _ctx() as narrow:
        ctx.set_data(X, Y)
        narrow.set_data(X[:, :5], Y[:, :3])
        for what, bad in bad_fits:
            for call in (lambda: ctx.row_diagnostics(bad, want_mu=True), lambda: ctx.row_diagnostics_new(bad, X, Y, want_mu=True)):
                with pytest.raises(PplsError) as e:
                    call()
                assert e.value.code == E_ARG, what
                _untouched(ctx)
        few = Theta(th["W"][:5, :4], th["C"][:3, :4], np.ones(4), 0.3, 0.4, 0.2, np.ones(4))   # r = 4 > min(p, q) = 3
        for call in (lambda: narrow.row_diagnostics(few, want_mu=True),
                     lambda: narrow.row_diagnostics_new(few, X[:, :5], Y[:, :3], want_mu=True)):
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_ARG
            _untouched(narrow)
        for rows in ([0, n], [-1], [3, 2, 10 ** 12]):
            with pytest.raises(PplsError, match="outside") as e:
                ctx.row_diagnostics(T, rows=rows, want_mu=True)
            assert e.value.code == E_ARG
            _untouched(ctx)
        # NULL data with n > 0, NULL indices with nrows > 0 are "all rows", a NULL theta, a bad layout
        bufs, s = ctx._rowdiag_out(3, r, True)
        t = T.struct()
        Xc, Yc = np.ascontiguousarray(X), np.ascontiguousarray(Y)
        dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))   # noqa: E731
        assert ctx._L.ppls_row_diagnostics_new(ctx.h, ct.byref(t), r, None, dp(Yc), 3, 1, ct.byref(s)) == E_ARG
        assert ctx._L.ppls_row_diagnostics_new(ctx.h, ct.byref(t), r, dp(Xc), None, 3, 1, ct.byref(s)) == E_ARG
        assert ctx._L.ppls_row_diagnostics_new(ctx.h, ct.byref(t), r, dp(Xc), dp(Yc), -1, 1, ct.byref(s)) == E_ARG
        assert ctx._L.ppls_row_diagnostics_new(ctx.h, ct.byref(t), r, dp(Xc), dp(Yc), 3, 2, ct.byref(s)) == E_ARG
        assert ctx._L.ppls_row_diagnostics_new(ctx.h, None, r, dp(Xc), dp(Yc), 3, 1, ct.byref(s)) == E_ARG
        assert ctx._L.ppls_row_diagnostics(ctx.h, None, r, None, 3, ct.byref(s)) == E_ARG
        assert ctx._L.ppls_row_diagnostics(ctx.h, ct.byref(t), 0, None, 3, ct.byref(s)) == E_ARG
        _untouched(ctx)
        # non-finite new rows: the whole call
        for blk, val in ((0, np.nan), (1, np.inf), (1, -np.inf)):
            Xb, Yb = X.copy(), Y.copy()
            (Yb if blk else Xb)[n - 1, 2] = val
            with pytest.raises(PplsError, match="NaN or Inf") as e:
                ctx.row_diagnostics_new(T, Xb, Yb, want_mu=True)
            assert e.value.code == E_ARG
            _untouched(ctx)
        with pytest.raises(ValueError, match="columns"):
            ctx.row_diagnostics_new(T, X[:, :-1], Y)
        # and the context still works
        _check("after the refusals", ctx.row_diagnostics(T, want_mu=True), rb.reference(X, Y, th), rb.bars(X, Y, th))


def test_python_refusals():
    from ppls_amd import PPLS, diagnostics_PPLS
    X, Y, th = _case(37, 41, 37, 5)
    with _ctx() as ctx:
        seq = PPLS(X, Y, 2, 5, 1e-4, "equal", ctx=ctx)
        with pytest.raises(ValueError, match="PPLS_simult"):
            diagnostics_PPLS(seq, ctx=ctx)
        with pytest.raises(ValueError, match="columns"):
            diagnostics_PPLS(dict(estimates=th), X[:, :40], Y, ctx=ctx)
        with pytest.raises(ValueError, match="columns"):
            diagnostics_PPLS(dict(estimates=th), X, Y[:, :3], ctx=ctx, new=True)
        with pytest.raises(ValueError, match="adjust"):
            diagnostics_PPLS(dict(estimates=th), ctx=ctx, adjust="holm")


# ------------------------------------------------------------------------------ 5. two shards
def test_two_shards_are_slices_of_one_context():
    from test_gpu_stream import ThreadAllReduce
    n, p, q, r = 67, 131, 9, 9
    X, Y, th = _case(n, p, q, r)
    T = rb.theta_of(th)
    with _ctx() as one:
        one.set_data(X, Y)
        full = one.row_diagnostics(T, want_mu=True)
    shares = [(0, 29), (29, n)]
    red = ThreadAllReduce(2)
    out, errs = [None] * 2, []

    def body(rank):
        try:
            lo, hi = shares[rank]
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.set_data(X[lo:hi], Y[lo:hi], n_total=n)
                out[rank] = c.row_diagnostics(T, want_mu=True)      # no collective: each rank's own rows
                if rank == 1:
                    out.append(c.row_diagnostics(T, rows=[hi - lo - 1, 0]))
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
        _same_bits(out[rank], {k: full[k][lo:hi] for k in rb.OUTPUTS})
    _same_bits(out[2], {k: full[k][[n - 1, 29]] for k in FIVE}, FIVE)


def test_timing_entry():
    X, Y, th = _case(37, 41, 37, 5)
    from ppls_amd import PplsError
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        t = ctx.rowdiag_timing(5, reps=2)
        assert t["ms"] > 0 and t["ms_mu"] > 0
        with pytest.raises(PplsError) as e:
            ctx.rowdiag_timing(38)
        assert e.value.code == E_ARG
