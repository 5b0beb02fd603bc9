"""Batched PO2PLS fits, prediction and cross-validation over (r, rx, ry) on the GPU: the batched
statistics pass and the batched EM loop bit for bit against the single-model entries, a failing model, side
effects, refusals, the cross-validation entry against the loop written out, the held-out error against the
rows, resident against streamed, predict_PO2PLS against the dense conditional mean, the choice end to end
and two ranks."""
import functools
import threading

import numpy as np
import pytest

import cv_bar
import po2_bar as B
import po2_cv_bar as CV
from sweep_bar import LD, U
from test_cv_stream_host import K_SSE, sse_bar
from test_gpu_po2 import _as_bar_theta, _ctx, _padded_G, _padded_S, _theta

pytestmark = pytest.mark.gpu

E_ARG, E_NUMERIC, E_STATE = -1, -3, -4
SENT = -7.25e77
FIELDS = ("W", "Wo", "C", "Co", "B", "sigT", "sigTo", "sigUo")


def _same_theta(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in FIELDS) and \
        (a.sigE, a.sigF, a.sigH) == (b.sigE, b.sigF, b.sigH)


@functools.lru_cache(maxsize=None)
def _problem(kind):
    """(X, Y) read-only: 'recovery' is seed 0 of po2_bar's problem (N = 400, p = 13, q = 9, truth (2, 2, 1));
    'odd' has p = 37, q = 21 (odd padding), N = 300, truth (8, 8, 3)."""
    if kind == "recovery":
        X, Y, _ = B.host_problem(0)
    else:
        from ppls_amd import simulate_PO2PLS
        tr = B.make_theta(np.random.default_rng(41), 37, 21, 8, 8, 3)
        X, Y = simulate_PO2PLS(300, tr["W"], tr["C"], tr["Wo"], tr["Co"], tr["B"], tr["sigE"], tr["sigF"], tr["sigH"],
                               tr["sigT"], tr["sigTo"], tr["sigUo"], np.random.default_rng(42))
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


MODELS = {   # (r, rx, ry, start seed): shapes differ and repeat; 'odd' has a candidate with r + rx = 16
    "recovery": [(2, 2, 1, 16), (2, 0, 0, 3), (1, 2, 1, 4), (2, 2, 1, 5), (2, 0, 1, 6), (1, 0, 0, 7), (2, 2, 0, 8)],
    "odd": [(8, 8, 3, 1), (3, 2, 1, 2), (1, 0, 0, 3), (3, 2, 1, 4)],
}


def _starts(kind):
    X, Y = _problem(kind)
    D = np.hstack([X, Y])
    S, N = D.T @ D, float(X.shape[0])
    return [B.start_theta(S, N, X.shape[1], Y.shape[1], r, rx, ry, seed) for r, rx, ry, seed in MODELS[kind]], S, N


# ------------------------------------------------------------------------------- 1. the batched pass
@pytest.mark.parametrize("p,q,widths", [(13, 9, [(4, 3), (2, 2), (13, 9), (3, 2), (1, 1)]),
                                        (37, 21, [(4, 3), (2, 2), (16, 11), (5, 6), (3, 2), (1, 1)])])
def test_batched_pass_equals_the_single_pass_bitwise(p, q, widths):
    """M, Q and G'G of every model from the shared panel launches (chunks of 16 columns; sum kx = 23 / 31 is no
    multiple of 16 and the third model's columns straddle the first chunk boundary on both sides) are the bits
    of ppls_po2_stats on that model alone, at every rows-per-wave: the panel's output does not depend, column by
    column, on the width or the rows per wave it is launched at.  One model also against the long-double pass."""
    rng = np.random.default_rng(7 * p + q)
    D = rng.standard_normal((300, p + q))
    S = D.T @ D
    Sp, ldx, ldy, live = _padded_S(S, p, q)
    Gs = [(rng.standard_normal((p, kx)), rng.standard_normal((q, ky))) for kx, ky in widths]
    assert sum(kx for kx, _ in widths) % 16 != 0 and widths[0][0] + widths[1][0] < 16 < sum(kx for kx, _ in widths[:3])
    with _ctx() as c:
        got = c.po2_stats_batch([_padded_G(gx, ldx) for gx, _ in Gs], [_padded_G(gy, ldy) for _, gy in Gs], Sp)
        for j, (gx, gy) in enumerate(Gs):
            for rw in (0, 1, 2, 4):
                one = c.po2_stats(_padded_G(gx, ldx), _padded_G(gy, ldy), Sp, rw=rw)
                for name, a, b in zip(("M", "Q", "GGx", "GGy"), got[j], one):
                    assert np.array_equal(a, b), (j, rw, name)
        M, Q, GGx, GGy = got[2]
        r = B.PassReference(S, p, q, *Gs[2]).ratios(M[live], Q, GGx, GGy)
        print(f"p={p} q={q} model 2: err / bar {r}")
        assert max(r.values()) <= 1.0, r


# ------------------------------------------------------------------- 2. the batch against single runs
def _singles(c, ths, steps, atol, type_):
    return [c.po2_em_run(_theta(t), steps, atol, type_=type_, want_eout=False) for t in ths]


def _assert_batch_equals_singles(batch, singles, skip=()):
    ests, lls, negs, status = batch
    for j, (est, ll, _, neg) in enumerate(singles):
        if j in skip:
            continue
        assert status[j] == 0
        assert len(lls[j]) == len(ll) and np.array_equal(lls[j], ll), j
        assert _same_theta(ests[j], est), j
        assert negs[j] == neg


@pytest.mark.parametrize("type_code", [0, 1])
@pytest.mark.parametrize("kind", ["recovery", "odd"])
def test_batch_equals_single_runs_five_forced_steps(kind, type_code):
    X, Y = _problem(kind)
    ths, _, _ = _starts(kind)
    with _ctx() as c:
        c.set_data(X, Y)
        singles = _singles(c, ths, 5, -np.inf, type_code)
        batch = c.po2_em_run_batch([_theta(t) for t in ths], 5, -np.inf, type_code)
        _assert_batch_equals_singles(batch, singles)
        assert all(len(ll) == 6 for ll in batch[1])
        one = c.po2_em_run_batch([_theta(ths[0])], 5, -np.inf, type_code)          # m = 1
        _assert_batch_equals_singles(one, singles[:1])


def test_batch_equals_single_runs_with_a_staggered_stop():
    """A finite atol between two well separated increments (as test_em_run_stop_rule_step_count: the geometric
    mean of the 10th and 11th increment of model 1, whose increments fall by 0.5 a step there) and a max_steps the
    slowest models do not reach: the single runs stop at two or more different passes and at least one runs to
    max_steps, so models freeze one after another inside the batch -- which must not show."""
    X, Y = _problem("recovery")
    ths, S, N = _starts("recovery")
    p, q = X.shape[1], Y.shape[1]
    hist = [np.asarray(B.em_loop(t, S, N, p, q, 60, -np.inf, np.float64)[1], dtype=np.float64) for t in ths]
    inc = np.diff(hist[1])
    assert inc[10] / inc[9] < 0.8
    atol = float(np.sqrt(inc[9] * inc[10]))
    stops = []
    for h in hist:                                   # entries of the history each model would return on the host
        d = np.diff(h)
        hit = np.flatnonzero(d < atol)
        stops.append(int(hit[0]) + 2 if hit.size else 61)
    distinct = sorted(set(stops))
    assert len(distinct) >= 3, stops
    max_steps = distinct[-1] - 2                     # the slowest model(s) run out of steps
    print(f"atol {atol:.3e}, host stop entries {stops}, max_steps {max_steps}")
    with _ctx() as c:
        c.set_data(X, Y)
        singles = _singles(c, ths, max_steps, atol, 0)
        n = [len(s[1]) for s in singles]
        print("device entries", n)
        assert len({v for v in n if v < max_steps + 1}) >= 2 and any(v == max_steps + 1 for v in n), n
        batch = c.po2_em_run_batch([_theta(t) for t in ths], max_steps, atol, 0)
        _assert_batch_equals_singles(batch, singles)


# ------------------------------------------------------------------------------- 3. a failing model
def _raw_batch(c, thetas, steps, atol, type_, m=None):
    """The C entry itself on the thetas' own buffers, with sentinel-filled outputs."""
    from ppls_amd._lib import PplsPo2Theta, _ip, dptr
    m = len(thetas) if m is None else m
    n_ = max(len(thetas), 1)
    arr = (PplsPo2Theta * n_)(*[t.struct() for t in thetas])
    ia = lambda v: np.ascontiguousarray(v, dtype=np.int32)   # noqa: E731
    ip = lambda a: a.ctypes.data_as(_ip)                     # noqa: E731
    r, rx, ry = ia([t.r for t in thetas]), ia([t.rx for t in thetas]), ia([t.ry for t in thetas])
    cap = steps + 1
    ll = np.full((n_, cap), SENT)
    n, neg, st = (np.full(n_, -99, dtype=np.int32) for _ in range(3))
    rc = c._L.ppls_po2_em_run_batch(c.h, m, arr, ip(r), ip(rx), ip(ry), steps, atol, type_, dptr(ll), cap, ip(n), ip(neg), ip(st))
    for t, s in zip(thetas, arr):
        t.pull(s)
    return rc, ll, n, neg, st


def test_a_failing_model_stops_only_itself():
    X, Y = _problem("recovery")
    ths, _, _ = _starts("recovery")
    dup = dict(ths[0])
    dup["Wo"] = np.column_stack([ths[0]["Wo"][:, 0], ths[0]["Wo"][:, 0]])      # two equal loading columns
    ths = [ths[1], dup, ths[0], ths[2]]
    from ppls_amd import PplsError
    with _ctx() as c:
        c.set_data(X, Y)
        with pytest.raises(PplsError) as ei:
            c.po2_em_run(_theta(dup), 5, -np.inf)
        assert ei.value.code == E_NUMERIC
        singles = [None if j == 1 else c.po2_em_run(_theta(t), 5, -np.inf, want_eout=False) for j, t in enumerate(ths)]
        mine = [_theta(t) for t in ths]
        rc, ll, n, neg, st = _raw_batch(c, mine, 5, -np.inf, 0)
        assert rc == 0 and list(st) == [0, E_NUMERIC, 0, 0]
        assert "model 1" in c._L.ppls_last_error(c.h).decode()
        assert _same_theta(mine[1], _theta(dup)) and np.all(ll[1] == SENT) and n[1] == 0       # untouched
        for j in (0, 2, 3):
            est, l1, _, neg1 = singles[j]
            assert n[j] == len(l1) == 6 and np.array_equal(ll[j], l1) and _same_theta(mine[j], est) and bool(neg[j]) == neg1


# --------------------------------------------------------------------------------- 4. no side effects
def test_batch_has_no_side_effects_on_the_context():
    import ppls_amd as pa
    from conftest import make_problem
    X, Y, t0 = make_problem(300, 37, 12, 3, seed=5)
    th = pa.Theta(t0["W"], t0["C"], t0["B"], t0["sigE"], t0["sigF"], t0["sigH"], t0["sigT"])
    rng = np.random.default_rng(3)
    pts = [B.make_theta(rng, 37, 12, 3, 2, 1), B.make_theta(rng, 37, 12, 2, 0, 0), B.make_theta(rng, 37, 12, 1, 3, 2)]

    def state(c):
        est, ll = c.em_state()[:2]
        return [est.W.copy(), est.C.copy(), est.B.copy(), est.sigT.copy(), np.array([est.sigE, est.sigF, est.sigH]), np.array(ll)]

    with _ctx() as c:
        c.set_data(X, Y)
        c.set_option("xprod", 1)
        c.xprod_prepare()
        c.em_begin(th)
        c.em_iterate(6)
        want = state(c)
    with _ctx() as c:
        c.set_data(X, Y)
        c.set_option("xprod", 1)
        c.xprod_prepare()
        before, S0 = c.xprod_stats(th), c.xprod_matrix(padded=True)[0]
        c.em_begin(th)
        c.em_iterate(3)
        c.po2_em_run_batch([_theta(t) for t in pts], 4, -np.inf)
        c.em_iterate(3)
        for a, b in zip(state(c), want):
            assert np.array_equal(a, b)
        after, S1 = c.xprod_stats(th), c.xprod_matrix(padded=True)[0]
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        assert np.array_equal(S0, S1)


# ---------------------------------------------------------------------------------------- 5. refusals
def test_batch_refusals_leave_everything_untouched():
    X, Y = _problem("recovery")
    ths, _, _ = _starts("recovery")
    p, q = X.shape[1], Y.shape[1]

    def refused(c, thetas, code, m=None, S0=None):
        keep = [t.copy() for t in thetas]
        rc, ll, n, neg, st = _raw_batch(c, thetas, 3, -np.inf, 0, m)
        assert rc == code, (rc, code)
        assert np.all(ll == SENT) and np.all(n == -99) and np.all(neg == -99) and np.all(st == -99)
        assert all(_same_theta(a, b) for a, b in zip(thetas, keep))
        if S0 is not None:
            assert np.array_equal(c.xprod_matrix(padded=True)[0], S0)

    with _ctx() as c:
        c.p, c.q = p, q
        refused(c, [_theta(ths[0])], E_STATE)                                   # no data
        c.set_data(X, Y)
        c.xprod_prepare()
        S0 = c.xprod_matrix(padded=True)[0]
        refused(c, [_theta(ths[0])], E_ARG, m=0, S0=S0)                         # m = 0
        refused(c, [_theta(ths[5])] * 257, E_ARG, S0=S0)                        # m > 256
        wide = B.make_theta(np.random.default_rng(0), p, q, 2, 12, 1, orthonormal=False)
        refused(c, [_theta(ths[0]), _theta(wide)], E_ARG, S0=S0)                # a shape outside the limits
        refused(c, [_theta(ths[0]), _theta(dict(ths[1], sigE=-0.5))], E_ARG, S0=S0)
        assert "model 1" in c._L.ppls_last_error(c.h).decode()
        rc, *_ = _raw_batch(c, [_theta(ths[0])], 3, -np.inf, 2)                 # no third orth type
        assert rc == E_ARG
    with _ctx() as d:                                                           # an open stream
        d.stream_begin(p, q, False, False)
        d.stream_rows(X[:10], Y[:10])
        refused(d, [_theta(ths[0])], E_STATE)


# ------------------------------------------------------------- 6. / 7. the CV entry and the held-out error
GRID = [(r, rx, ry) for r in (1, 2) for rx in (0, 2) for ry in (0, 1)]


def _fold_stream(c, X, Y, labels, K):
    c.stream_begin(X.shape[1], Y.shape[1], False, False, nr_folds=K)
    c.stream_rows(X, Y, labels)
    c.stream_end()


def test_cv_entry_equals_the_loop_written_out_and_the_rows():
    """ppls_po2_cv_stream against select, po2_start, single po2_em_run, po2_predict_map and heldout_sse_fold called
    one by one: rmsep, cond and steps bit for bit, the context selected on -1 afterwards.  Then every fold's
    rmsep against the long-double residuals of the returned fit's map on the fold's own rows, within sse_bar."""
    from ppls_amd import po2_predict_map
    X, Y = _problem("recovery")
    n, p, q = X.shape[0], X.shape[1], Y.shape[1]
    K, steps, atol, ss = 3, 30, 1e-4, 4
    labels = (np.arange(n) % K).astype(np.int32)
    rng = np.random.default_rng(9)
    V0x, V0y = rng.standard_normal((p, 2)), rng.standard_normal((q, 1))
    with _ctx() as c:
        _fold_stream(c, X, Y, labels, K)
        res = c.po2_cv_stream(GRID, steps, atol, 0, V0x, V0y, ss, want_fits=True)
        assert c.stream_fold_info()["selected"] == -1
        assert np.all(res["status"] == 0) and np.all(np.isfinite(res["rmsep"]))
        worst = 0.0
        for f in range(K):
            rows = np.flatnonzero(labels == f)
            c.stream_select(f)
            for j, (r, rx, ry) in enumerate(GRID):
                th = c.po2_start(r, rx, ry, V0x[:, :rx], V0y[:, :ry], ss)
                est, ll, _, _ = c.po2_em_run(th, steps, atol, want_eout=False)
                L, Bp = po2_predict_map(est, "X")
                sse, mag = c.heldout_sse_fold(L, est.C, Bp, f)
                assert res["rmsep"][f, j] == np.sqrt(sse[r - 1] / (float(rows.size) * q)), (f, j)
                assert res["cond"][f, j] == mag[r - 1] / sse[r - 1] and res["steps"][f, j] == len(ll) - 1
                assert _same_theta(res["fits"][f][j], est)
                # 7. the same map on the fold's rows in long double
                A = CV.composed(_as_bar_theta(est.as_dict()), 0, L, Bp)
                R = Y[rows].astype(LD) - X[rows].astype(LD) @ A.T
                want = float(np.sum(R * R))
                got = res["rmsep"][f, j] ** 2 * rows.size * q
                bar = sse_bar(mag, rows.size, p, q, r, K_SSE)[r - 1] + 4 * float(U) * want   # + the root and the square
                worst = max(worst, abs(got - want) / bar)
                assert abs(got - want) <= bar, (f, j, got, want, bar)
        c.stream_select(-1)
        print(f"held-out sse: worst err / bar {worst:.3g}")
    assert len({int(s) for s in np.ravel(res["steps"])}) > 1


# ------------------------------------------------------------------------- 8. resident against streamed
def test_crossval_resident_equals_streamed_bitwise():
    from ppls_amd import crossval_PO2PLS, fold_labels
    X, Y = _problem("recovery")
    n, K = X.shape[0], 3
    perm = np.random.default_rng(21).permutation(n)
    labels = fold_labels(n, K, folds=perm)
    args = dict(EMsteps=20, atol=1e-4, start_steps=3)
    with _ctx() as src, _ctx() as st:
        src.set_data(X, Y)
        src.xprod_prepare()
        X0, Y0 = src.get_data()
        S0 = src.xprod_matrix(padded=True)[0]
        a = crossval_PO2PLS(None, None, [1, 2], [0, 2], [0, 1], K, folds=perm, rng=np.random.default_rng(5), ctx=src, **args)
        X1, Y1 = src.get_data()
        assert np.array_equal(X0, X1) and np.array_equal(Y0, Y1) and np.array_equal(S0, src.xprod_matrix(padded=True)[0])
        _fold_stream(st, X, Y, labels, K)
        b = crossval_PO2PLS(None, None, [1, 2], [0, 2], [0, 1], K, rng=np.random.default_rng(5), ctx=st, **args)
        assert st.stream_fold_info()["selected"] == -1
    for key in ("errors", "per_fold", "cond", "steps", "failed"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["best"] == b["best"] and a["which_error"] == b["which_error"] and a["class"] == "cvPO2PLS"
    assert a["errors"].shape == (2, 2, 2) and a["per_fold"].shape == (K, 2, 2, 2)
    with pytest.raises(ValueError):                       # a cell outside the limits, before any device work
        crossval_PO2PLS(X, Y, [2], [12], [0], K)


# ---------------------------------------------------------------------------- 9. predict_PO2PLS
@pytest.mark.parametrize("xy", ["X", "Y"])
def test_predict_po2pls_against_the_dense_conditional_mean(xy):
    """Entrywise: cv_bar's bar of ppls_predict for the map's (L, Bp), plus ||row||_2 x the map's normwise bar_A
    (po2_cv_bar) against the dense Sigma_yx Sigma_xx^-1 in long double."""
    from ppls_amd import po2_predict_map, predict_PO2PLS
    xory = int(xy == "Y")
    th = B.make_theta(np.random.default_rng(77), 37, 21, 3, 2, 1, orthonormal=False, scale=2.0)
    new = np.random.default_rng(78).standard_normal((57, 21 if xory else 37))
    with _ctx() as c:
        c.set_data(np.zeros((0, 37)), np.zeros((0, 21)))
        got = predict_PO2PLS(th, new, xy, ctx=c)
    L, Bp = po2_predict_map(th, xy)
    fitW, fitC = (th["W"], L) if xory else (L, th["C"])
    want = new.astype(LD) @ CV.dense_conditional(th, xory).T
    bar = cv_bar.bars_predict(new, fitW, fitC, Bp, xory) + np.linalg.norm(new, axis=1, keepdims=True) * float(CV.composed_bar(th, xory))
    ratio = float(np.max(np.abs(got.astype(LD) - want) / bar))
    print(f"predict_PO2PLS {xy}: err / bar {ratio:.3g}")
    assert got.shape == want.shape and ratio <= 1.0


def test_predict_po2pls_rescale_on_a_scaled_context():
    """rescale=True on a context whose data were scaled on the device: new rows in loaded units go through the
    stored centre and scale, the map, and back.  The bar adds the roundings of the two affine maps (3 u each way)."""
    from ppls_amd import po2_predict_map, predict_PO2PLS
    X, Y = _problem("odd")
    X, Y = X * 3.0 + 1.5, Y * 0.5 - 2.0
    th = B.make_theta(np.random.default_rng(79), 37, 21, 3, 2, 1)
    new = X[:40]
    with _ctx() as c:
        c.set_data(X, Y)
        c.scale_data(True, True)
        sc = c.scaling()
        got = predict_PO2PLS(th, new, "X", ctx=c, rescale=True)
    L, Bp = po2_predict_map(th, "X")
    z = (new - sc["centerX"]) / sc["scaleX"]
    A = CV.dense_conditional(th, 0)
    zl = (new.astype(LD) - sc["centerX"].astype(LD)) / sc["scaleX"].astype(LD)
    want = (zl @ A.T) * sc["scaleY"].astype(LD) + sc["centerY"].astype(LD)
    inner = cv_bar.bars_predict(z, L, th["C"], Bp, 0) + np.linalg.norm(z, axis=1, keepdims=True) * float(CV.composed_bar(th, 0))
    inner = inner + 3 * float(U) * np.asarray((np.abs(new) + np.abs(sc["centerX"])) / sc["scaleX"] @ np.abs(A).T, dtype=np.float64)
    bar = inner * sc["scaleY"] + 3 * float(U) * (np.abs(np.asarray(want, dtype=np.float64)) + np.abs(sc["centerY"]))
    ratio = float(np.max(np.abs(got.astype(LD) - want) / bar))
    print(f"predict_PO2PLS rescale: err / bar {ratio:.3g}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------ 10. end to end
def test_crossval_po2pls_end_to_end_seed_0():
    """Seed 0 of the recovery problem, folds i % 4: every cell finite, the true sizes (2, 2, 1) at least 5 % better
    than the shared-only (2, 0, 0), and the chosen model has r = 2 and rx >= 1 (the best few cells differ by
    1e-4 to 1e-3 only, so the exact cell is not asserted)."""
    from ppls_amd import crossval_PO2PLS, cv_PO2PLS
    X, Y = _problem("recovery")
    n = X.shape[0]
    folds = np.argsort(np.arange(n) % 4, kind="stable")
    rs, rxs, rys = [1, 2], [0, 1, 2], [0, 1]
    with _ctx() as c:
        res = crossval_PO2PLS(X, Y, rs, rxs, rys, 4, folds=folds, rng=np.random.default_rng(0), ctx=c)
        one = cv_PO2PLS(None, None, 2, 2, 1, 4, folds=folds, rng=np.random.default_rng(0), ctx=c)
    e = res["errors"]
    print("errors\n", e, "\nbest", res["best"], "steps", res["steps"].max(), f"time {res['time']:.2f} s")
    assert np.all(np.isfinite(e)) and not np.any(res["failed"])
    full, shared = e[1, 2, 1], e[1, 0, 0]
    assert full < 0.95 * shared, (full, shared)
    assert res["best"][0] == 2 and res["best"][1] >= 1
    assert one == full                           # one cell alone: the same draws, the same folds, the same bits


# ------------------------------------------------------------------------------------- 11. two ranks
def test_cv_entry_two_ranks_agree_bitwise():
    from test_gpu_stream import ThreadAllReduce
    X, Y = _problem("recovery")
    n, p, q, K = X.shape[0], X.shape[1], Y.shape[1], 3
    labels = (np.arange(n) % K).astype(np.int32)
    rng = np.random.default_rng(9)
    V0x, V0y = rng.standard_normal((p, 2)), rng.standard_normal((q, 1))
    cut = [0, 173, n]
    red = ThreadAllReduce(2)
    out, errs = [None, None], []

    def body(rank):
        try:
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.stream_begin(p, q, False, False, nr_folds=K)
                c.stream_rows(X[cut[rank]:cut[rank + 1]], Y[cut[rank]:cut[rank + 1]], labels[cut[rank]:cut[rank + 1]])
                c.stream_end()
                out[rank] = c.po2_cv_stream(GRID, 20, 1e-4, 0, V0x, V0y, 3)
        except BaseException as ex:   # noqa: BLE001
            errs.append(ex)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
    assert not errs, errs
    for key in ("rmsep", "cond", "steps", "status"):
        assert np.array_equal(out[0][key], out[1][key]), key
    assert np.all(out[0]["status"] == 0)
