"""Streamed data on the device: ppls_stream_begin / _rows / _rows_from / _end and the streamed state.

S = [X Y]'[X Y] of the centred and scaled data is accumulated from row chunks; the
references and the bars are those of tests/test_stream_host.py:

* near-centred data: entrywise |S - S_ref| <= k gamma_n sqrt(S_jj S_ll), S_ref R's two-pass scale()
  and the Gram in long double, k = K_STAGES = 7 on one context and K_SHARDED = 8 where the cross-rank
  merge runs; two device results of the same rows (other chunks, device chunks, the resident Gram,
  shards) are also held to one bar of each other;
* the ill-conditioned input (means 1e6): max |S / (N - 1) - ref| <= 64 u max_j |mean_j| / sd_j, the
  bar a one-pass S - N m m' misses by five orders of magnitude;
* fits: the bars of tests/test_gpu_xprod.py (log-likelihood 1e-10 relative, loadings 1e-8 absolute,
  scalars and moments 1e-8 relative) against a resident context with the same transform.
"""
import functools
import os
import threading

import numpy as np
import pytest

from conftest import make_problem
from oracle.r_rng import RRNG
from test_stream_host import (K_SHARDED, K_STAGES, gram_bar, ill_bar, ill_conditioned, s_ref, split_rows)

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
STREAMED = "the rows were streamed and are not resident"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L = np.longdouble


def _ctx(dtype=0, xprod=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", xprod)
    return c


def _theta(th):
    from ppls_amd import Theta
    return Theta(th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])


def _relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def _data(n, p, q):
    rng = np.random.default_rng(1000 * n + 10 * p + q)

    def block(m):
        j = np.arange(m)
        return rng.standard_normal((n, m)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7
    X, Y = block(p), block(q)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def _ref(n, p, q, center, scale):
    """(S, centre, scale) in long double for _data(n, p, q), computed once and shared."""
    X, Y = _data(n, p, q)
    S, cen, sd = s_ref(X, Y, center, scale)
    out = tuple(np.asarray(v, dtype=np.float64) for v in (S, cen, sd))
    for v in out:
        v.setflags(write=False)
    return out


def _stream(c, X, Y, bounds, center, scale, order="C"):
    c.stream_begin(X.shape[1], Y.shape[1], center, scale)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        c.stream_rows(np.array(X[lo:hi], order=order), np.array(Y[lo:hi], order=order))
    return c.stream_end()


def _check_S(tag, S, ref, n, k=K_STAGES):
    bar = gram_bar(ref, n, k)
    err = np.abs(S - ref)
    print(f"{tag}: max |S - ref| {err.max():.3g}, max err / bar {np.max(err / bar):.3g}")
    assert S.shape == ref.shape
    assert np.all(err <= bar)


# ------------------------------------------------------------------------------ 1. S, no transform
SHAPES = [(300, 12, 9), (257, 33, 7), (400, 130, 7), (350, 5, 140)]


@pytest.mark.parametrize("order", ["C", "F"], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("n,p,q", SHAPES)
def test_s_parity_no_transform(n, p, q, order):
    X, Y = _data(n, p, q)
    ref, _, _ = _ref(n, p, q, False, False)
    with _ctx() as c, _ctx() as res:
        out = _stream(c, X, Y, split_rows(n), False, False, order)
        assert out["n"] == n and c.n_local == 0 and c.n_total == n
        assert c.stream_info() == dict(state="streamed", rows_local=n, n_total=n, chunks=len(split_rows(n)) - 1)
        S = c.xprod_matrix()
        Sp, ldx = c.xprod_matrix(padded=True)
        ssq = c.ssq()
        res.set_data(X, Y)
        G, _ = res.gram(2)
    _check_S(f"({n},{p},{q}) {order}", S, ref, n)
    assert np.all(np.abs(S - G) <= gram_bar(ref, n))              # the resident Gram: another summation order
    assert np.array_equal(Sp, Sp.T)                                # exactly symmetric
    live = np.zeros(Sp.shape[0], dtype=bool)
    live[:p] = True
    live[ldx:ldx + q] = True
    assert not Sp[~live].any() and not Sp[:, ~live].any()          # the padding is exactly zero
    assert np.array_equal(Sp[np.ix_(live, live)], S)
    assert _relerr(ssq, (np.trace(S[:p, :p]), np.trace(S[p:, p:]))) < 1e-14   # ||X||^2, ||Y||^2 from S


# ------------------------------------------------------------------------------ 2. center / scale
@pytest.mark.parametrize("center,scale", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "center", "scale", "center_scale"])
def test_center_scale_combinations(center, scale):
    n, p, q = 300, 12, 9
    X, Y = _data(n, p, q)
    ref, cen, sd = _ref(n, p, q, center, scale)
    with _ctx() as c, _ctx() as res:
        out = _stream(c, X, Y, split_rows(n), center, scale)
        S = c.xprod_matrix()
        ssq = c.ssq()
        res.set_data(X, Y)
        res.scale_data(center, scale)
        want = res.scaling()
        want_ssq = res.ssq()
    _check_S(f"center={center} scale={scale}", S, ref, n)
    got_c = np.r_[out["centerX"], out["centerY"]]
    got_s = np.r_[out["scaleX"], out["scaleY"]]
    assert np.abs(got_c - cen).max() <= 1e-12 * max(np.abs(cen).max(), 1.0)
    assert _relerr(got_s, sd) < 1e-12
    for k in ("centerX", "centerY"):
        assert np.abs(out[k] - want[k]).max() <= 1e-12 * max(np.abs(want[k]).max(), 1.0)
    for k in ("scaleX", "scaleY"):
        assert np.max(np.abs(out[k] / want[k] - 1)) < 1e-12
    assert _relerr(ssq, want_ssq) < 1e-12
    if scale:                                                      # every column has sum of squares N - 1
        assert np.abs(np.diag(S) - (n - 1)).max() < 1e-11 * n


# ------------------------------------------------------------------------------ 3. |mean| >> sd
def test_ill_conditioned():
    """Means 1e6 at sd 1: max |S / (N - 1) - ref| against the long-double two-pass reference, at the
    bar 64 u max |mean| / sd (~7e-9).  A one-pass S - N m m' is off by ~1e-3 here
    (tests/test_stream_host.py)."""
    X, Y = ill_conditioned()
    n = X.shape[0]
    ref, cen, sd = s_ref(X, Y, True, True)
    ref = np.asarray(ref / L(n - 1), dtype=np.float64)
    bar = ill_bar(X, Y)
    with _ctx() as c:
        out = _stream(c, X, Y, split_rows(n), True, True)
        S = c.xprod_matrix()
    err = np.abs(S / (n - 1) - ref).max()
    print(f"ill-conditioned: max err {err:.3g}, bar {bar:.3g}")
    assert err <= bar
    assert _relerr(np.r_[out["centerX"], out["centerY"]], np.asarray(cen, dtype=np.float64)) < 1e-12
    assert np.max(np.abs(np.r_[out["scaleX"], out["scaleY"]] / np.asarray(sd, dtype=np.float64) - 1)) <= bar


# ------------------------------------------------------------------------------ 4. chunking
def test_chunking_invariance_and_repeatability():
    n, p, q = 300, 12, 9
    X, Y = _data(n, p, q)
    ref, _, _ = _ref(n, p, q, True, True)
    bar = gram_bar(ref, n)
    plans = dict(one=[0, n], ones=[0, 1, 2, 3, 4, 5, n], sixtyfour=list(range(0, n, 64)) + [n])
    S = {}
    with _ctx() as c:
        for name, bounds in plans.items():
            _stream(c, X, Y, bounds, True, True)
            S[name] = c.xprod_matrix(padded=True)[0]
        _stream(c, X, Y, plans["sixtyfour"], True, True)
        again = c.xprod_matrix(padded=True)[0]
        with _ctx() as d:                                          # ... and in another context
            _stream(d, X, Y, plans["sixtyfour"], True, True)
            other = d.xprod_matrix(padded=True)[0]
    assert np.array_equal(again, S["sixtyfour"]) and np.array_equal(other, S["sixtyfour"])
    live = np.abs(S["one"]).sum(axis=0) > 0
    for a in plans:
        for b in plans:
            diff = np.abs(S[a] - S[b])[np.ix_(live, live)]
            print(f"{a} vs {b}: max diff / bar {np.max(diff / bar):.3g}")
            assert np.all(diff <= bar)
    for name in plans:                                             # ... and each against the long-double reference
        _check_S(f"plan {name}", S[name][np.ix_(live, live)], ref, n)


# ------------------------------------------------------------------------------ 5. device chunks
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_stream_rows_from(dtype):
    from ppls_amd import PplsError
    n, p, q, r = 300, 33, 7, 2
    _, _, th = make_problem(8, p, q, r, seed=4)
    bounds = [0, 1, 130, 130, 300]                                 # a one-row chunk and an empty source
    host = []
    with _ctx() as c, _ctx(dtype) as src:
        c.stream_begin(p, q, True, True)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            src.generate_synthetic(n, p, q, _theta(th), 11, row0=lo, n_local=hi - lo)
            before = src.get_data()
            c.stream_rows_from(src)
            after = src.get_data()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            host.append(before)
        out = c.stream_end()
        S = c.xprod_matrix()
        info = c.stream_info()
        c.stream_begin(p, q, True, True)                           # the same rows from the host
        for Xc, Yc in host:
            c.stream_rows(Xc, Yc)
        out_h = c.stream_end()
        Sh = c.xprod_matrix()
        src.generate_synthetic(10, p + 1, q, _theta(make_problem(8, p + 1, q, r)[2]), 1)
        c.stream_begin(p, q)
        with pytest.raises(PplsError) as e:                        # another shape is refused
            c.stream_rows_from(src)
        assert e.value.code == E_ARG
        with pytest.raises(PplsError) as e:                        # ... and the context itself
            c.stream_rows_from(c)
        assert e.value.code == E_ARG
    assert out["n"] == n and info["chunks"] == 3
    X = np.vstack([h[0] for h in host])
    Y = np.vstack([h[1] for h in host])
    ref, _, _ = s_ref(X, Y, True, True)
    ref = np.asarray(ref, dtype=np.float64)
    _check_S(f"rows_from dtype={dtype}", S, ref, n)
    print("device chunks == host chunks bitwise:", np.array_equal(S, Sh))
    assert np.all(np.abs(S - Sh) <= gram_bar(ref, n))
    for k in ("centerX", "scaleX", "centerY", "scaleY"):
        assert _relerr(out[k], out_h[k]) < 1e-12


# ------------------------------------------------------------------------------ 6. fits
def _fit_pair():
    """A streamed context and a resident one that carries the same transform, xprod = 1."""
    n, p, q = 300, 12, 9
    X, Y, _ = make_problem(n, p, q, 3, seed=21)
    X = X + 0.5
    Y = Y * 2.0 - 1.0
    c, res = _ctx(), _ctx(0, 1)
    _stream(c, X, Y, split_rows(n), True, True)
    res.set_data(X, Y)
    res.scale_data(True, True)
    return c, res, (n, p, q)


def _assert_fit(est, ll, eout, ref_est, ref_ll, ref_eout):
    assert len(ll) == len(ref_ll)
    assert _relerr(ll, ref_ll) < 1e-10
    assert np.abs(est.W - ref_est.W).max() < 1e-8
    assert np.abs(est.C - ref_est.C).max() < 1e-8
    assert _relerr(est.B, ref_est.B) < 1e-8
    assert _relerr(est.sigT, ref_est.sigT) < 1e-8
    assert _relerr([est.sigE, est.sigF, est.sigH], [ref_est.sigE, ref_est.sigF, ref_est.sigH]) < 1e-8
    if eout is not None:
        assert eout.mu_T is None and eout.mu_U is None
        for k in ("Ctt", "Cuu", "Cut", "Chh"):
            assert np.abs(getattr(ref_eout, k)).max() > 0           # the moments are filled
            assert _relerr(getattr(eout, k), getattr(ref_eout, k)) < 1e-8
        assert abs(eout.Cee - ref_eout.Cee) / ref_eout.Cee < 1e-8 and eout.Cee > 0
        assert abs(eout.Cff - ref_eout.Cff) / ref_eout.Cff < 1e-8 and eout.Cff > 0


@pytest.mark.parametrize("r", [1, 3, 8])
def test_em_run_on_streamed_context(r):
    c, res, (n, p, q) = _fit_pair()
    with c, res:
        th0 = make_problem(n, p, q, r, seed=5 + r)[2]
        ref = res.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)
        got = c.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)
        _assert_fit(got[0], got[1], got[2], ref[0], ref[1], ref[2])
        # estep / loglik / em_step read S too
        e, e_ref = c.estep(_theta(th0), want_mu=False), res.estep(_theta(th0), want_mu=False)
        assert _relerr(e.Chh, e_ref.Chh) < 1e-8 and abs(e.Cee / e_ref.Cee - 1) < 1e-8
        assert abs(c.loglik(_theta(th0)) / res.loglik(_theta(th0)) - 1) < 1e-10
        t1, _ = c.em_step(_theta(th0))
        t1r, _ = res.em_step(_theta(th0))
        assert np.abs(t1.W - t1r.W).max() < 1e-8 and _relerr(t1.B, t1r.B) < 1e-8


def test_em_session_on_streamed_context():
    c, res, (n, p, q) = _fit_pair()
    with c, res:
        th0 = make_problem(n, p, q, 3, seed=8)[2]
        outs = []
        for k in (c, res):
            k.em_begin(_theta(th0))
            k.em_iterate(10)
            k.em_iterate(15)
            outs.append(k.em_state())
        (est, ll), (ref_est, ref_ll) = outs
        assert len(ll) == 24
        _assert_fit(est, ll, None, ref_est, ref_ll, None)


def test_ppls_and_ppls_simult_on_streamed_context():
    from ppls_amd import PPLS, PPLS_simult, PPLSi
    c, res, (n, p, q) = _fit_pair()
    with c, res:
        fit = PPLS(None, None, 3, 200, 1e-4, "equal", ctx=c)
        ref = PPLS(None, None, 3, 200, 1e-4, "equal", ctx=res)
        assert np.array_equal(fit["Other_output"]["Number_steps"], ref["Other_output"]["Number_steps"])
        assert np.abs(fit["W"] - ref["W"]).max() < 1e-8 and np.abs(fit["C"] - ref["C"]).max() < 1e-8
        assert _relerr(fit["B"], ref["B"]) < 1e-8 and _relerr(fit["sig"], ref["sig"]) < 1e-8
        assert _relerr(fit["Other_output"]["Loglikelihoods"], ref["Other_output"]["Loglikelihoods"]) < 1e-10
        one = PPLSi(None, None, 200, 1e-4, "equal", ctx=c)
        assert np.abs(one["W"] - ref["W"][:, 0]).max() < 1e-8
        init = dict(W=ref["W"], C=ref["C"], B=np.diag(ref["B"]), sigE=ref["sig"][2, 0], sigF=ref["sig"][2, 1],
                    sigH=ref["sig"][2, 2], sigT=np.diag(ref["sig"][:, 3]))
        sim = PPLS_simult(None, None, 3, 15, -np.inf, init=init, ctx=c)
        sim_ref = PPLS_simult(None, None, 3, 15, -np.inf, init=init, ctx=res)
        E, Er = sim["Expectations"], sim_ref["Expectations"]
        assert E["mu_T"] is None and E["mu_U"] is None and Er["mu_T"].shape == (n, 3)
        for k in ("Ctt", "Cuu", "Cut", "Cee", "Cff", "Chh"):
            assert _relerr(E[k], Er[k]) < 1e-8
        assert _relerr(sim["loglik"], sim_ref["loglik"]) < 1e-10
        assert np.abs(sim["estimates"]["W"] - sim_ref["estimates"]["W"]).max() < 1e-8
        sim2 = PPLS_simult(None, None, 2, 5, 1e-4, ctx=c, seed=3)   # the default initialiser runs from S too
        assert sim2["estimates"]["W"].shape == (p, 2) and np.all(np.isfinite(sim2["loglik"]))
        with pytest.raises(NotImplementedError, match="streamed"):
            PPLS(None, None, 2, 20, 1e-4, "o2m", ctx=c)


# ------------------------------------------------------------------------------ 7. the reference's example
def test_reference_example_streamed_raw():
    """PPLS-Ex.R:39-43 with scale() done by the stream: the raw rnorm draws go in 37-row chunks with
    center = scale = 1, and PPLS(., ., 3, 1e4, 1e-4, 'equal') prints the reference's table."""
    from ppls_amd import PPLS, print_PPLS, stream_data
    G = np.load(os.path.join(GOLD, "rcheck_ppls_ex.npz"))
    rng = RRNG(1)
    X = rng.matrix_rnorm(100, 10)
    Y = rng.matrix_rnorm(100, 12)
    with _ctx() as ctx:
        out = stream_data(((X[i:i + 37], Y[i:i + 37]) for i in range(0, 100, 37)), ctx=ctx)
        assert out["n"] == 100 and ctx.stream_info()["chunks"] == 3
        fit = PPLS(None, None, 3, 10000, 1e-4, "equal", ctx=ctx)
    rows, _ = print_PPLS(fit)
    got, want = np.asarray(rows), np.asarray(G["table_equal"])
    assert list(want[:, 5]) == [729, 811, 87]
    assert got.shape == want.shape                                 # test_gpu_scale.py's table check
    assert np.array_equal(got[:, 5], want[:, 5]), f"#steps {got[:, 5]} != printed {want[:, 5]}"
    assert np.abs(got[:, :5] - want[:, :5]).max() < 1e-9, f"\n{got}\n!=\n{want}"
    assert np.abs(got[:, 6]).max() < 5e-4


# ------------------------------------------------------------------------------ 8. predict(rescale=True)
@pytest.mark.parametrize("xy", ["X", "Y"])
def test_predict_rescale_on_streamed_context(xy):
    from ppls_amd import PPLS, predict_PPLS
    n, p, q = 80, 11, 6
    X, Y = (np.array(a) for a in _data(n, p, q))
    Y += X[:, :q] * 0.8
    rng = np.random.default_rng(9)
    with _ctx() as ctx:
        sc = _stream(ctx, X, Y, [0, 30, 80], True, True)
        fit = PPLS(None, None, 2, 30, 1e-4, "equal", ctx=ctx)
        W, C, B = fit["W"], fit["C"], np.asarray(fit["B"])
        cX, sX, cY, sY = sc["centerX"], sc["scaleX"], sc["centerY"], sc["scaleY"]
        assert np.abs(cX).max() > 0 and np.abs(sX - 1).max() > 0
        if xy == "X":
            new = rng.standard_normal((7, p)) * 3 + 1
            want = ((new - cX) / sX) @ W @ np.diag(B) @ C.T * sY + cY
        else:
            new = rng.standard_normal((7, q)) * 3 + 1
            want = ((new - cY) / sY) @ C @ np.diag(1 / B) @ W.T * sX + cX
        got = predict_PPLS(fit, new, xy, ctx=ctx, rescale=True)
    assert got.shape == want.shape
    assert _relerr(got, want) < 1e-12


# ------------------------------------------------------------------------------ 9. state and refusals
def test_streamed_state_refusals():
    from ppls_amd import PplsError, cv_PPLS, crossval_PPLS, scores_PPLS, variances_PPLS_simult
    n, p, q, r = 120, 12, 9, 2
    X, Y, th0 = make_problem(n, p, q, r, seed=2)
    th = _theta(th0)
    one = dict(W=th0["W"][:, :1], C=th0["C"][:, :1], B=1.0, sigE=1.0, sigF=1.0, sigH=0.5, sigT=1.0)
    with _ctx() as c, _ctx() as other:
        other.set_data(X[:50], Y[:50])
        _stream(c, X, Y, [0, 50, n], True, True)
        est, ll, eout, _ = c.em_run(th, 5, -np.inf, 0, want_mu=False)
        fit = dict(estimates=est.as_dict(), Expectations=dict(mu_T=np.zeros((0, r)), mu_U=np.zeros((0, r)),
                                                              Ctt=np.eye(r), Cuu=np.eye(r)))
        e_in = c.estep(th, want_mu=False)
        e_in.mu_T = np.zeros((0, r), order="F")
        e_in.mu_U = np.zeros((0, r), order="F")
        calls = dict(
            estep_mu=lambda: c.estep(th, want_mu=True),
            em_run_mu=lambda: c.em_run(th, 3, -np.inf, 0, want_mu=True),
            em_step_mu=lambda: c.em_step(th, want_fit=True),
            mstep=lambda: c.mstep(e_in),
            scores=lambda: c.scores(th0["W"], th0["C"]),
            sweep_stats=lambda: c.sweep_stats(th),
            scores_PPLS=lambda: scores_PPLS(fit, None, None, ctx=c),
            get_data=lambda: c.get_data(0, 0),
            get_data_rows=lambda: c.get_data_rows(0, 0),
            variances=lambda: c.variances(np.zeros((0, r)), np.ones(r), 0.5, 0),
            variances_PPLS_simult=lambda: variances_PPLS_simult(fit, None, "X", ctx=c),
            heldout_sse=lambda: c.heldout_sse(th0["W"], th0["C"], np.diag(th0["B"]), []),
            cv_ppls=lambda: c.cv_ppls(1, [], [60, 60], 5, 1e-4, [[one], [one]]),
            cv_PPLS=lambda: cv_PPLS(None, None, 1, 2, ctx=c, rng=np.random.default_rng(0)),
            crossval_PPLS=lambda: crossval_PPLS(None, None, [1], 2, ctx=c),
            set_data_from=lambda: other.set_data_from(c, []),
            xprod_downdate=lambda: other.xprod_downdate(c, [0]),
            scale_data=lambda: c.scale_data(),
            meta_emstep=lambda: c.meta_emstep(th0["W"][:, 0], th0["C"][:, 0], [60, 60], np.ones((2, 5))),
            meta_ppls=lambda: c.meta_ppls([60, 60], 3, 1e-4, one),
            comm_init=lambda: c.comm_init(1, 0, b"\0" * 128),
            set_reducer=lambda: c.set_reducer(lambda buf: None),
            dtype=lambda: c.set_option("dtype", 1),
            gram=lambda: c.gram(2),
        )
        for name, call in calls.items():
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE and STREAMED in str(e.value), f"{name}: {e.value}"
        # none of the refusals disturbed the state: the same run again, bit for bit
        est2, ll2, _, _ = c.em_run(th, 5, -np.inf, 0, want_mu=False)
        assert np.array_equal(ll, ll2) and np.array_equal(est.W, est2.W)
        # xprod = 0 neither frees S nor changes the path
        c.set_option("xprod", 0)
        est3, ll3, _, _ = c.em_run(th, 5, -np.inf, 0, want_mu=False)
        assert np.array_equal(ll, ll3) and np.array_equal(est.W, est3.W) and np.array_equal(est.C, est3.C)
        assert c.streamed and c.xprod_info(r)["ready"]
        # xprod_release ends the state: no data
        c.xprod_release()
        assert c.stream_info()["state"] == "none"
        with pytest.raises(PplsError) as e:
            c.em_run(th, 5, -np.inf, 0, want_mu=False)
        assert e.value.code == E_STATE


def test_open_stream_refuses_fits_and_bad_calls():
    from ppls_amd import PplsError
    n, p, q, r = 60, 12, 9, 2
    X, Y, th0 = make_problem(n, p, q, r, seed=2)
    with _ctx() as c:
        for call in (lambda: c.stream_rows(X, Y), lambda: c.stream_end()):      # no stream open
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE
        c.set_data(X, Y)
        c.stream_begin(p, q, True, True)                            # drops the resident data
        c.stream_rows(X[:20], Y[:20])
        assert c.stream_info() == dict(state="open", rows_local=20, n_total=20, chunks=1)
        for call in (lambda: c.em_run(_theta(th0), 3, -np.inf, 0, want_mu=False), lambda: c.ssq(),
                     lambda: c.em_begin(_theta(th0)), lambda: c.get_data(0, 1), lambda: c.scale_data(),
                     lambda: c.xprod_prepare(), lambda: c.set_option("dtype", 1),
                     lambda: c.set_reducer(lambda buf: None), lambda: c.comm_init(1, 0, b"\0" * 128)):
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE
        c.stream_rows(np.zeros((0, p)), np.zeros((0, q)))           # nrows = 0: a no-op
        with pytest.raises(ValueError):
            c.stream_rows(X[:5, :3], Y[:5])
        c.stream_rows(X[20:], Y[20:])
        assert c.stream_end()["n"] == n


def test_refused_streams_leave_no_data():
    from ppls_amd import PplsError
    n, p, q = 60, 12, 9
    X, Y = (np.array(a) for a in _data(n, p, q))
    with _ctx() as c:
        Yc = Y.copy()
        Yc[:, 2] = 2.0                                              # a constant column under scale = 1
        with pytest.raises(PplsError) as e:
            _stream(c, X, Yc, [0, 25, n], True, True)
        assert e.value.code == E_ARG and "Y column 3 " in str(e.value)
        assert c.stream_info()["state"] == "none"
        with pytest.raises(PplsError) as e:
            c.ssq()
        assert e.value.code == E_STATE
        assert _stream(c, X, Yc, [0, 25, n], True, False)["n"] == n    # fine without scaling
        Xn = X.copy()
        Xn[40, 3] = np.nan                                          # a NaN in the second chunk
        for center, scale in ((False, False), (True, True)):
            with pytest.raises(PplsError) as e:
                _stream(c, Xn, Y, [0, 25, n], center, scale)
            assert e.value.code == E_ARG
            assert c.stream_info()["state"] == "none"
        with pytest.raises(PplsError) as e:                         # N = 1 with scale = 1
            _stream(c, X, Y, [0, 1], True, True)
        assert e.value.code == E_ARG and "at least 2 rows" in str(e.value)
        with pytest.raises(PplsError) as e:                         # no rows at all
            _stream(c, X, Y, [0, 0], False, False)
        assert e.value.code == E_ARG


def test_set_data_after_streaming_restores_ordinary_behaviour():
    import json
    name = sorted(f for f in os.listdir(GOLD) if f.endswith(".npz") and not f.startswith(("seq_", "meta_", "rcheck_")))[0]
    g = np.load(os.path.join(GOLD, name))
    meta = json.loads(str(g["meta"]))
    X, Y = np.asarray(g["X"]), np.asarray(g["Y"])
    with _ctx() as c:
        _stream(c, X, Y, [0, X.shape[0] // 2, X.shape[0]], True, True)
        c.set_data(X, Y)
        assert c.stream_info()["state"] == "none" and c.n_local == X.shape[0]
        sc = c.scaling()
        assert not sc["centerX"].any() and np.all(sc["scaleY"] == 1.0)
        th0 = dict(W=g["W0"], C=g["C0"], B=np.diag(g["B0"]), sigE=g["sig0"][0], sigF=g["sig0"][1],
                   sigH=g["sig0"][2], sigT=np.diag(g["T0"]))
        est, ll, eout, _ = c.em_run(_theta(th0), meta["EMsteps"], meta["atol"], 0 if meta["type"] == "SVD" else 1)
        assert len(ll) == meta["steps_done"]
        assert _relerr(ll, g["loglik"]) < 1e-10
        assert np.abs(est.W - g["W"]).max() < 1e-8 and np.abs(est.C - g["C"]).max() < 1e-8
        assert _relerr(eout.mu_T, g["mu_T"]) < 1e-8
        gX, _ = c.get_data()
        assert np.array_equal(gX, X)


# ------------------------------------------------------------------------------ 10. shards
class ThreadAllReduce:
    """Sum over k host threads in rank order (tests/test_gpu_scale.py's): every rank gets the
    bitwise-same result; a bounded barrier, so a missed collective fails instead of hanging."""

    def __init__(self, k):
        self.bar = threading.Barrier(k, timeout=60)
        self.bufs = [None] * k

    def fn(self, rank):
        def reduce(buf):
            self.bufs[rank] = buf.copy()
            self.bar.wait()
            tot = self.bufs[0].copy()
            for b in self.bufs[1:]:
                tot += b
            self.bar.wait()
            buf[:] = tot
        return reduce


def _run_ranks(X, Y, chunks, work):
    """Three contexts on GPU 0 with the host reducer; rank i streams the row ranges chunks[i]."""
    red = ThreadAllReduce(3)
    out, errs = [None] * 3, []

    def body(rank):
        try:
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.stream_begin(X.shape[1], Y.shape[1], True, True)
                for lo, hi in chunks[rank]:
                    c.stream_rows(X[lo:hi], Y[lo:hi])
                out[rank] = work(c, rank)
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
    if errs:
        raise errs[0]
    return out


SHARD_CHUNKS = [[(0, 1), (1, 70)], [(70, 134), (134, 135), (135, 300)], []]     # 2, 3 and 0 chunks


def test_sharded_stream_equals_one_context():
    n, p, q, r = 300, 12, 9, 3
    X, Y = _data(n, p, q)
    ref, _, _ = _ref(n, p, q, True, True)
    th0 = make_problem(n, p, q, r, seed=6)[2]

    def work(c, rank):
        out = c.stream_end()
        return out, c.xprod_matrix(), c.ssq(), c.stream_info(), c.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)

    outs = _run_ranks(X, Y, SHARD_CHUNKS, work)
    with _ctx() as one:
        flat = [0] + [hi for ch in SHARD_CHUNKS for _, hi in ch]
        want = _stream(one, X, Y, flat, True, True)
        S1 = one.xprod_matrix()
        fit1 = one.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)
    for rank, (out, S, ssq, info, fit) in enumerate(outs):
        assert out["n"] == n and info["n_total"] == n and info["rows_local"] == [70, 230, 0][rank]
        assert np.array_equal(S, outs[0][1]) and ssq == outs[0][2]          # every rank holds the same S
        _check_S(f"rank {rank}", S, ref, n, K_SHARDED)
        assert np.all(np.abs(S - S1) <= gram_bar(ref, n, K_SHARDED))
        for k in ("centerX", "scaleX", "centerY", "scaleY"):
            assert np.array_equal(out[k], outs[0][0][k])
            assert np.abs(out[k] - want[k]).max() <= 1e-12 * max(np.abs(want[k]).max(), 1.0)
        _assert_fit(fit[0], fit[1], fit[2], fit1[0], fit1[1], fit1[2])


def test_sharded_refusal_is_the_same_on_every_rank():
    from ppls_amd import PplsError
    X, Y = (np.array(a) for a in _data(300, 12, 9))
    Y[:, 2] = 2.0

    def work(c, rank):
        try:
            c.stream_end()
        except PplsError as e:
            return e.code, str(e), c.stream_info()["state"]
        return 0, "", ""

    outs = _run_ranks(X, Y, SHARD_CHUNKS, work)
    for code, msg, state in outs:
        assert code == E_ARG and "Y column 3 " in msg and state == "none"
        assert msg == outs[0][1]
