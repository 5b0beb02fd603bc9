"""PO2PLS from the cross-products on the GPU (ppls_po2.hip): the statistics pass and the Gram
against entrywise long-double bars, the small kernel against its normwise bars, the E-step and the
log-likelihood against the dense restatement of EMstepC / loglC on four kinds of context, the EM loop
against the long-double loop, the fit end to end, two ranks, and the refusals.

Every bar is a priori (tests/po2_bar.py).  The loop's criterion is the issue's: loadings compared as
projectors, within 16 x the fp64 numpy loop's own distance from the long-double loop, floor 1e-13 x scale.
"""
import threading

import numpy as np
import pytest

import po2_bar as B
from sweep_bar import LD, padded_width

pytestmark = pytest.mark.gpu

E_ARG, E_NUMERIC, E_STATE = -1, -3, -4


def _ctx():
    from ppls_amd import Context
    return Context(0)


def _theta(th):
    from ppls_amd import Po2Theta
    return Po2Theta(th["W"], th["Wo"], th["C"], th["Co"], th["B"], th["sigT"], th["sigTo"], th["sigUo"], th["sigE"],
                    th["sigF"], th["sigH"])


def _as_bar_theta(est):
    """A Po2Theta's as_dict() (diagonal matrices) as po2_bar's dict of vectors."""
    d = dict(est)
    for k in ("B", "sigT", "sigTo", "sigUo"):
        d[k] = np.diag(np.asarray(d[k])) if np.ndim(d[k]) == 2 else np.asarray(d[k])
    return d


def _padded_S(S, p, q):
    ldx, ldy = padded_width(p), padded_width(q)
    Sp = np.zeros((ldx + ldy, ldx + ldy))
    live = np.r_[np.arange(p), ldx + np.arange(q)]
    Sp[np.ix_(live, live)] = S
    return Sp, ldx, ldy, live


def _padded_G(G, ld):
    out = np.zeros((ld, G.shape[1]))
    out[:G.shape[0]] = G
    return out


# --------------------------------------------------------------------------- 1. the pass and the Gram
WIDTHS = [(1, 1), (5, 5), (6, 5), (5, 6), (16, 1), (1, 16), (16, 16)]
PS = [2, 37, 128, 129, 255, 256, 257, 258]


def _pass_case(c, p, q, kx, ky, rows=40, rws=(0, 1, 2, 4, 8)):
    rng = np.random.default_rng(1000 * p + 10 * q + kx + 31 * ky)
    D = rng.standard_normal((rows, p + q))
    S = D.T @ D
    Gx, Gy = rng.standard_normal((p, kx)), rng.standard_normal((q, ky))
    ref = B.PassReference(S, p, q, Gx, Gy)
    Sp, ldx, ldy, live = _padded_S(S, p, q)
    pad = np.setdiff1d(np.arange(ldx + ldy), live)
    worst = 0.0
    for rw in rws:
        if rw == 8 and max(kx, ky) > 8:
            continue
        M, Q, GGx, GGy = c.po2_stats(_padded_G(Gx, ldx), _padded_G(Gy, ldy), Sp, rw=rw)
        r = ref.ratios(M[live], Q, GGx, GGy)
        print(f"p={p} q={q} widths=({kx},{ky}) rw={rw}: err / bar {r}")
        assert max(r.values()) <= 1.0, (rw, r)
        assert np.all(M[pad] == 0.0)                       # padding rows of S give exact zeros
        assert np.array_equal(Q, Q.T) and np.array_equal(GGx, GGx.T) and np.array_equal(GGy, GGy.T)
        again = c.po2_stats(_padded_G(Gx, ldx), _padded_G(Gy, ldy), Sp, rw=rw)
        for a, b in zip((M, Q, GGx, GGy), again):
            assert np.array_equal(a, b)                    # the same bits twice
        worst = max(worst, max(r.values()))
    return worst


@pytest.mark.parametrize("p", PS)
def test_pass_and_gram_shapes(p):
    """Every p at the tile boundaries with q = 3 and transposed, widths (5, 6), every rows-per-wave; the
    last workgroup always runs past the end of P here (P is no multiple of waves x rows-per-wave)."""
    with _ctx() as c:
        _pass_case(c, p, 3, 5, 6)
        if p >= 6:
            _pass_case(c, 7, p, 6, 5)
        else:
            _pass_case(c, 3, p, 2, 2)


@pytest.mark.parametrize("kx,ky", WIDTHS)
def test_pass_and_gram_widths(kx, ky):
    with _ctx() as c:
        _pass_case(c, 129, 37, kx, ky)


def test_pass_past_the_nontemporal_threshold():
    """One S just past the launcher's non-temporal threshold (8 P^2 > 200 MiB), formed from 64 rows."""
    from ppls_amd._lib import lib
    p, q = 5100, 2                      # P = 5120 + 2: the smallest even P past the threshold
    P = padded_width(p) + padded_width(q)
    assert lib().ppls_po2_panel_nt(P) == 1 and lib().ppls_po2_panel_nt(P - 2) == 0
    with _ctx() as c:
        _pass_case(c, p, q, 2, 1, rows=64, rws=(0,))


def test_existing_tile_kernel_unchanged_by_a_po2_call():
    """ppls_xprod_stats (the PPLS_simult tile kernel) gives the same bits before and after PO2 calls on
    the same context, and S itself is left bit for bit."""
    from conftest import make_problem
    from ppls_amd import Theta
    X, Y, t0 = make_problem(300, 37, 12, 3, seed=5)
    th = Theta(t0["W"], t0["C"], t0["B"], t0["sigE"], t0["sigF"], t0["sigH"], t0["sigT"])
    rng = np.random.default_rng(3)
    pt = B.make_theta(rng, 37, 12, 3, 2, 1)
    with _ctx() as c:
        c.set_data(X, Y)
        c.xprod_prepare()
        before, S0 = c.xprod_stats(th), c.xprod_matrix(padded=True)[0]
        c.po2_estep(_theta(pt))
        c.po2_em_run(_theta(pt), 3, -np.inf)
        after, S1 = c.xprod_stats(th), c.xprod_matrix(padded=True)[0]
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        assert np.array_equal(S0, S1)


# --------------------------------------------------------------------------------- 2. the small kernel
SMALL = [  # p, q, r, rx, ry, orthonormal
    (13, 9, 2, 2, 1, True), (13, 9, 2, 2, 1, False), (13, 9, 3, 0, 2, False), (13, 9, 3, 2, 0, False),
    (13, 9, 4, 0, 0, True), (40, 36, 9, 7, 7, False),   # k = 32
]


def _small_inputs(p, q, r, rx, ry, orthonormal, seed=0):
    rng = np.random.default_rng(seed + 7 * p + r)
    th = B.make_theta(rng, p, q, r, rx, ry, orthonormal, scale=1.4)
    N = 60
    D = rng.standard_normal((N, p + q))
    S = D.T @ D
    ref = B.sform(th, S, N, p, q)       # long double: Q, GG and everything after them
    Q64, GGx64, GGy64 = (np.asarray(ref[k], dtype=np.float64) for k in ("Q", "GGx", "GGy"))
    ssqX, ssqY = float(np.trace(S[:p, :p])), float(np.trace(S[p:, p:]))
    # the kernel's inputs are the fp64 roundings: the reference restarts from exactly those
    ref = B.small(th, Q64, GGx64, GGy64, N, p, q, ssqX, ssqY)
    return th, N, ssqX, ssqY, Q64, GGx64, GGy64, ref


@pytest.mark.parametrize("p,q,r,rx,ry,orthonormal", SMALL)
def test_small_kernel_inside_its_bars(p, q, r, rx, ry, orthonormal):
    th, N, ssqX, ssqY, Q, GGx, GGy, ref = _small_inputs(p, q, r, rx, ry, orthonormal)
    bars = B.small_bars(ref, th, N, p, q, ssqX, ssqY)
    with _ctx() as c:
        e, ll, st = c.po2_small(Q, GGx, GGy, _theta(th), p, q, N, ssqX, ssqY)
    assert st == 0
    kx, k = r + rx, 2 * r + rx + ry
    Czz = np.zeros((k, k))
    t, to, u, uo = slice(0, r), slice(r, kx), slice(kx, kx + r), slice(kx + r, k)
    Czz[t, t], Czz[to, to], Czz[t, to], Czz[to, t] = e.Ctt, e.Ctoto, e.Ctto, e.Ctto.T
    Czz[u, u], Czz[uo, uo], Czz[u, uo], Czz[uo, u] = e.Cuu, e.Cuouo, e.Cuuo, e.Cuuo.T
    Czz[u, t], Czz[t, u] = e.Cut, e.Cut.T
    known = np.zeros((k, k), dtype=bool)
    for a, b in ((t, t), (to, to), (t, to), (to, t), (u, u), (uo, uo), (u, uo), (uo, u), (u, t), (t, u)):
        known[a, b] = True
    refZ = np.where(known, np.asarray(ref["Czz"], dtype=LD), LD(0))
    got = dict(K=e.K, Czz=Czz, Chh=e.Chh, Cee=e.Cee, Cff=e.Cff, loglik=ll)
    rr = B.small_ratios(got, dict(ref, Czz=refZ), bars)
    print(f"k={k} orthonormal={orthonormal} rho={float(bars['rho']):.2e}: err / bar {rr}")
    assert max(rr.values()) <= 1.0, rr
    assert np.array_equal(e.Ctt, e.Ctt.T) and np.array_equal(e.Cuu, e.Cuu.T)


def test_small_kernel_refuses_a_lambda_that_is_not_positive_definite():
    """PPLS_E_NUMERIC with the status word set and every output (moment blocks, K, Cee, Cff, loglik) as it was."""
    import ctypes as ct
    from ppls_amd import Po2Expect
    from ppls_amd._lib import dptr
    SENT = -7.25e77
    th, N, ssqX, ssqY, Q, GGx, GGy, _ = _small_inputs(13, 9, 2, 2, 1, True)
    with _ctx() as c:
        for theta, ggx, want in ((th, -50.0 * np.eye(4), -22), (dict(th, sigTo=np.array([1.0, -1.0])), GGx, -21)):
            t = _theta(theta)
            e = Po2Expect(13, 9, 2, 2, 1, want_cdz=False)
            for nm in e.NAMES:
                getattr(e, nm)[...] = SENT
            ts, es = t.struct(), e.struct()
            es.Cee = es.Cff = SENT
            GG = np.concatenate([np.ravel(ggx, order="F"), np.ravel(GGy, order="F")])
            ll, st = ct.c_double(SENT), ct.c_int(0)
            rc = c._L.ppls_po2_small(c.h, dptr(np.asfortranarray(Q)), dptr(GG), ct.byref(ts), 2, 2, 1, 13, 9, float(N), ssqX, ssqY,
                                     ct.byref(es), ct.byref(ll), ct.byref(st))
            assert (rc, st.value, ll.value) == (E_NUMERIC, want, SENT)
            assert all(np.all(getattr(e, nm) == SENT) for nm in e.NAMES) and es.Cee == SENT == es.Cff
        e, ll, st = c.po2_small(Q, -50.0 * np.eye(4), GGy, _theta(th), 13, 9, N, ssqX, ssqY)
        assert (e, ll, st) == (None, None, -22)


# ----------------------------------------------------------- 3. E-step and log-likelihood on contexts
def _estep_check(c, th, tag):
    """ppls_po2_estep / ppls_po2_loglik on context c against the dense long-double restatement on the S
    the context holds, inside the pass's bars propagated through the small algebra's."""
    e = c.po2_estep(_theta(th))          # on resident rows this forms S (and keeps it)
    ll = c.po2_loglik(_theta(th))
    _estep_values_check(e, ll, c.xprod_matrix(), float(c.n_total), c.p, c.q, th, tag)


def _estep_values_check(e, ll, S, N, p, q, th, tag):
    """An E-step's outputs (e, ll) against the dense long-double restatement on S with N rows."""
    dense = B.dense_estep(th, S, N)
    ll_ref = B.dense_loglik(th, S, N)
    ref = B.sform(th, S, N, p, q)
    Gx, Gy = B.loadings(th)
    pr = B.PassReference(S, p, q, Gx, Gy)
    bar_GG = np.sqrt(np.sum(pr.bar_GGx ** 2) + np.sum(pr.bar_GGy ** 2))
    ssqX, ssqY = float(np.trace(S[:p, :p])), float(np.trace(S[p:, p:]))
    bars = B.small_bars(ref, th, N, p, q, ssqX, ssqY, e_Q=np.sqrt(np.sum(pr.bar_Q ** 2)), e_G=bar_GG)
    r, rx, ry, kx, ky, k = B.shape(th)
    worst = {}
    for name in ("Ctt", "Ctoto", "Ctto", "Cuu", "Cuouo", "Cuuo", "Cut"):
        worst[name] = B.ratio(getattr(e, name), dense[name], bars["Czz"])
    worst["Chh"] = B.ratio(e.Chh, dense["Chh"], bars["Chh"])
    worst["Cee"] = B.ratio(np.array([e.Cee]), np.array([dense["Cee"]]), np.array([bars["Cee"]]))
    worst["Cff"] = B.ratio(np.array([e.Cff]), np.array([dense["Cff"]]), np.array([bars["Cff"]]))
    worst["loglik"] = B.ratio(np.array([ll]), np.array([ll_ref]), np.array([bars["loglik"]]))
    # C_dz = M K / N: the bar of a raw update without its second term
    M, K = np.asarray(ref["M"], dtype=LD), np.abs(np.asarray(ref["K"], dtype=LD))
    bar_dz = (pr.bar_M @ K + np.abs(M).sum(axis=1, keepdims=True) * bars["K"] + B.gamma(k + 2) * (np.abs(M) @ K)) / LD(N) * B.SLACK
    got_dz = np.vstack([np.hstack([e.Cxt, e.Cxto, np.zeros((p, ky))]), np.hstack([np.zeros((q, kx)), e.Cyu, e.Cyuo])])
    ref_dz = np.vstack([np.hstack([dense["Cxt"], dense["Cxto"], np.zeros((p, ky), dtype=LD)]),
                        np.hstack([np.zeros((q, kx), dtype=LD), dense["Cyu"], dense["Cyuo"]])])
    worst["Cdz"] = B.ratio(got_dz, ref_dz, bar_dz)
    print(f"{tag}: err / bar {worst}")
    assert max(worst.values()) <= 1.0, (tag, worst)


def test_estep_and_loglik_on_four_kinds_of_context():
    rng = np.random.default_rng(21)
    n, p, q, r, rx, ry = 240, 37, 14, 3, 2, 2
    X = rng.standard_normal((n, p)) @ rng.standard_normal((p, p)) * 0.3 + 1.5
    Y = X[:, :q] * 0.5 + rng.standard_normal((n, q)) + 0.7
    th = B.make_theta(rng, p, q, r, rx, ry, orthonormal=False, scale=1.2)
    with _ctx() as c:
        c.set_data(X, Y)
        _estep_check(c, th, "resident")          # S formed here, by the route o2m_xprod uses, and kept
        assert c.xprod_info()["ready"]
        with _ctx() as d:
            cnt = rng.integers(0, 4, n)
            d.xprod_resample(c, cnt)
            _estep_check(d, th, "resampled")
    with _ctx() as c:
        c.stream_begin(p, q, True, True)
        for lo, hi in ((0, 50), (50, 171), (171, n)):
            c.stream_rows(X[lo:hi], Y[lo:hi])
        c.stream_end()
        _estep_check(c, th, "streamed, centred and scaled")
        with _ctx() as d:
            d.xprod_adjust(c, 2)
            th2 = B.make_theta(rng, p, q - 2, r, rx, ry, orthonormal=False, scale=1.2)
            _estep_check(d, th2, "covariate-adjusted")


# ------------------------------------------------------------------------------------ 4. the EM loop
def _loop_problem(seed=16, n=None):
    X, Y, tr = B.host_problem(seed)
    s = B.HOST_SHAPE
    S = np.hstack([X, Y]).T @ np.hstack([X, Y])
    t0 = B.start_theta(S, s["N"], s["p"], s["q"], s["r"], s["rx"], s["ry"], seed)
    return X, Y, tr, t0, s


def _loading_distances(est, ref):
    return {k: B.projector_distance(est[k], np.asarray(ref[k], dtype=np.float64)) for k in ("W", "Wo", "C", "Co")}


def _loop_check(est, ll, S, N, p, q, t0, steps, type_name):
    """A forced device run of `steps` EM steps against the long-double loop on S: loadings as projectors,
    within 16 x the fp64 numpy loop's own distance (floor 1e-13 x scale); scalars and history alike."""
    thL, llL, momL = B.em_loop(t0, S, N, p, q, steps, -np.inf, LD, type_name)
    th64, ll64, _ = B.em_loop(t0, S, N, p, q, steps, -np.inf, np.float64, type_name)
    assert len(ll) == steps + 1 == len(llL)              # steps + 1 entries
    got = B.canonical(_as_bar_theta(est.as_dict()))
    refc, f64c = B.canonical({k: np.asarray(v, dtype=np.float64) for k, v in thL.items()}), B.canonical(th64)
    own = _loading_distances(f64c, refc)
    dev = _loading_distances(got, refc)
    print(type_name, "projector distances: fp64 numpy loop", own, "device", dev)
    for k in own:                                # scale of a projector: sqrt(columns)
        assert dev[k] <= max(16 * own[k], 1e-13 * np.sqrt(max(got[k].shape[1], 1))), (k, dev[k], own[k])
    for k in ("B", "sigT", "sigTo", "sigUo", "sigE", "sigF", "sigH"):
        a, b, o_ = np.ravel(got[k]), np.ravel(refc[k]).astype(np.float64), np.ravel(f64c[k])
        scale = float(np.max(np.abs(b)))
        assert np.max(np.abs(a - b)) <= max(16 * np.max(np.abs(o_ - b)), 1e-13 * scale), (k, a, b)
    llr = np.asarray(llL, dtype=np.float64)
    own_ll = np.max(np.abs(np.asarray(ll64) - llr))
    assert np.max(np.abs(ll - llr)) <= max(16 * own_ll, 1e-13 * np.max(np.abs(llr)))


@pytest.mark.parametrize("type_name,type_code", [("SVD", 0), ("QR", 1)])
def test_em_run_five_forced_steps_against_the_long_double_loop(type_name, type_code):
    X, Y, _, t0, s = _loop_problem()
    with _ctx() as c:
        c.set_data(X, Y)
        est, ll, eout, neg = c.po2_em_run(_theta(t0), 5, -np.inf, type_=type_code)
        S = c.xprod_matrix()                     # the loops below start from the S the device holds
        again = c.po2_estep(est)                 # the returned Expectations belong to the returned estimates
    _loop_check(est, ll, S, float(s["N"]), s["p"], s["q"], t0, 5, type_name)
    assert not neg
    for name in ("Ctt", "Ctoto", "Cuu", "Cut", "Chh", "K", "Cxt", "Cyuo"):
        assert np.array_equal(getattr(again, name), getattr(eout, name)), name


def test_em_run_stop_rule_step_count():
    X, Y, _, t0, s = _loop_problem()
    with _ctx() as c:
        c.set_data(X, Y)
        c.xprod_prepare()
        S = c.xprod_matrix()
        _, ll64, _ = B.em_loop(t0, S, float(s["N"]), s["p"], s["q"], 60, -np.inf, np.float64)
        inc = np.diff(ll64)
        # an atol between two well separated increments: the count cannot flip on rounding
        i = int(np.argmax(inc[1:] / inc[:-1] < 0.8)) + 1 if np.any(inc[1:] / inc[:-1] < 0.8) else 10
        i = min(max(i, 3), 50)
        atol = float(np.sqrt(inc[i - 1] * inc[i]))
        _, llh, _ = B.em_loop(t0, S, float(s["N"]), s["p"], s["q"], 60, atol, np.float64)
        est, ll, _, _ = c.po2_em_run(_theta(t0), 60, atol)
        print(f"atol {atol:.3e}: host loop {len(llh)} entries, device {len(ll)}")
        assert len(ll) == len(llh) < 61
        assert ll[-1] - ll[-2] < atol and np.all(np.diff(ll)[:-1] >= atol)
        # the same count with the QR type (the stop rule does not depend on the orth type's signs)
        _, llq, _ = B.em_loop(t0, S, float(s["N"]), s["p"], s["q"], 60, atol, np.float64, "QR")
        _, llqd, _, _ = c.po2_em_run(_theta(t0), 60, atol, type_=1)
        assert len(llqd) == len(llq) < 61
        from ppls_amd import PplsError
        with pytest.raises(PplsError) as ei:     # no third type
            c.po2_em_run(_theta(t0), 5, 1e-4, type_=2)
        assert ei.value.code == E_ARG


@pytest.mark.parametrize("type_name,type_code", [("SVD", 0), ("QR", 1)])
def test_one_ecm_step_before_the_canonical_form(type_name, type_code):
    """ppls_po2_em_step returns the update as the device leaves it, so the column signs of orth are seen:
    entrywise against the long-double ECM step, within 16 x the fp64 numpy step's own distance (floor
    1e-13 x scale).  On this problem R's QR rule flips columns of W and Wo relative to the positive-diagonal
    Cholesky-QR factor, so a wrong pivot sign would show."""
    X, Y, _, t0, s = _loop_problem(seed=17)
    p, q, N = s["p"], s["q"], float(s["N"])
    with _ctx() as c:
        c.set_data(X, Y)
        got = c.po2_em_step(_theta(t0), type_=type_code)
        S = c.xprod_matrix()
    ref = B.ecm_update(t0, B.sform(t0, S, N, p, q, LD), p, LD, type_name)
    own = B.ecm_update(t0, B.sform(t0, S, N, p, q, np.float64), p, np.float64, type_name)
    if type_name == "QR":
        flipped = 0
        th64, mom = B.cast(t0, np.float64), B.sform(t0, S, N, p, q, np.float64)
        for side, key in ((0, "W"), (1, "C")):
            raw = B.raw_updates(th64, mom, p, side, 0)
            Qc = raw @ np.linalg.inv(np.linalg.cholesky(raw.T @ raw).T)
            flipped += int(np.sum(np.sum(Qc * own[key], axis=0) < 0))
        assert flipped >= 1
    for k in ("W", "Wo", "C", "Co", "B", "sigT", "sigTo", "sigUo", "sigE", "sigF", "sigH"):
        a, b, o_ = np.asarray(getattr(got, k)), np.asarray(ref[k], dtype=np.float64), np.asarray(own[k], dtype=np.float64)
        bound = max(16 * float(np.max(np.abs(o_ - b))), 1e-13 * float(np.max(np.abs(b))))
        print(type_name, k, float(np.max(np.abs(a - b))), bound)
        assert np.max(np.abs(a - b)) <= bound, (k, a, b)


def test_an_open_em_session_continues_bitwise_across_po2_calls():
    """ppls_po2_start, PO2PLS and the other entries end no ppls_em_begin session and leave the 'o2m_xprod'
    record: six ppls_em_iterate steps with PO2 calls in the middle give the bits of six uninterrupted ones."""
    import ppls_amd as pa
    from conftest import make_problem
    X, Y, t0 = make_problem(300, 37, 12, 3, seed=5)
    th = pa.Theta(t0["W"], t0["C"], t0["B"], t0["sigE"], t0["sigF"], t0["sigH"], t0["sigT"])
    rng = np.random.default_rng(2)

    def state(c):
        est, ll = c.em_state()[:2]
        return [est.W.copy(), est.C.copy(), est.B.copy(), est.sigT.copy(), np.array([est.sigE, est.sigF, est.sigH]), np.array(ll)]

    with _ctx() as c:
        c.set_data(X, Y)
        c.set_option("xprod", 1)
        c.em_begin(th)
        c.em_iterate(6)
        want = state(c)
    with _ctx() as c:
        c.set_data(X, Y)
        c.set_option("xprod", 1)
        pa.PPLS(None, None, 2, 5, 1e-4, "o2m_xprod", ctx=c)
        info = c.o2m_info()
        c.em_begin(th)
        c.em_iterate(3)
        start = c.po2_start(2, 2, 1, rng.standard_normal((37, 2)), rng.standard_normal((12, 1)), 4)
        fit = pa.PO2PLS(None, None, 2, 2, 1, EMsteps=4, rng=rng, ctx=c)
        c.po2_estep(start)
        c.po2_loglik(start)
        c.po2_em_step(start)
        assert fit["class"] == "PO2PLS" and c.o2m_info() == info
        c.em_iterate(3)
        got = state(c)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# -------------------------------------------------------------------------------- 5. PO2PLS end to end
@pytest.mark.parametrize("seed", B.HOST_SEEDS)
def test_po2pls_recovers_what_the_shared_only_model_loses(seed):
    import ppls_amd as pa
    X, Y, tr, _, s = _loop_problem(seed=seed)
    with _ctx() as c:
        c.set_data(X, Y)
        fit = pa.PO2PLS(None, None, s["r"], s["rx"], s["ry"], EMsteps=300, atol=1e-6, rng=np.random.default_rng(5), ctx=c)
        shared = pa.PO2PLS(None, None, s["r"], 0, 0, EMsteps=300, atol=1e-6, rng=np.random.default_rng(5), ctx=c)
        P0 = tr["W"] @ tr["W"].T
        W1, W0 = fit["estimates"]["W"], shared["estimates"]["W"]
        e1, e0 = np.linalg.norm(W1 @ W1.T - P0), np.linalg.norm(W0 @ W0.T - P0)
        print(f"loading-space error: with the specific parts {e1:.3f}, shared only {e0:.3f}; "
              f"b {np.diag(fit['estimates']['B'])} vs {np.diag(shared['estimates']['B'])}; steps {len(fit['loglik']) - 1}")
        assert e1 < 0.5 * e0
        ll = fit["loglik"]
        assert np.all(np.diff(ll) >= -1e-9 * np.abs(ll[-1]))
        assert fit["class"] == "PO2PLS"
        # canonical form on return
        est = fit["estimates"]
        can = pa.canonical_PO2PLS(est)
        for k in ("W", "Wo", "C", "Co", "B", "sigT", "sigTo", "sigUo"):
            assert np.array_equal(np.asarray(can[k]), np.asarray(est[k])), k
        # scores against numpy
        Z = pa.scores_PO2PLS(fit, ctx=c)
        Gx, Gy = np.hstack([est["W"], est["Wo"]]), np.hstack([est["C"], est["Co"]])
        Zr = np.hstack([X @ Gx, Y @ Gy]) @ fit["Expectations"]["K"]
        assert np.max(np.abs(Z - Zr)) <= 1e-12 * np.max(np.abs(Zr))
        sm = pa.summary_PO2PLS(fit)
        assert abs(sm["X"]["joint"] + sm["X"]["specific"] + sm["X"]["noise"] - 1) < 1e-12


def test_po2pls_start_values_and_later_ppls_simult_unchanged():
    import ppls_amd as pa
    X, Y, tr, _, s = _loop_problem(seed=17)
    p, q, r, rx, ry = s["p"], s["q"], s["r"], s["rx"], s["ry"]
    init = dict(W=tr["W"], C=tr["C"], B=np.diag(tr["B"]), sigE=0.6, sigF=0.6, sigH=0.4, sigT=np.diag(tr["sigT"]))
    with _ctx() as c:
        c.set_data(X, Y)
        c.set_option("xprod", 1)
        before = pa.PPLS_simult(None, None, r, EMsteps=6, init=init, ctx=c)
        # ppls_po2_start: the joint part is the one-step 'o2m_xprod' sequential fit ...
        rng = np.random.default_rng(9)
        V0x, V0y = rng.standard_normal((p, rx)), rng.standard_normal((q, ry))
        th = c.po2_start(r, rx, ry, V0x, V0y, 10)
        f0 = pa.PPLS(None, None, r, 1, 1e-4, "o2m_xprod", ctx=c)
        assert np.array_equal(th.W, f0["W"]) and np.array_equal(th.C, f0["C"]) and np.array_equal(th.B, f0["B"])
        assert np.array_equal(th.sigT, f0["sig"][:, 3])
        assert (th.sigE, th.sigF, th.sigH) == tuple(f0["sig"][r - 1, :3])
        # ... and the specific parts the written-out subspace iteration
        S = c.xprod_matrix()

        def written_out(Sb, L, V):
            Qb = np.linalg.qr(L)[0]
            pj = lambda A: A - Qb @ (Qb.T @ A)
            V = np.linalg.qr(pj(V))[0]
            for _ in range(10):
                V = np.linalg.qr(pj(Sb @ V))[0]
            return V, np.sqrt(np.diag(V.T @ Sb @ V) / s["N"])

        Vx, dx = written_out(S[:p, :p], th.W, V0x)
        Vy, dy = written_out(S[p:, p:], th.C, V0y)
        assert B.projector_distance(th.Wo, Vx) <= 1e-10 and B.projector_distance(th.Co, Vy) <= 1e-10
        assert np.allclose(np.sort(th.sigTo), np.sort(dx), rtol=1e-9) and np.allclose(th.sigUo, dy, rtol=1e-9)
        Qw = np.linalg.qr(th.W)[0]
        assert np.max(np.abs(Qw.T @ th.Wo)) <= 1e-12           # orthogonal to the joint loadings
        assert np.max(np.abs(th.Wo.T @ th.Wo - np.eye(rx))) <= 1e-12
        # rx = ry = 0 needs no draws; a refused start leaves theta_out as it was
        th0 = c.po2_start(r, 0, 0)
        assert np.array_equal(th0.W, th.W) and th0.rx == 0 == th0.ry
        with pytest.raises(pa.PplsError) as ei:
            c.po2_start(r, rx, ry, np.zeros((p, rx)), V0y, 10)    # a zero block has no span
        assert ei.value.code == E_NUMERIC
        with pytest.raises(pa.PplsError) as ei:
            c.po2_start(r, 13, ry, np.zeros((p, 13)), V0y, 10)
        assert ei.value.code == E_ARG
        pa.PO2PLS(None, None, r, rx, ry, EMsteps=5, rng=np.random.default_rng(1), ctx=c)
        after = pa.PPLS_simult(None, None, r, EMsteps=6, init=init, ctx=c)
        for k in ("W", "C", "B", "sigT"):
            assert np.array_equal(before["estimates"][k], after["estimates"][k]), k
        assert np.array_equal(before["loglik"], after["loglik"])


def test_scores_refused_without_rows():
    import ppls_amd as pa
    X, Y, tr, t0, s = _loop_problem(seed=17)
    with _ctx() as c:
        c.stream_begin(s["p"], s["q"], False, False)
        c.stream_rows(X, Y)
        c.stream_end()
        fit = pa.PO2PLS(None, None, s["r"], s["rx"], s["ry"], EMsteps=3, init={**t0, "B": np.diag(t0["B"])}, ctx=c)
        with pytest.raises(pa.PplsError) as ei:
            pa.scores_PO2PLS(fit, ctx=c)
        assert ei.value.code == E_STATE


# --------------------------------------------------------------------------------------- 6. two ranks
def test_two_ranks_agree_bitwise():
    from test_gpu_stream import ThreadAllReduce
    X, Y, _, t0, s = _loop_problem(seed=16)
    n = X.shape[0]
    cut = [0, 173, n]
    red = ThreadAllReduce(2)
    out, errs = [None, None], []

    def body(rank):
        try:
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.set_data(X[cut[rank]:cut[rank + 1]], Y[cut[rank]:cut[rank + 1]], n_total=n)
                c.xprod_prepare()                               # the one collective: S is replicated afterwards
                e, le = c.po2_estep(_theta(t0)), c.po2_loglik(_theta(t0))
                est, ll, _, _ = c.po2_em_run(_theta(t0), 4, -np.inf)
                out[rank] = (e, est, ll, c.xprod_matrix(), le)
        except BaseException as ex:   # noqa: BLE001
            errs.append(ex)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    (e0, est0, ll0, S0, le0), (e1, est1, ll1, S1, le1) = out
    assert np.array_equal(S0, S1) and np.array_equal(ll0, ll1) and le0 == le1
    for k in ("W", "Wo", "C", "Co", "B", "sigT", "sigTo", "sigUo"):
        assert np.array_equal(getattr(est0, k), getattr(est1, k)), k
    for k in ("Ctt", "Cuu", "Cut", "Chh", "K", "Cxt", "Cyu"):
        assert np.array_equal(getattr(e0, k), getattr(e1, k)), k
    # the sharded run itself against the references on the S it holds, with N = all ranks' rows: the
    # E-step inside the bars, the loop by the loop test's criterion
    _estep_values_check(e0, le0, S0, float(n), s["p"], s["q"], t0, "rank 0 of 2")
    _loop_check(est0, ll0, S0, float(n), s["p"], s["q"], t0, 4, "SVD")
    # and one rank: inside the same bars, and within two bars of the sharded run
    with _ctx() as c:
        c.set_data(X, Y)
        _estep_check(c, t0, "one rank")
        est_1, ll_1, _, _ = c.po2_em_run(_theta(t0), 4, -np.inf)
        _loop_check(est_1, ll_1, c.xprod_matrix(), float(n), s["p"], s["q"], t0, 4, "SVD")


# ---------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_outputs_theta_and_S_untouched():
    from ppls_amd import PplsError
    X, Y, _, t0, s = _loop_problem(seed=16)
    with _ctx() as c:
        th = _theta(t0)
        with pytest.raises(PplsError) as ei:       # neither S nor rows
            c.p, c.q = s["p"], s["q"]
            c.po2_estep(th)
        assert ei.value.code == E_STATE
        c.set_data(X, Y)
        c.xprod_prepare()
        S0 = c.xprod_matrix(padded=True)[0]

        def refused(theta, code, calls=("estep", "loglik", "em_run")):
            """The C entries themselves, on theta's own buffers and on outputs filled with a sentinel."""
            import ctypes as ct
            from ppls_amd import Po2Expect
            from ppls_amd._lib import dptr
            SENT = -7.25e77
            L, r_, rx_, ry_ = c._L, theta.r, theta.rx, theta.ry
            keep = {k: np.array(getattr(theta, k)) for k in ("W", "Wo", "C", "Co", "B", "sigT", "sigTo", "sigUo")}
            ts = theta.struct()

            def filled():
                e = Po2Expect(c.p, c.q, r_, rx_, ry_)
                for nm in e.NAMES:
                    getattr(e, nm)[...] = SENT
                es = e.struct()
                es.Cee = es.Cff = SENT
                return e, es

            def untouched(e, es):
                return all(np.all(getattr(e, nm) == SENT) for nm in e.NAMES) and es.Cee == SENT == es.Cff

            if "estep" in calls:
                e, es = filled()
                assert L.ppls_po2_estep(c.h, ct.byref(ts), r_, rx_, ry_, ct.byref(es)) == code and untouched(e, es)
            if "loglik" in calls:
                out = ct.c_double(SENT)
                assert L.ppls_po2_loglik(c.h, ct.byref(ts), r_, rx_, ry_, ct.byref(out)) == code and out.value == SENT
            if "em_run" in calls:
                e, es = filled()
                ll, nl, neg = np.full(4, SENT), ct.c_int(-99), ct.c_int(-99)
                rc = L.ppls_po2_em_run(c.h, ct.byref(ts), r_, rx_, ry_, 3, -np.inf, 0, dptr(ll), 4, ct.byref(nl), ct.byref(neg),
                                       ct.byref(es))
                assert rc == code and untouched(e, es) and np.all(ll == SENT) and nl.value == -99 == neg.value
            for k, v in keep.items():
                assert np.array_equal(getattr(theta, k), v, equal_nan=True), k
            assert (ts.sigE, ts.sigF, ts.sigH) == (theta.sigE, theta.sigF, theta.sigH)
            assert np.array_equal(c.xprod_matrix(padded=True)[0], S0)

        refused(_theta(dict(t0, sigE=-0.5)), E_ARG)
        refused(_theta(dict(t0, sigTo=np.array([1.0, np.nan]))), E_ARG)
        refused(_theta(dict(t0, sigUo=np.array([0.0]))), E_ARG)
        bad = dict(t0)
        bad["W"] = t0["W"].copy()
        bad["W"][3, 1] = np.inf
        refused(_theta(bad), E_ARG)
        # sizes: r + rx > min(16, p)
        rng = np.random.default_rng(0)
        wide = B.make_theta(rng, s["p"], s["q"], 2, 12, 1, orthonormal=False)
        refused(_theta(wide), E_ARG)
        # rank-deficient loadings: a repeated specific column makes the update singular
        dup = dict(t0)
        dup["Wo"] = np.column_stack([t0["Wo"][:, 0], t0["Wo"][:, 0]])
        refused(_theta(dup), E_NUMERIC, calls=("em_run",))
        # Lambda not positive definite at the entry level: loadings whose Gram overflows
        huge = dict(t0, W=t0["W"] * 1e160, C=t0["C"] * 1e160)
        refused(_theta(huge), E_NUMERIC)
        # an open stream
        with _ctx() as d:
            d.stream_begin(s["p"], s["q"], False, False)
            d.stream_rows(X[:10], Y[:10])
            with pytest.raises(PplsError) as ei:
                d.po2_estep(_theta(t0))
            assert ei.value.code == E_STATE
