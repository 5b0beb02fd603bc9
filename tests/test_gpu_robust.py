"""The real-weighted MFMA Gram, ppls_robust_weights, ppls_xprod_weighted and robust_PPLS_simult on the device
(DESIGN §24).

References and bars are those of tests/robust_bar.py: the weighted Gram against long double from the weights
as the device holds them (fp64), |G - S_ref| <= K_W gamma(n) sqrt(S_aa S_bb) with K_W = 2; the weights and the
t log-likelihood against long double within the bars derived from tests/rowdiag_bar.py's bar on d2.  Fits are
compared with the loop written out on the CPU oracle (robust_bar.oracle_loop), with the tolerances
tests/test_gpu_stream.py::_assert_fit uses between two evaluations of one fit.
"""
import ctypes as ct
import functools
import math
import threading

import numpy as np
import pytest

import robust_bar as rob
import rowdiag_bar as rb
from resample_bar import K_W, K_W_SHARDED, inside, weighted_bar, weighted_ref
from test_gpu_stream import STREAMED, ThreadAllReduce, _assert_fit, _theta

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
NU = 4.0


def _ctx(dtype=0, xprod=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", xprod)
    return c


# ------------------------------------------------------------------------------ 1. the kernel alone
# tests/test_gpu_resample.py's five: fewer than two ring rounds; steady state, a tail and a partial k-step; an
# off-diagonal tile; X's padding meeting Y inside a quadrant
KERNEL_SHAPES = [(1, 3, 2), (5, 3, 2), (27, 5, 3), (257, 130, 3), (64, 70, 61)]


def _kernel_rows(n, p, q):
    rng = np.random.default_rng(1000 * n + 10 * p + q)

    def block(m):
        j = np.arange(m)
        return rng.standard_normal((n, m)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7
    return block(p), block(q)


def _pick(D, p, q, xory):
    return D if xory == 2 else D[:, p:] if xory else D[:, :p]


def _check_weighted(tag, G, D, w, n):
    ref = weighted_ref(D, w)
    ok, worst = inside(G, ref, n)
    print(f"{tag}: max err / bar {worst:.3g} (K_W = {K_W})")
    assert ok
    assert np.array_equal(G, G.T)                                   # exactly symmetric
    return ref


@pytest.mark.parametrize("n,p,q", KERNEL_SHAPES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_real_weighted_gram(dtype, n, p, q):
    X, Y = _kernel_rows(n, p, q)
    w = rob.draw_weights(n, p + q, NU, seed=7)                      # fp64 on the host and on the device alike
    cnt = (np.arange(n) * 5 + 2) % 4
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        D = np.hstack(ctx.get_data())                               # the rows as stored (fp32: rounded)
        for xory in (0, 1, 2):
            Dk = _pick(D, p, q, xory)
            for nsplit in (1, 2, 3):
                tag = f"{'fp32' if dtype else 'fp64'} ({n},{p},{q}) xory {xory} nsplit {nsplit}"
                G, _ = ctx.gram(xory, nsplit, weight=w)
                _check_weighted(tag, G, Dk, w, n)
                # all weights 1.0: the unweighted kernel's bits; integer weights: the count kernel's
                assert np.array_equal(ctx.gram(xory, nsplit, weight=np.ones(n))[0], ctx.gram(xory, nsplit)[0])
                assert np.array_equal(ctx.gram(xory, nsplit, weight=cnt.astype(np.float64))[0],
                                      ctx.gram(xory, nsplit, count=cnt.astype(np.int32))[0])


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_real_weighted_gram_with_an_all_zero_split(dtype):
    n, p, q = 27, 5, 3
    X, Y = _kernel_rows(n, p, q)
    w = rob.draw_weights(n, p + q, NU, seed=3)
    w[9:18] = 0.0                                                   # the whole middle split of three
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        D = np.hstack(ctx.get_data())
        for xory in (0, 1, 2):
            _check_weighted(f"zero split, xory {xory}", ctx.gram(xory, 3, weight=w)[0], _pick(D, p, q, xory), w, n)
        _check_weighted("zero split, auto", ctx.gram(2, 0, weight=w)[0], D, w, n)


def test_real_weighted_gram_refuses_bad_weights():
    from ppls_amd import PplsError
    X, Y = _kernel_rows(5, 3, 2)
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        for bad in (-0.5, np.nan, np.inf):
            w = np.ones(5)
            w[2] = bad
            with pytest.raises(PplsError) as e:
                ctx.gram(2, 1, weight=w)
            assert e.value.code == E_ARG
        with pytest.raises(ValueError):
            ctx.gram(2, 1, weight=np.ones(4))
        with pytest.raises(ValueError, match="not both"):
            ctx.gram(2, 1, weight=np.ones(5), count=np.ones(5, dtype=np.int32))
        assert ctx._L.ppls_gram_weighted_real(ctx.h, 2, 1, None, None, None) == E_ARG


def test_real_weighted_occupancy_equals_unweighted():
    with _ctx() as ctx:
        for f32 in (False, True):
            assert ctx.gram_occupancy(f32, weighted="real") == ctx.gram_occupancy(f32) >= 1


# ------------------------------------------------------------------------------ 2. the weight kernel
WEIGHT_SHAPES = [(300, 12, 9, 2), (70, 130, 5, 3)]


def _nus(m):
    return np.array([NU]) if m == 1 else rob.nu_grid(1.0, 1000.0, 16)


@pytest.mark.parametrize("m", [1, 16])
@pytest.mark.parametrize("n,p,q,r", WEIGHT_SHAPES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_robust_weights(dtype, n, p, q, r, m):
    X, Y, th = rb.make_case(n, p, q, r, seed=3)
    nus, keep = _nus(m), (0 if m == 1 else 5)
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        ll, sw = ctx.robust_weights(rb.theta_of(th), nus, keep)
        w, d2 = ctx.robust_get()
        diag = ctx.row_diagnostics(rb.theta_of(th))
        assert np.array_equal(d2, diag["d2"])                       # the bits the diagnostics report
        ref, bar = rob.reference(X, Y, th, nus, keep, bool(dtype)), rob.bars(X, Y, th, nus, keep, bool(dtype))
        ok_w, worst_w = rob.inside(w, ref["w"], bar["w"])
        ok_l, worst_l = rob.inside(ll, ref["loglik_t"], bar["loglik_t"])
        print(f"dtype {dtype} ({n},{p},{q},{r}) m {m}: err / bar  w {worst_w:.3g}  l_t {worst_l:.3g}")
        assert ok_w and ok_l
        assert abs(sw - float(ref["w"].sum())) <= float(bar["w"].sum()) + rob.gamma(rob.depth(n)) * float(ref["w"].sum())
        # two calls, and any grid of the row pass: bitwise the same
        ll2, sw2 = ctx.robust_weights(rb.theta_of(th), nus, keep)
        assert np.array_equal(ll, ll2) and sw == sw2 and np.array_equal(w, ctx.robust_get()[0])
        # the weights of another nu of the list are other weights
        if m > 1:
            ctx.robust_weights(rb.theta_of(th), nus, keep + 1)
            assert not rob.inside(ctx.robust_get()[0], ref["w"], bar["w"])[0]


def test_robust_sums_do_not_depend_on_the_grid():
    n, p, q, r = 2500, 5, 3, 2                                      # three row blocks
    X, Y, th = rb.make_case(n, p, q, r, seed=4)
    nus = _nus(16)
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        outs = []
        for grid in (0, 1, 2, 7):
            ctx.set_option("robust_grid", grid)
            outs.append(ctx.robust_weights(rb.theta_of(th), nus, 2) + ctx.robust_get())
        for o in outs[1:]:
            assert np.array_equal(o[0], outs[0][0]) and o[1] == outs[0][1]
            assert np.array_equal(o[2], outs[0][2]) and np.array_equal(o[3], outs[0][3])
        ref, bar = rob.reference(X, Y, th, nus, 2), rob.bars(X, Y, th, nus, 2)
        assert rob.inside(outs[0][0], ref["loglik_t"], bar["loglik_t"])[0]


def test_robust_weights_refusals_leave_everything_untouched():
    from ppls_amd import PplsError
    n, p, q, r = 70, 13, 5, 3
    X, Y, th = rb.make_case(n, p, q, r, seed=5)
    with _ctx() as ctx, _ctx() as streamed:
        ctx.set_data(X, Y)
        with pytest.raises(PplsError) as e:
            ctx.robust_get()                                        # nothing kept yet
        assert e.value.code == E_STATE
        ctx.robust_weights(rb.theta_of(th), NU)
        w0, d0 = ctx.robust_get()

        def refused(code, fn, match=None):
            with pytest.raises(PplsError, match=match) as e:
                fn()
            assert e.value.code == code
            ll, sw = ctx._robust_last                               # NaN before the call: nothing was written
            assert np.all(np.isnan(ll)) and np.all(np.isnan(sw))
            w, d = ctx.robust_get()                                 # and the kept weights survive
            assert np.array_equal(w, w0) and np.array_equal(d, d0)

        t = rb.theta_of(th)
        refused(E_ARG, lambda: ctx.robust_weights(t, np.ones(17)))
        refused(E_ARG, lambda: ctx.robust_weights(t, np.ones(0)))
        refused(E_ARG, lambda: ctx.robust_weights(t, [4.0, np.nan]))
        refused(E_ARG, lambda: ctx.robust_weights(t, [4.0, np.inf]))
        refused(E_ARG, lambda: ctx.robust_weights(t, [0.0]))
        refused(E_ARG, lambda: ctx.robust_weights(t, [-1.0, 4.0]))
        refused(E_ARG, lambda: ctx.robust_weights(t, [4.0, 5.0], keep=2))
        refused(E_ARG, lambda: ctx.robust_weights(t, [4.0, 5.0], keep=-1))
        bad = dict(th)
        bad["sigE"] = 0.0
        refused(E_ARG, lambda: ctx.robust_weights(rb.theta_of(bad), NU))
        bad = dict(th, W=np.array(th["W"]))
        bad["W"][0, 0] = np.nan
        refused(E_ARG, lambda: ctx.robust_weights(rb.theta_of(bad), NU), "non-finite")
        big = dict(th, W=np.eye(p, q + 1), C=np.ones((q, q + 1)), B=np.eye(q + 1), sigT=np.eye(q + 1))   # r > min(p, q)
        refused(E_ARG, lambda: ctx.robust_weights(rb.theta_of(big), NU))
        # a context without rows
        streamed.xprod_weighted(ctx, np.ones(n))
        with pytest.raises(PplsError, match=STREAMED) as e:
            streamed.robust_weights(t, NU)
        assert e.value.code == E_STATE


# ------------------------------------------------------------------------------ 3. xprod_weighted
N, P_, Q_, R_ = 300, 12, 9, 2


@functools.lru_cache(maxsize=None)
def _problem():
    X, Y, th0, Wt, Ct = rob.contaminated(1)
    g = rob.em_steps(X, Y, dict(th0), 60)                           # the Gaussian fit, from the oracle
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, g, Wt, Ct


def _source(dtype=0):
    X, Y, g, _, _ = _problem()
    src = _ctx(dtype)
    src.set_data(X, Y)
    return src


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_xprod_weighted_state_and_matrix(dtype):
    g = _problem()[2]
    with _source(dtype) as src, _ctx() as dst, _ctx() as host:
        src.robust_weights(_theta(g), NU)
        w, _ = src.robust_get()                                     # the weights as the device holds them
        D = np.hstack(src.get_data())
        dst.xprod_weighted(src)
        assert dst.stream_info() == dict(state="streamed", rows_local=0, n_total=N, chunks=0)   # N, not sum u
        assert dst.streamed and dst.n_local == 0 and dst.n_total == N and (dst.p, dst.q) == (P_, Q_)
        assert abs(w.sum() - N) > 1.0
        S = dst.xprod_matrix()
        ok, worst = inside(S, weighted_ref(D, w), N)
        print(f"xprod_weighted dtype {dtype}: max err / bar {worst:.3g}")
        assert ok and np.array_equal(S, S.T)
        sx, sy = 0.0, 0.0                                           # the block traces, in column order
        for j in range(P_):
            sx += S[j, j]
        for j in range(Q_):
            sy += S[P_ + j, P_ + j]
        assert dst.ssq() == (sx, sy)
        # host weights that are the device's: the same bits
        host.xprod_weighted(src, w)
        assert np.array_equal(host.xprod_matrix(padded=True)[0], dst.xprod_matrix(padded=True)[0])
        assert host.ssq() == dst.ssq() and host.n_total == N


def test_xprod_weighted_again_equals_fresh_and_leaves_the_source():
    from ppls_amd import PplsError
    g = _problem()[2]
    w1 = rob.draw_weights(N, P_ + Q_, NU, seed=1)
    w2 = rob.draw_weights(N, P_ + Q_, NU, seed=2)
    with _source() as src, _ctx() as dst, _ctx() as fresh:
        X0, Y0 = src.get_data()
        src.robust_weights(_theta(g), NU)
        kept = src.robust_get()
        dst.xprod_weighted(src, w1)
        S1 = dst.xprod_matrix()
        dst.em_begin(_theta(g))
        dst.em_iterate(3)
        dst.xprod_weighted(src, w2)
        with pytest.raises(PplsError):                              # the session on the first S is over
            dst.em_iterate(1)
        fresh.xprod_weighted(src, w2)
        assert np.array_equal(dst.xprod_matrix(padded=True)[0], fresh.xprod_matrix(padded=True)[0])
        assert dst.ssq() == fresh.ssq() and not np.array_equal(S1, dst.xprod_matrix())
        dst.xprod_weighted(src, w1)
        assert np.array_equal(dst.xprod_matrix(), S1)
        # a count-weighted S in the same dst afterwards, and back
        dst.xprod_resample(src, np.ones(N, dtype=np.int32))
        dst.xprod_weighted(src, np.ones(N))
        fresh.xprod_resample(src, np.ones(N, dtype=np.int32))
        assert np.array_equal(dst.xprod_matrix(), fresh.xprod_matrix())
        # the source: rows, kept weights and state as they were
        X1, Y1 = src.get_data()
        assert np.array_equal(X0, X1) and np.array_equal(Y0, Y1)
        assert all(np.array_equal(a, b) for a, b in zip(kept, src.robust_get()))
        assert src.stream_info()["state"] == "none" and src.n_local == N


def test_xprod_weighted_refusals():
    from ppls_amd import Context, PplsError
    g = _problem()[2]
    w = rob.draw_weights(N, P_ + Q_, NU, seed=1)
    with _source() as src, _ctx() as dst, _ctx() as empty, _ctx() as streamed:
        dst.xprod_weighted(src, w)
        S, info = dst.xprod_matrix(), dst.stream_info()

        def refused(code, fn, match=None):
            with pytest.raises(PplsError, match=match) as e:
                fn()
            assert e.value.code == code
            assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)   # dst holds what it held

        for bad in (-1e-3, np.nan, np.inf):
            v = w.copy()
            v[17] = bad
            refused(E_ARG, lambda: dst.xprod_weighted(src, v), "negative or not finite")
        refused(E_ARG, lambda: dst.xprod_weighted(src, np.zeros(N)), "all zero")
        refused(E_STATE, lambda: dst.xprod_weighted(src), "keeps none")          # NULL with nothing kept
        with pytest.raises(PplsError) as e:
            src.xprod_weighted(src, w)                                            # dst == src
        assert e.value.code == E_ARG and src.stream_info()["state"] == "none"
        wp = w.ctypes.data_as(ct.POINTER(ct.c_double))
        assert dst._L.ppls_xprod_weighted(dst.h, empty.h, wp) == E_STATE          # src without data
        streamed.xprod_weighted(src, w)
        assert dst._L.ppls_xprod_weighted(dst.h, streamed.h, wp) == E_STATE       # src streamed
        assert STREAMED.encode() in dst._L.ppls_last_error(dst.h)
        assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)
        try:
            other = Context(1)
        except PplsError:
            other = None                                                          # one GPU: no second device to refuse
        if other is not None:
            with other:
                with pytest.raises(PplsError) as e:
                    other.xprod_weighted(src, w)
                assert e.value.code == E_ARG
        with pytest.raises(ValueError):
            dst.xprod_weighted(src, w[:-1])
        # whatever replaces or rescales the rows drops the kept weights
        src.robust_weights(_theta(g), NU)
        dst.xprod_weighted(src)
        info, S = dst.stream_info(), dst.xprod_matrix()
        src.scale_data(True, False)
        refused(E_STATE, lambda: dst.xprod_weighted(src), "keeps none")
        with pytest.raises(PplsError) as e:
            src.robust_get()
        assert e.value.code == E_STATE
        src.robust_weights(_theta(g), NU)
        src.set_data(*_problem()[:2])
        refused(E_STATE, lambda: dst.xprod_weighted(src), "keeps none")


# ------------------------------------------------------------------------------ 4. fits
def _canonical(th):
    from oracle import ppls_oracle as o
    W, C, B, T = o.canonicalize(th["W"], th["C"], th["B"], th["sigT"])
    return _theta(dict(th, W=W, C=C, B=B, sigT=T))


def test_robust_fit_equals_the_written_out_loop():
    from ppls_amd import robust_PPLS_simult
    X, Y, g, Wt, Ct = _problem()
    ref = rob.oracle_loop(X, Y, dict(g), NU, outer=40, inner=5, atol=-np.inf)
    with _ctx() as ctx, _ctx() as work:
        fit = robust_PPLS_simult(X, Y, R_, NU, outer=40, inner=5, atol=-np.inf, init=g, ctx=ctx, work=work)
        assert work.h is not None and work.streamed and ctx.n_local == N          # the caller's contexts stay
    assert fit["steps"] == ref["steps"] == 40 and not fit["converged"] and fit["nu"] == NU and fit["gaussian"] is None
    _assert_fit(_theta(fit["estimates"]), fit["loglik"], None, _canonical(ref["theta"]), ref["loglik"], None)
    assert np.abs(fit["weights"] - ref["weights"]).max() < 1e-8 and np.abs(fit["d2"] / ref["d2"] - 1).max() < 1e-8
    ew, ec = rob.space_error(fit["estimates"]["W"], Wt), rob.space_error(fit["estimates"]["C"], Ct)
    print(f"W error Gaussian {rob.space_error(g['W'], Wt):.3f} robust {ew:.3f}; C error {rob.space_error(g['C'], Ct):.3f} / {ec:.3f}; "
          f"sigE {fit['estimates']['sigE']:.3f}")
    assert ew <= 0.3 and rob.space_error(g["W"], Wt) >= 1.0
    assert ec < rob.space_error(g["C"], Ct)
    assert np.all(np.diff(fit["loglik"]) >= 0)


def test_robust_fit_stops_on_atol_and_starts_from_its_own_gaussian_fit():
    from ppls_amd import robust_PPLS_simult
    X, Y, g, _, _ = _problem()
    ref = rob.oracle_loop(X, Y, dict(g), NU, outer=50, inner=5, atol=1e-2)
    with _ctx() as ctx:
        fit = robust_PPLS_simult(X, Y, R_, NU, outer=50, inner=5, atol=1e-2, init=g, ctx=ctx)
        assert fit["converged"] and fit["steps"] == ref["steps"] < 50 and len(fit["loglik"]) == fit["steps"] + 1
        own = robust_PPLS_simult(None, None, R_, NU, outer=3, ctx=ctx)            # init = None: PPLS_simult's defaults
        assert own["gaussian"]["class"] == "PPLS_simult" and own["steps"] == 3 and len(own["loglik"]) == 4
        ll = own["loglik"]
        assert np.all(np.diff(ll) >= -1e-10 * np.abs(ll[:-1]))


def test_robust_fit_on_scaled_resident_rows():
    from ppls_amd import robust_PPLS_simult
    X, Y, g, _, _ = _problem()
    with _ctx() as ctx:
        ctx.set_data(X + 0.25, Y - 0.5)
        ctx.scale_data(True, False)
        Xs, Ys = ctx.get_data()
        fit = robust_PPLS_simult(None, None, R_, NU, outer=4, inner=5, atol=-np.inf, init=g, ctx=ctx)
    ref = rob.oracle_loop(Xs, Ys, dict(g), NU, outer=4, inner=5, atol=-np.inf)
    _assert_fit(_theta(fit["estimates"]), fit["loglik"], None, _canonical(ref["theta"]), ref["loglik"], None)


def test_robust_fit_estimates_nu():
    """t_5-mixed rows: the device loop and the oracle loop choose nu from the same four-round grid search.  Each
    ends within one point of its last grid of the maximiser of its own l_t(theta, .), and the two l_t differ by
    rounding alone, so the two nu lie within two of those points of each other."""
    from ppls_amd import robust_PPLS_simult
    X, Y, th0 = rob.t_mixed(1)
    g = rob.em_steps(X, Y, dict(th0), 30)
    ref = rob.oracle_loop(X, Y, dict(g), "estimate", outer=12, inner=3, atol=-np.inf)
    with _ctx() as ctx:
        fit = robust_PPLS_simult(X, Y, 2, "estimate", outer=12, inner=3, atol=-np.inf, init=g, ctx=ctx)
    d2, logdet = rob.dense_d2_logdet(X, Y, ref["theta"])
    step = rob.best_nu(d2, logdet, X.shape[0], X.shape[1] + Y.shape[1])[2]
    print(f"nu: device {fit['nu']:.4f}, oracle {ref['nu']:.4f}, last grid ratio {step:.5f}")
    assert abs(math.log(fit["nu"] / ref["nu"])) <= 2 * math.log(step) * (1 + 1e-9)
    assert 3.0 < fit["nu"] < 8.0                                    # (the rows are t_5 about the model)
    assert np.all(np.diff(fit["loglik"]) >= 0)
    assert np.abs(fit["loglik"] / ref["loglik"] - 1).max() < 1e-8


# ------------------------------------------------------------------------------ 5. shards
SHARES = {2: [(0, 70), (70, 300)], 3: [(0, 70), (70, 300), (300, 300)]}


def _run_ranks(k, work):
    """k contexts on GPU 0 with the threaded host reducer, rank i holding the rows SHARES[k][i]."""
    X, Y = _problem()[:2]
    red = ThreadAllReduce(k)
    out, errs = [None] * k, []

    def body(rank):
        try:
            lo, hi = SHARES[k][rank]
            with _ctx() as src:
                src.set_reducer(red.fn(rank))
                src.set_data(X[lo:hi], Y[lo:hi], n_total=N)
                out[rank] = work(src, rank)
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(k)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
    if errs:
        raise errs[0]
    return out


@pytest.mark.parametrize("k", [2, 3])
def test_sharded_weights_and_cross_products(k):
    X, Y, g = _problem()[:3]
    nus = _nus(16)

    def work(src, rank):
        ll, sw = src.robust_weights(_theta(g), nus, 5)
        w, d2 = src.robust_get()
        with _ctx() as dst:
            dst.xprod_weighted(src)
            return ll, sw, w, d2, dst.xprod_matrix(), dst.ssq(), dst.stream_info()

    outs = _run_ranks(k, work)
    with _source() as one, _ctx() as dst:
        ll1, sw1 = one.robust_weights(_theta(g), nus, 5)
        w1, d1 = one.robust_get()
        dst.xprod_weighted(one)
        S1 = dst.xprod_matrix()
    ref, bar = rob.reference(X, Y, g, nus, 5), rob.bars(X, Y, g, nus, 5, ranks=k)
    Sref = weighted_ref(np.hstack([X, Y]), w1)
    for rank, (ll, sw, w, d2, S, ssq, info) in enumerate(outs):
        lo, hi = SHARES[k][rank]
        assert np.array_equal(w, w1[lo:hi]) and np.array_equal(d2, d1[lo:hi])     # a row's weight: the same bits
        assert np.array_equal(ll, outs[0][0]) and sw == outs[0][1]                # every rank: the same sums
        ok, worst = rob.inside(ll, ref["loglik_t"], bar["loglik_t"])
        print(f"{k} ranks, rank {rank}: l_t err / bar {worst:.3g}")
        assert ok and np.all(np.abs(ll - ll1) <= 2 * bar["loglik_t"])
        assert info == dict(state="streamed", rows_local=0, n_total=N, chunks=0)
        assert np.array_equal(S, outs[0][4]) and ssq == outs[0][5]
        assert inside(S, Sref, N, K_W_SHARDED)[0]
        assert np.all(np.abs(S - S1) <= weighted_bar(Sref, N, K_W_SHARDED))


@pytest.mark.parametrize("k", [2, 3])
def test_sharded_bad_weight_is_refused_on_every_rank(k):
    from ppls_amd import PplsError
    w = rob.draw_weights(N, P_ + Q_, NU, seed=1)
    w[100] = np.nan                                                               # rank 1's row

    def work(src, rank):
        lo, hi = SHARES[k][rank]
        with _ctx() as dst:
            try:
                dst.xprod_weighted(src, w[lo:hi])
            except PplsError as e:
                return e.code, dst.stream_info()["state"]
            return 0, ""

    assert _run_ranks(k, work) == [(E_ARG, "none")] * k
