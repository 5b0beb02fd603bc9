"""The weighted MFMA Gram, ppls_xprod_resample and bootstrap_PPLS_simult on the device.

References and bars are those of tests/resample_bar.py: S_ref = sum_i c_i d_i d_i' in long double over
the rows as the context stores them, |G - S_ref| <= K_W gamma(n) sqrt(S_aa S_bb) with K_W = 2 (one more
stage where a cross-rank sum follows); the unweighted Gram of the repeated rows has one stage over
N' = sum c rows.  Fits on a resampled context are compared with the same call on a resident context
that holds the repeated rows (xprod = 1), with the tolerances tests/test_gpu_stream.py::_assert_fit
uses between a streamed and a resident context: both sides differ only in the rounding of S.
"""
import ctypes as ct
import functools
import threading

import numpy as np
import pytest

from conftest import make_problem
from resample_bar import K_W, K_W_SHARDED, draw_counts, inside, weighted_bar, weighted_ref
from test_gpu_stream import STREAMED, ThreadAllReduce, _assert_fit, _relerr, _theta

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
L = np.longdouble


def _ctx(dtype=0, xprod=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", xprod)
    return c


# ------------------------------------------------------------------------------ 1. the kernel alone
# (1, 3, 2); (5, 3, 2): fewer than 2 PPLS_GRING k-steps; (27, 5, 3): steady state, a tail and a partial
# k-step (27 = 4 6 + 3); (257, 130, 3): an off-diagonal tile, a diagonal tile's dead quadrant, a padded odd
# q; (64, 70, 61): X's padding meets Y inside a quadrant
KERNEL_SHAPES = [(1, 3, 2), (5, 3, 2), (27, 5, 3), (257, 130, 3), (64, 70, 61)]


def _kernel_rows(n, p, q):
    rng = np.random.default_rng(1000 * n + 10 * p + q)

    def block(m):
        j = np.arange(m)
        return rng.standard_normal((n, m)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7
    return block(p), block(q)


def _pick(D, p, q, xory):
    return D if xory == 2 else D[:, p:] if xory else D[:, :p]


def _check_weighted(tag, G, D, c, n):
    ref = weighted_ref(D, c)
    ok, worst = inside(G, ref, n)
    print(f"{tag}: max err / bar {worst:.3g} (K_W = {K_W})")
    assert ok
    assert np.array_equal(G, G.T)                                   # exactly symmetric
    return ref


@pytest.mark.parametrize("n,p,q", KERNEL_SHAPES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_weighted_gram(dtype, n, p, q):
    X, Y = _kernel_rows(n, p, q)
    c = draw_counts(n, seed=7 * n + p) if n > 1 else np.array([2], dtype=np.int32)
    one = np.ones(n, dtype=np.int32)
    with _ctx(dtype) as ctx, _ctx(dtype) as rep:
        ctx.set_data(X, Y)
        Xs, Ys = ctx.get_data()                                     # the rows as stored (fp32: rounded)
        D = np.hstack([Xs, Ys])
        rep.set_data(np.repeat(Xs, c, axis=0), np.repeat(Ys, c, axis=0))
        nrep = int(c.sum())
        for xory in (0, 1, 2):
            Dk = _pick(D, p, q, xory)
            for nsplit in (1, 2, 3):
                tag = f"{'fp32' if dtype else 'fp64'} ({n},{p},{q}) xory {xory} nsplit {nsplit}"
                G, _ = ctx.gram(xory, nsplit, count=c)
                ref = _check_weighted(tag, G, Dk, c, n)
                # count = 1 everywhere is the unweighted kernel's result, bit for bit
                G1, _ = ctx.gram(xory, nsplit, count=one)
                G0, _ = ctx.gram(xory, nsplit)
                assert np.array_equal(G1, G0)
                # the unweighted Gram of the repeated rows: another summation, one stage over sum c rows
                Gr, _ = rep.gram(xory, nsplit)
                both = weighted_bar(ref, n) + weighted_bar(ref, nrep, 1)
                assert np.all(np.abs(G - Gr) <= both)


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_weighted_gram_with_an_all_zero_split(dtype):
    n, p, q = 27, 5, 3
    X, Y = _kernel_rows(n, p, q)
    c = draw_counts(n, seed=3)
    c[9:18] = 0                                                     # the whole middle split of three
    c[0] = 7
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        D = np.hstack(ctx.get_data())
        for xory in (0, 1, 2):
            G, _ = ctx.gram(xory, 3, count=c)
            _check_weighted(f"zero split, xory {xory}", G, _pick(D, p, q, xory), c, n)
        G, _ = ctx.gram(2, 0, count=c)                              # and the automatic plan
        _check_weighted("zero split, auto", G, D, c, n)


def test_weighted_gram_refuses_bad_counts():
    from ppls_amd import PplsError
    X, Y = _kernel_rows(5, 3, 2)
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        with pytest.raises(PplsError) as e:
            ctx.gram(2, 1, count=np.array([1, 0, -1, 2, 1], dtype=np.int32))
        assert e.value.code == E_ARG
        with pytest.raises(ValueError):
            ctx.gram(2, 1, count=np.ones(4, dtype=np.int32))
        assert ctx._L.ppls_gram_weighted(ctx.h, 2, 1, None, None, None) == E_ARG


def test_weighted_occupancy_equals_unweighted():
    with _ctx() as ctx:
        for f32 in (False, True):
            assert ctx.gram_occupancy(f32, weighted=True) == ctx.gram_occupancy(f32) >= 1


# ------------------------------------------------------------------------------ 2. xprod_resample
N, P_, Q_ = 300, 12, 9


@functools.lru_cache(maxsize=None)
def _problem():
    """tests/test_gpu_stream.py::_fit_pair's shape and data recipe."""
    X, Y, _ = make_problem(N, P_, Q_, 3, seed=21)
    X = X + 0.5
    Y = Y * 2.0 - 1.0
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def _source(dtype=0, xprod=0):
    """The data, scaled on the device."""
    X, Y = _problem()
    src = _ctx(dtype, xprod)
    src.set_data(X, Y)
    src.scale_data(True, True)
    return src


@functools.lru_cache(maxsize=None)
def _counts(seed=0):
    from ppls_amd import bootstrap_counts
    c = bootstrap_counts(N, 1, seed)[0]
    c.setflags(write=False)
    return c


def _resident_repeat(src, c, xprod=1):
    Xs, Ys = src.get_data()
    res = _ctx(0, xprod)
    res.set_data(np.repeat(Xs, c, axis=0), np.repeat(Ys, c, axis=0))
    return res


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_resample_state_and_matrix(dtype):
    c = draw_counts(N, seed=5)
    with _source(dtype) as src, _ctx() as dst:
        D = np.hstack(src.get_data())
        dst.xprod_resample(src, c)
        assert dst.stream_info() == dict(state="streamed", rows_local=0, n_total=int(c.sum()), chunks=0)
        assert dst.streamed and dst.n_local == 0 and dst.n_total == int(c.sum()) and (dst.p, dst.q) == (P_, Q_)
        assert dst.stream_fold_info()["nr_folds"] == 0
        S = dst.xprod_matrix()
        ref = weighted_ref(D, c)
        ok, worst = inside(S, ref, N)
        print(f"xprod_resample dtype {dtype}: max err / bar {worst:.3g}")
        assert ok and np.array_equal(S, S.T)
        Sp, ldx = dst.xprod_matrix(padded=True)
        live = np.zeros(Sp.shape[0], dtype=bool)
        live[:P_] = True
        live[ldx:ldx + Q_] = True
        assert not Sp[~live].any() and not Sp[:, ~live].any() and np.array_equal(Sp[np.ix_(live, live)], S)
        sx, sy = 0.0, 0.0                                           # the block traces, in column order
        for j in range(P_):
            sx += S[j, j]
        for j in range(Q_):
            sy += S[P_ + j, P_ + j]
        assert dst.ssq() == (sx, sy)
        a, b = dst.scaling(), src.scaling()
        for k in a:
            assert np.array_equal(a[k], b[k])
        assert np.abs(a["centerX"]).max() > 0                       # (src's record is not the identity)


@pytest.mark.parametrize("r", [1, 3, 8])
def test_em_run_on_resampled_context(r):
    c = _counts()
    with _source() as src, _ctx() as dst:
        dst.xprod_resample(src, c)
        with _resident_repeat(src, c) as res:
            th0 = make_problem(N, P_, Q_, r, seed=5 + r)[2]
            ref = res.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)
            got = dst.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)
            _assert_fit(got[0], got[1], got[2], ref[0], ref[1], ref[2])
            e, e_ref = dst.estep(_theta(th0), want_mu=False), res.estep(_theta(th0), want_mu=False)
            assert _relerr(e.Chh, e_ref.Chh) < 1e-8 and abs(e.Cee / e_ref.Cee - 1) < 1e-8
            assert abs(dst.loglik(_theta(th0)) / res.loglik(_theta(th0)) - 1) < 1e-10


def test_session_ppls_and_ppls_simult_on_resampled_context():
    from ppls_amd import PPLS, PPLS_simult
    c = _counts()
    with _source() as src, _ctx() as dst:
        dst.xprod_resample(src, c)
        with _resident_repeat(src, c) as res:
            th0 = make_problem(N, P_, Q_, 3, seed=8)[2]
            outs = []
            for k in (dst, res):
                k.em_begin(_theta(th0))
                k.em_iterate(10)
                k.em_iterate(15)
                outs.append(k.em_state())
            (est, ll), (ref_est, ref_ll) = outs
            assert len(ll) == 24
            _assert_fit(est, ll, None, ref_est, ref_ll, None)
            # the sequential PPLS: the building block serves it
            fit = PPLS(None, None, 3, 200, 1e-4, "equal", ctx=dst)
            ref = PPLS(None, None, 3, 200, 1e-4, "equal", ctx=res)
            assert np.array_equal(fit["Other_output"]["Number_steps"], ref["Other_output"]["Number_steps"])
            assert np.abs(fit["W"] - ref["W"]).max() < 1e-8 and np.abs(fit["C"] - ref["C"]).max() < 1e-8
            assert _relerr(fit["B"], ref["B"]) < 1e-8 and _relerr(fit["sig"], ref["sig"]) < 1e-8
            assert _relerr(fit["Other_output"]["Loglikelihoods"], ref["Other_output"]["Loglikelihoods"]) < 1e-10
            init = dict(W=ref["W"], C=ref["C"], B=np.diag(ref["B"]), sigE=ref["sig"][2, 0], sigF=ref["sig"][2, 1],
                        sigH=ref["sig"][2, 2], sigT=np.diag(ref["sig"][:, 3]))
            sim = PPLS_simult(None, None, 3, 15, -np.inf, init=init, ctx=dst)
            sim_ref = PPLS_simult(None, None, 3, 15, -np.inf, init=init, ctx=res)
            E, Er = sim["Expectations"], sim_ref["Expectations"]
            assert E["mu_T"] is None and E["mu_U"] is None
            for k in ("Ctt", "Cuu", "Cut", "Cee", "Cff", "Chh"):
                assert _relerr(E[k], Er[k]) < 1e-8
            assert len(sim["loglik"]) == len(sim_ref["loglik"]) and _relerr(sim["loglik"], sim_ref["loglik"]) < 1e-10
            assert np.abs(sim["estimates"]["W"] - sim_ref["estimates"]["W"]).max() < 1e-8
            assert np.abs(sim["estimates"]["C"] - sim_ref["estimates"]["C"]).max() < 1e-8


def test_second_resample_equals_a_fresh_one_and_ends_the_session():
    from ppls_amd import PplsError
    c1, c2 = _counts(1), _counts(2)
    with _source() as src, _ctx() as dst, _ctx() as fresh:
        dst.xprod_resample(src, c1)
        S1 = dst.xprod_matrix()
        dst.em_begin(_theta(make_problem(N, P_, Q_, 3, seed=8)[2]))
        dst.em_iterate(3)
        dst.xprod_resample(src, c2)
        with pytest.raises(PplsError):                              # the session of the first replicate is over
            dst.em_iterate(1)
        fresh.xprod_resample(src, c2)
        assert np.array_equal(dst.xprod_matrix(padded=True)[0], fresh.xprod_matrix(padded=True)[0])
        assert dst.ssq() == fresh.ssq() and dst.n_total == fresh.n_total == int(c2.sum())
        assert not np.array_equal(S1, dst.xprod_matrix())
        dst.xprod_resample(src, c1)                                 # and back: the first one, bit for bit
        assert np.array_equal(dst.xprod_matrix(), S1)


def test_source_is_left_untouched():
    th0 = make_problem(N, P_, Q_, 3, seed=8)[2]
    with _source(0, 1) as src, _source(0, 1) as twin, _ctx() as dst:
        X0, Y0 = src.get_data()
        for k in (src, twin):
            k.em_begin(_theta(th0))
            k.em_iterate(5)
        S0 = src.xprod_matrix()
        dst.xprod_resample(src, _counts(3))
        for k in (src, twin):
            k.em_iterate(5)
        (est, ll), (t_est, t_ll) = src.em_state(), twin.em_state()
        assert np.array_equal(ll, t_ll) and len(ll) == 9
        for k in ("W", "C", "B", "sigT"):
            assert np.array_equal(getattr(est, k), getattr(t_est, k))
        assert (est.sigE, est.sigF, est.sigH) == (t_est.sigE, t_est.sigF, t_est.sigH)
        X1, Y1 = src.get_data()
        assert np.array_equal(X0, X1) and np.array_equal(Y0, Y1)
        assert np.array_equal(S0, src.xprod_matrix()) and np.array_equal(S0, twin.xprod_matrix())
        assert src.stream_info()["state"] == "none" and src.n_local == N


def test_refusals():
    from ppls_amd import Context, PplsError
    c = _counts()
    with _source() as src, _ctx() as dst, _ctx() as empty, _ctx() as streamed:
        dst.xprod_resample(src, c)
        S = dst.xprod_matrix()
        info = dst.stream_info()

        def refused(code, fn, match=None):
            with pytest.raises(PplsError, match=match) as e:
                fn()
            assert e.value.code == code
            assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)   # dst holds what it held

        neg = np.array(c)
        neg[17] = -1
        refused(E_ARG, lambda: dst.xprod_resample(src, neg), "negative")
        refused(E_ARG, lambda: dst.xprod_resample(src, np.zeros(N, dtype=np.int32)), "sum to 0")
        with pytest.raises(PplsError) as e:
            src.xprod_resample(src, c)                                  # dst == src
        assert e.value.code == E_ARG and src.stream_info()["state"] == "none"
        assert dst._L.ppls_xprod_resample(dst.h, src.h, None) == E_ARG  # count == NULL with rows
        assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)
        cp = np.ascontiguousarray(c).ctypes.data_as(ct.POINTER(ct.c_int32))
        assert dst._L.ppls_xprod_resample(dst.h, empty.h, cp) == E_STATE  # src without data
        assert b"no data" in dst._L.ppls_last_error(dst.h)
        streamed.xprod_resample(src, c)
        assert dst._L.ppls_xprod_resample(dst.h, streamed.h, cp) == E_STATE   # src streamed
        assert STREAMED.encode() in dst._L.ppls_last_error(dst.h)
        assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)
        try:
            other = Context(1)
        except PplsError:
            other = None                                                # one GPU: no second device to refuse
        if other is not None:
            with other:
                with pytest.raises(PplsError) as e:
                    other.xprod_resample(src, c)
                assert e.value.code == E_ARG
        with pytest.raises(ValueError):
            dst.xprod_resample(src, c[:-1])
        with pytest.raises(ValueError):
            dst.xprod_resample(src, c.astype(np.float64))
        # what needs rows is refused with the streamed message
        with pytest.raises(PplsError, match=STREAMED) as e:
            dst.scores(np.ones((P_, 1)), np.ones((Q_, 1)))
        assert e.value.code == E_STATE
        with pytest.raises(PplsError, match=STREAMED) as e:
            dst.variances(np.zeros((0, 1)), np.ones(1), 0.5, 0)
        assert e.value.code == E_STATE
        with pytest.raises(PplsError, match=STREAMED):
            dst.get_data(0, 0)
        # a context that held resident rows before becomes a resampled one all the same
        with _source() as was:
            was.xprod_resample(src, c)
            assert was.streamed and np.array_equal(was.xprod_matrix(), S)


# ------------------------------------------------------------------------------ 3. shards
SHARES = [(0, 70), (70, 300), (300, 300)]


def _run_ranks(work):
    """Three contexts on GPU 0 with the threaded host reducer, rank i holding the rows SHARES[i] of the
    scaled data; work(src, rank) runs on every rank."""
    with _source() as one:
        Xs, Ys = one.get_data()
    red = ThreadAllReduce(3)
    out, errs = [None] * 3, []

    def body(rank):
        try:
            lo, hi = SHARES[rank]
            with _ctx() as src:
                src.set_reducer(red.fn(rank))
                src.set_data(Xs[lo:hi], Ys[lo:hi], n_total=N)
                out[rank] = work(src, rank)
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
    return out, np.hstack([Xs, Ys])


def test_sharded_resample_equals_one_context():
    c = _counts(4)

    def work(src, rank):
        lo, hi = SHARES[rank]
        with _ctx() as dst:
            dst.xprod_resample(src, c[lo:hi])
            return dst.xprod_matrix(), dst.ssq(), dst.stream_info()

    outs, D = _run_ranks(work)
    ref = weighted_ref(D, c)
    with _source() as src, _ctx() as dst:
        dst.xprod_resample(src, c)
        S1 = dst.xprod_matrix()
    for rank, (S, ssq, info) in enumerate(outs):
        assert info == dict(state="streamed", rows_local=0, n_total=int(c.sum()), chunks=0)
        assert np.array_equal(S, outs[0][0]) and ssq == outs[0][1]      # every rank holds the same S
        ok, worst = inside(S, ref, N, K_W_SHARDED)
        print(f"rank {rank}: max err / bar {worst:.3g} (K = {K_W_SHARDED})")
        assert ok
        assert np.all(np.abs(S - S1) <= weighted_bar(ref, N, K_W_SHARDED))


def test_sharded_negative_count_is_refused_on_every_rank():
    from ppls_amd import PplsError
    c = np.array(_counts(4))
    c[100] = -3                                                         # rank 1's row

    def work(src, rank):
        lo, hi = SHARES[rank]
        with _ctx() as dst:
            try:
                dst.xprod_resample(src, c[lo:hi])
            except PplsError as e:
                return e.code, dst.stream_info()["state"]
            return 0, ""

    outs, _ = _run_ranks(work)
    assert outs == [(E_ARG, "none")] * 3


# ------------------------------------------------------------------------------ 4. bootstrap_PPLS_simult
BN, BP, BQ, BA, NBOOT = 400, 7, 5, 2, 8
BSTEPS, BATOL = 30, -np.inf


@functools.lru_cache(maxsize=None)
def _boot_problem():
    X, Y, th0 = make_problem(BN, BP, BQ, BA, seed=31)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y, th0


def _boot_fit(ctx):
    from ppls_amd import PPLS_simult
    th0 = _boot_problem()[2]
    return PPLS_simult(None, None, BA, 50, 1e-4, init=th0, ctx=ctx)


def _written_out(ctx, fit, counts):
    """The same loop with np.repeat + set_data + PPLS_simult(init = the fit's estimates) + align_signs."""
    from ppls_amd import PPLS_simult, PplsError, align_signs, bootstrap_summary
    Xs, Ys = ctx.get_data()
    est0 = fit["estimates"]
    reps, failed = [], []
    with _ctx(0, 1) as res:
        for b in range(counts.shape[0]):
            res.set_data(np.repeat(Xs, counts[b], axis=0), np.repeat(Ys, counts[b], axis=0))
            try:
                f = PPLS_simult(None, None, BA, BSTEPS, BATOL, "SVD", init=est0, ctx=res)
            except PplsError:
                failed.append(b)
                continue
            e = dict(f["estimates"])
            e["W"], e["C"] = align_signs(e["W"], est0["W"]), align_signs(e["C"], est0["C"])
            reps.append(e)
    return bootstrap_summary(reps, 0.95), reps, failed


def _close(a, b, tol=1e-8):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


def test_bootstrap_equals_the_written_out_loop():
    from ppls_amd import bootstrap_PPLS_simult, bootstrap_counts
    X, Y, _ = _boot_problem()
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        fit = _boot_fit(ctx)
        out = bootstrap_PPLS_simult(fit, None, None, NBOOT, BSTEPS, BATOL, rng=77, ctx=ctx, keep=True)
        again = bootstrap_PPLS_simult(fit, None, None, NBOOT, BSTEPS, BATOL, rng=77, ctx=ctx, keep=True)
        counts = bootstrap_counts(BN, NBOOT, 77)
        given = bootstrap_PPLS_simult(fit, None, None, EMsteps=BSTEPS, atol=BATOL, ctx=ctx, counts=counts)
        (se, ci), reps, failed = _written_out(ctx, fit, counts)
        assert ctx.stream_info()["state"] == "none" and ctx.n_local == BN     # the rows stay where they are
    assert out["nboot"] == NBOOT and out["failed"] == failed == [] and len(set(out["steps"])) == 1 and out["steps"][0] > 0
    assert len(out["replicates"]) == NBOOT and "replicates" not in given
    for k in ("W", "C", "B", "sigE", "sigF", "sigH", "sigT"):
        assert np.all(np.asarray(out["se"][k]) > 0)
        assert _close(out["se"][k], se[k]) and _close(out["ci"][k][0], ci[k][0]) and _close(out["ci"][k][1], ci[k][1])
        # the same seed: bitwise the same, and so are the counts passed in
        assert np.array_equal(out["se"][k], again["se"][k]) and np.array_equal(out["se"][k], given["se"][k])
        for j in (0, 1):
            assert np.array_equal(out["ci"][k][j], again["ci"][k][j])
        for b in range(NBOOT):
            assert np.array_equal(out["replicates"][b][k], again["replicates"][b][k])
            assert _close(out["replicates"][b][k], reps[b][k])
    est0 = fit["estimates"]
    for e in out["replicates"]:                                               # aligned with the fit, each against its own
        assert np.all(np.einsum("ij,ij->j", e["W"], est0["W"]) > 0) and np.all(np.einsum("ij,ij->j", e["C"], est0["C"]) > 0)
    assert out["se"]["W"].shape == (BP, BA) and out["se"]["B"].shape == (BA,) and np.ndim(out["se"]["sigE"]) == 0


def test_bootstrap_skips_a_failed_replicate():
    """Replicate 2 draws one row N times: S_c has rank one and, without a stop rule (atol = -Inf), the
    reference's fit stops on it -- the CPU oracle's svd() raises on the non-finite X'mu_T within 30
    steps (with atol = 1e-4 it would end quietly on a negative increment instead, so the test fits
    without the stop rule)."""
    from ppls_amd import bootstrap_PPLS_simult, bootstrap_counts, bootstrap_summary
    X, Y, _ = _boot_problem()
    counts = bootstrap_counts(BN, NBOOT, 5)
    counts[2] = 0
    counts[2, 17] = BN
    with _ctx() as ctx, _ctx() as work:
        ctx.set_data(X, Y)
        fit = _boot_fit(ctx)
        out = bootstrap_PPLS_simult(fit, None, None, EMsteps=BSTEPS, atol=BATOL, ctx=ctx, work=work, keep=True,
                                    counts=counts)
        assert work.h is not None and work.streamed                            # the caller's work context stays open
        (se, ci), reps, failed = _written_out(ctx, fit, counts)
        with pytest.raises(ValueError, match="needs two"):
            bootstrap_PPLS_simult(fit, None, None, EMsteps=BSTEPS, atol=BATOL, ctx=ctx, counts=counts[[2, 2, 0]])
    assert out["failed"] == [2] == failed and out["nboot"] == NBOOT and out["steps"][2] == 0
    assert len(out["replicates"]) == NBOOT - 1
    want_se, _ = bootstrap_summary(out["replicates"])
    for k in want_se:
        assert np.array_equal(out["se"][k], want_se[k]) and _close(out["se"][k], se[k])


def test_bootstrap_with_the_default_initialiser_and_given_data():
    from ppls_amd import bootstrap_PPLS_simult
    X, Y, _ = _boot_problem()
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        fit = _boot_fit(ctx)
        a = bootstrap_PPLS_simult(fit, X, Y, 4, 20, 1e-4, init=None, rng=3, ctx=ctx)
        b = bootstrap_PPLS_simult(fit, X, Y, 4, 20, 1e-4, init=None, rng=3, ctx=ctx)
    assert a["nboot"] == 4 and len(a["steps"]) == 4
    for k in a["se"]:
        assert np.all(np.isfinite(a["se"][k])) and np.array_equal(a["se"][k], b["se"][k])
    with pytest.raises(ValueError, match="init"):
        bootstrap_PPLS_simult(fit, X, Y, 4, init="random")
