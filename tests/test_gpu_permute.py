"""The permuted cross block, ppls_xprod_permute and permutation_PPLS on the device.

References and bars are those of tests/permute_bar.py: C_ref = sum_i x_i y_perm[i]' in long double over the
rows as the context stores them, |C - C_ref| <= K_P gamma(n + nsplit) outer(dx, dy) with K_P = 1 (one more
stage where a cross-rank sum follows).  Fits on a permuted context are compared with the same call on a
resident context loaded with (X, Y[perm]) under xprod = 1, with the tolerances
tests/test_gpu_stream.py::_assert_fit uses between a streamed and a resident context: both sides differ
only in the rounding of S.
"""
import ctypes as ct
import functools
import threading

import numpy as np
import pytest

from conftest import make_problem
from permute_bar import K_P, K_P_SHARDED, inside, permutations, permuted_bar, permuted_ref
from test_gpu_resample import KERNEL_SHAPES, N, P_, Q_, SHARES, _ctx, _kernel_rows, _problem, _source
from test_gpu_stream import STREAMED, ThreadAllReduce, _assert_fit, _relerr, _theta

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4

# ------------------------------------------------------------------------------ 1. the kernel alone
# tests/test_gpu_resample.py's shapes, for its reasons row by row, and (33, 3, 130): q spans more than one
# quadrant column while p does not
SHAPES = KERNEL_SHAPES + [(33, 3, 130)]


@pytest.mark.parametrize("n,p,q", SHAPES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_permuted_cross_block(dtype, n, p, q):
    X, Y = _kernel_rows(n, p, q)
    with _ctx(dtype) as ctx:
        ctx.set_data(X, Y)
        Xs, Ys = ctx.get_data()                                     # the rows as stored (fp32: rounded)
        G2 = ctx.gram(2)[0]
        for name, perm in permutations(n, seed=7 * n + p).items():
            ref = permuted_ref(Xs, Ys, perm)
            for nsplit in (0, 3):
                bar = permuted_bar(Xs, Ys, n, nsplit)
                C, ms = ctx.gram_permuted(perm, nsplit)
                ok, worst = inside(C, ref, bar)
                print(f"{'fp32' if dtype else 'fp64'} ({n},{p},{q}) {name} nsplit {nsplit}: max err / bar {worst:.3g} "
                      f"(K_P = {K_P})")
                assert ok and C.shape == (p, q) and ms >= 0.0
                again, _ = ctx.gram_permuted(perm, nsplit)
                assert np.array_equal(C, again)                     # the same call, the same bits
                if name == "identity":                              # the joint Gram's X'Y block: another summation
                    both = bar + permuted_bar(Xs, Ys, n, 1)
                    assert np.all(np.abs(C - G2[:p, p:]) <= both)
        assert ctx.gram_permuted(np.arange(n), 0, want=False)[0] is None


def test_gram_occupancies_are_the_parent_commits():
    """The new kernel is a translation unit of its own: the joint Gram's instantiations keep their code and
    their occupancy.  2 workgroups per compute unit is what the commit before this feature returns for
    all four (fp64 / fp32 storage, unweighted / weighted; profiles/bootstrap_c3.json and _c5.json record it)."""
    with _ctx() as ctx:
        for f32 in (False, True):
            assert ctx.gram_occupancy(f32) == 2
            assert ctx.gram_occupancy(f32, weighted=True) == 2
            assert ctx.xperm_occupancy(f32) >= 1


def test_kernel_refuses_bad_permutations():
    from ppls_amd import PplsError
    X, Y = _kernel_rows(5, 3, 2)
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        for bad, match in (([0, 1, 1, 3, 4], "repeats"), ([0, 1, 2, 3, 5], "out of range"), ([0, -1, 2, 3, 4], "out of range")):
            with pytest.raises(PplsError, match=match) as e:
                ctx.gram_permuted(np.array(bad))
            assert e.value.code == E_ARG
        with pytest.raises(ValueError):
            ctx.gram_permuted(np.arange(4))
        assert ctx._L.ppls_xgram_permuted(ctx.h, 0, None, None, None) == E_ARG
        with pytest.raises(PplsError) as e:
            ctx.gram_permuted(np.arange(5), nsplit=65)
        assert e.value.code == E_ARG


# ------------------------------------------------------------------------------ 2. xprod_permute
@functools.lru_cache(maxsize=None)
def _perm(seed=0):
    from ppls_amd import permutation_indices
    perm = permutation_indices(N, 1, seed)[0]
    perm.setflags(write=False)
    return perm


def _resident_permuted(src, perm, xprod=1):
    Xs, Ys = src.get_data()
    res = _ctx(0, xprod)
    res.set_data(Xs, Ys[perm])
    return res


def _blocks(S):
    return S[:P_, :P_], S[P_:, P_:], S[:P_, P_:]


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_permute_state_and_matrix(dtype):
    perm = _perm(5)
    with _source(dtype) as src, _ctx() as dst:
        Xs, Ys = src.get_data()
        assert not src.xprod_info()["ready"]
        dst.xprod_permute(src, perm)
        assert src.xprod_info()["ready"]                            # src without S gets one, and keeps it
        assert dst.stream_info() == dict(state="streamed", rows_local=0, n_total=N, chunks=0)
        assert dst.streamed and dst.n_local == 0 and dst.n_total == N and (dst.p, dst.q) == (P_, Q_)
        assert dst.stream_fold_info()["nr_folds"] == 0
        S, S0 = dst.xprod_matrix(), src.xprod_matrix()
        assert np.array_equal(S, S.T)                               # exactly symmetric
        xx, yy, xy = _blocks(S)
        xx0, yy0, _ = _blocks(S0)
        assert np.array_equal(xx, xx0) and np.array_equal(yy, yy0)  # the diagonal blocks: src's, bit for bit
        ok, worst = inside(xy, permuted_ref(Xs, Ys, perm), permuted_bar(Xs, Ys, N, 0))
        print(f"xprod_permute dtype {dtype}: max err / bar {worst:.3g}")
        assert ok
        Sp, ldx = dst.xprod_matrix(padded=True)
        live = np.zeros(Sp.shape[0], dtype=bool)
        live[:P_] = True
        live[ldx:ldx + Q_] = True
        assert not Sp[~live].any() and not Sp[:, ~live].any() and np.array_equal(Sp[np.ix_(live, live)], S)
        assert dst.ssq() == src.ssq()
        a, b = dst.scaling(), src.scaling()
        for k in a:
            assert np.array_equal(a[k], b[k])
        assert np.abs(a["centerX"]).max() > 0                       # (src's record is not the identity)


@pytest.mark.parametrize("r", [1, 3])
def test_em_run_on_permuted_context(r):
    perm = _perm()
    with _source() as src, _ctx() as dst:
        dst.xprod_permute(src, perm)
        with _resident_permuted(src, perm) as res:
            th0 = make_problem(N, P_, Q_, r, seed=5 + r)[2]
            ref = res.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)
            got = dst.em_run(_theta(th0), 25, -np.inf, 0, want_mu=False)
            _assert_fit(got[0], got[1], got[2], ref[0], ref[1], ref[2])


def test_ppls_and_ppls_simult_on_permuted_context():
    from ppls_amd import PPLS, PPLS_simult
    perm = _perm()
    with _source() as src, _ctx() as dst:
        dst.xprod_permute(src, perm)
        with _resident_permuted(src, perm) as res:
            fit = PPLS(None, None, 3, 200, 1e-4, "o2m_xprod", ctx=dst)
            ref = PPLS(None, None, 3, 200, 1e-4, "o2m_xprod", ctx=res)
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


def test_second_permute_equals_a_fresh_one_and_ends_the_session():
    from ppls_amd import PplsError
    p1, p2 = _perm(1), _perm(2)
    with _source() as src, _ctx() as dst, _ctx() as fresh:
        dst.xprod_permute(src, p1)
        S1 = dst.xprod_matrix()
        dst.em_begin(_theta(make_problem(N, P_, Q_, 3, seed=8)[2]))
        dst.em_iterate(3)
        dst.xprod_permute(src, p2)
        with pytest.raises(PplsError):                              # the session of the first replicate is over
            dst.em_iterate(1)
        fresh.xprod_permute(src, p2)
        assert np.array_equal(dst.xprod_matrix(padded=True)[0], fresh.xprod_matrix(padded=True)[0])
        assert dst.ssq() == fresh.ssq() and dst.n_total == fresh.n_total == N
        assert not np.array_equal(S1, dst.xprod_matrix())
        dst.xprod_permute(src, p1)                                  # and back: the first one, bit for bit
        assert np.array_equal(dst.xprod_matrix(), S1)
        # a destination that held another source's replicate, or a bootstrap replicate, takes this source's
        # diagonal blocks all the same
        with _ctx() as other:
            X, Y = _problem()
            other.set_data(X * 2.0, Y + 1.0)
            dst.xprod_permute(other, p1)
            dst.xprod_permute(src, p1)
            assert np.array_equal(dst.xprod_matrix(), S1)
        from ppls_amd import bootstrap_counts
        dst.xprod_resample(src, bootstrap_counts(N, 1, 3)[0])
        dst.xprod_permute(src, p1)
        assert np.array_equal(dst.xprod_matrix(), S1) and dst.n_total == N


def test_source_is_left_untouched():
    th0 = make_problem(N, P_, Q_, 3, seed=8)[2]
    with _source(0, 1) as src, _source(0, 1) as twin, _ctx() as dst:
        X0, Y0 = src.get_data()
        for k in (src, twin):
            k.em_begin(_theta(th0))
            k.em_iterate(5)
        S0 = src.xprod_matrix()
        dst.xprod_permute(src, _perm(3))
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
    perm = _perm()
    with _source() as src, _ctx() as dst, _ctx() as empty, _ctx() as streamed:
        dst.xprod_permute(src, perm)
        S = dst.xprod_matrix()
        info = dst.stream_info()

        def refused(code, fn, match=None):
            with pytest.raises(PplsError, match=match) as e:
                fn()
            assert e.value.code == code
            assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)   # dst holds what it held

        rep = np.array(perm)
        rep[17] = rep[18]
        refused(E_ARG, lambda: dst.xprod_permute(src, rep), "repeats")
        neg = np.array(perm)
        neg[17] = -1
        refused(E_ARG, lambda: dst.xprod_permute(src, neg), "out of range")
        big = np.array(perm)
        big[17] = N
        refused(E_ARG, lambda: dst.xprod_permute(src, big), "out of range")
        with pytest.raises(ValueError):
            dst.xprod_permute(src, perm[:-1])                           # wrong length
        with pytest.raises(ValueError):
            dst.xprod_permute(src, perm.astype(np.float64))
        assert dst._L.ppls_xprod_permute(dst.h, src.h, None) == E_ARG   # perm == NULL with rows
        assert b"NULL permutation" in dst._L.ppls_last_error(dst.h)
        assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)
        with pytest.raises(PplsError, match="same context") as e:
            src.xprod_permute(src, perm)                                # dst == src
        assert e.value.code == E_ARG and src.stream_info()["state"] == "none"
        pp = np.ascontiguousarray(perm).ctypes.data_as(ct.POINTER(ct.c_int64))
        assert dst._L.ppls_xprod_permute(dst.h, empty.h, pp) == E_STATE  # src without data
        assert b"no data" in dst._L.ppls_last_error(dst.h)
        streamed.xprod_permute(src, perm)
        assert dst._L.ppls_xprod_permute(dst.h, streamed.h, pp) == E_STATE   # src streamed
        assert STREAMED.encode() in dst._L.ppls_last_error(dst.h)
        assert dst.stream_info() == info and np.array_equal(dst.xprod_matrix(), S)
        try:
            other = Context(1)
        except PplsError:
            other = None                                                # one GPU: no second device to refuse
        if other is not None:
            with other:
                with pytest.raises(PplsError) as e:
                    other.xprod_permute(src, perm)
                assert e.value.code == E_ARG
        # what needs rows is refused with the streamed message
        with pytest.raises(PplsError, match=STREAMED) as e:
            dst.scores(np.ones((P_, 1)), np.ones((Q_, 1)))
        assert e.value.code == E_STATE
        with pytest.raises(PplsError, match=STREAMED):
            dst.get_data(0, 0)
        with pytest.raises(PplsError, match=STREAMED):
            dst.gram_permuted(np.arange(0))
        # a context that held resident rows before becomes a permuted one all the same
        with _source() as was:
            was.xprod_permute(src, perm)
            assert was.streamed and np.array_equal(was.xprod_matrix(), S)


# ------------------------------------------------------------------------------ 3. shards
def _run_ranks(work):
    """tests/test_gpu_resample.py::_run_ranks: three contexts on GPU 0 with the threaded host reducer, rank i
    holding the rows SHARES[i] of the scaled data; work(src, rank) runs on every rank."""
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
    return out, Xs, Ys


def _shard_perms(seed):
    """One permutation within each shard, and the block-diagonal permutation of all rows they make."""
    rng = np.random.default_rng(seed)
    local = [rng.permutation(hi - lo).astype(np.int64) for lo, hi in SHARES]
    return local, np.concatenate([lo + pl for (lo, _), pl in zip(SHARES, local)])


def test_sharded_permute_equals_one_context():
    local, whole = _shard_perms(4)

    def work(src, rank):
        with _ctx() as dst:
            dst.xprod_permute(src, local[rank])
            return dst.xprod_matrix(), dst.ssq(), dst.stream_info(), src.xprod_matrix()

    outs, Xs, Ys = _run_ranks(work)
    ref = permuted_ref(Xs, Ys, whole)
    bar = permuted_bar(Xs, Ys, N, 0, K_P_SHARDED)
    with _source() as src, _ctx() as dst:
        dst.xprod_permute(src, whole)
        S1 = dst.xprod_matrix()
    for rank, (S, ssq, info, S_src) in enumerate(outs):
        assert info == dict(state="streamed", rows_local=0, n_total=N, chunks=0)
        assert np.array_equal(S, outs[0][0]) and ssq == outs[0][1]      # every rank holds the same S
        assert np.array_equal(S, S.T)
        xx, yy, xy = _blocks(S)
        xx0, yy0, _ = _blocks(S_src)
        assert np.array_equal(xx, xx0) and np.array_equal(yy, yy0)      # the sharded source's own diagonal blocks
        ok, worst = inside(xy, ref, bar)
        print(f"rank {rank}: max err / bar {worst:.3g} (K = {K_P_SHARDED})")
        assert ok
        assert np.all(np.abs(xy - _blocks(S1)[2]) <= bar + permuted_bar(Xs, Ys, N, 0))


def test_sharded_bad_index_is_refused_on_every_rank():
    from ppls_amd import PplsError
    local, _ = _shard_perms(4)
    local[1] = np.array(local[1])
    local[1][30] = local[1][31]                                         # rank 1 repeats a row

    def work(src, rank):
        with _ctx() as dst:
            try:
                dst.xprod_permute(src, local[rank])
            except PplsError as e:
                return e.code, dst.stream_info()["state"]
            return 0, ""

    outs, _, _ = _run_ranks(work)
    assert outs == [(E_ARG, "none")] * 3


# ------------------------------------------------------------------------------ 4. permutation_PPLS
TN, TP, TQ, TA, NPERM = 120, 8, 6, 2, 19
TSTEPS, TATOL = 100, 1e-4


@functools.lru_cache(maxsize=None)
def _test_problem():
    X, Y, _ = make_problem(TN, TP, TQ, TA, seed=31)                     # a strong planted link (B = 1.5, 1.1)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def _written_out(ctx, fit, perms):
    """The same loop with xprod_permute + PPLS, the statistics and the p-values by hand."""
    import warnings
    from ppls_amd import PPLS, PplsError
    obs = dict(B=np.abs(fit["B"]), cov=np.abs(fit["B"]) * fit["sig"][:, 3] ** 2,
               loglik=np.asarray(fit["Other_output"]["Loglikelihoods"]))
    null = {k: np.full((perms.shape[0], TA), np.nan) for k in obs}
    failed = []
    with _ctx() as work:
        for b in range(perms.shape[0]):
            try:
                work.xprod_permute(ctx, perms[b])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    f = PPLS(None, None, TA, TSTEPS, TATOL, "o2m_xprod", ctx=work)
            except PplsError:
                failed.append(b)
                continue
            k = len(f["B"])
            null["B"][b, :k] = np.abs(f["B"])
            null["cov"][b, :k] = np.abs(f["B"]) * f["sig"][:, 3] ** 2
            null["loglik"][b, :k] = f["Other_output"]["Loglikelihoods"]
    pv = {}
    for key in obs:
        pv[key] = np.array([(1 + sum(1 for v in null[key][:, k] if v >= obs[key][k])) /
                            (1 + sum(1 for v in null[key][:, k] if not np.isnan(v))) for k in range(TA)])
    return obs, null, pv, failed


def test_permutation_ppls_equals_the_written_out_loop():
    from ppls_amd import PPLS, permutation_PPLS, permutation_indices
    X, Y = _test_problem()
    with _ctx() as ctx:
        ctx.set_data(X, Y)
        ctx.scale_data(True, False)
        fit = PPLS(None, None, TA, TSTEPS, TATOL, "o2m_xprod", ctx=ctx)
        assert len(fit["B"]) == TA
        out = permutation_PPLS(fit, None, None, NPERM, TSTEPS, TATOL, rng=77, ctx=ctx, keep=True)
        again = permutation_PPLS(fit, None, None, NPERM, TSTEPS, TATOL, rng=77, ctx=ctx)
        perms = permutation_indices(TN, NPERM, 77)
        given = permutation_PPLS(fit, None, None, EMsteps=TSTEPS, atol=TATOL, ctx=ctx, perms=perms)
        obs, null, pv, failed = _written_out(ctx, fit, perms)
        assert ctx.stream_info()["state"] == "none" and ctx.n_local == TN      # the rows stay where they are
    assert out["nperm"] == NPERM and out["failed"] == failed == [] and min(out["steps"]) > 0
    assert len(out["replicates"]) == NPERM and "replicates" not in given
    for key in ("B", "cov", "loglik"):
        assert out["null"][key].shape == (NPERM, TA) and not np.isnan(out["null"][key]).any()
        assert np.array_equal(out["observed"][key], obs[key])
        assert np.abs(out["null"][key] - null[key]).max() <= 1e-8 * np.abs(null[key]).max()
        assert np.array_equal(out["pvalue"][key], pv[key])
        assert np.array_equal(out["null"][key], again["null"][key]) and np.array_equal(out["null"][key], given["null"][key])
        assert np.array_equal(out["pvalue"][key], again["pvalue"][key])
    assert out["pvalue"]["loglik"][0] == 1 / 20                          # the planted link beats every replicate
    assert out["pvalue"]["B"][0] == 1 / 20 and out["pvalue"]["cov"][0] == 1 / 20


def test_permutation_ppls_skips_a_failed_replicate():
    """Replicate 2 is no permutation (a row twice): xprod_permute refuses it, the replicate is listed and
    skipped, the work context keeps the replicate before it and stays open."""
    from ppls_amd import PPLS, permutation_PPLS, permutation_indices, permutation_pvalues
    X, Y = _test_problem()
    perms = permutation_indices(TN, NPERM, 5)
    perms[2, 7] = perms[2, 8]
    with _ctx() as ctx, _ctx() as work:
        ctx.set_data(X, Y)
        fit = PPLS(None, None, TA, TSTEPS, TATOL, "o2m_xprod", ctx=ctx)
        out = permutation_PPLS(fit, None, None, EMsteps=TSTEPS, atol=TATOL, ctx=ctx, work=work, perms=perms, keep=True)
        assert work.h is not None and work.streamed                      # the caller's work context stays open
        obs, null, pv, failed = _written_out(ctx, fit, perms)
        with pytest.raises(ValueError, match="none of the"):
            permutation_PPLS(fit, None, None, EMsteps=TSTEPS, atol=TATOL, ctx=ctx, perms=perms[[2, 2]])
        with pytest.raises(ValueError, match="perms"):
            permutation_PPLS(fit, None, None, ctx=ctx, perms=perms[:, :-1])
    assert out["failed"] == [2] == failed and out["nperm"] == NPERM and out["steps"][2] == 0
    assert out["replicates"][2] is None and len(out["replicates"]) == NPERM
    for key in ("B", "cov", "loglik"):
        assert np.isnan(out["null"][key][2]).all() and not np.isnan(np.delete(out["null"][key], 2, axis=0)).any()
        assert np.array_equal(out["pvalue"][key], pv[key])
        assert np.array_equal(out["pvalue"][key], permutation_pvalues(out["observed"][key], np.delete(out["null"][key], 2, axis=0)))
    assert out["pvalue"]["loglik"][0] == 1 / 19
