"""Cross-validation on the device: predict.PPLS, cv_PPLS, crossval_PPLS (crossval_PPLS.R:12-114).

The reference for the CV loop is its numpy restatement below (``cv_restated``): R's fold
construction, ``oracle.ppls_oracle.ppls`` on ``X[-fold, ]`` for the fits and plain numpy for
``sqrt(mse(Y[fold, ], predict(fit, X[fold, ], "X")))`` with OmicsPLS's mse(x, y) = mean((x - y)^2).
It is computed once per case and shared by the tests that need it.

Tolerances are the project's (tests/test_gpu_parity.py, tests/test_gpu_init.py): loadings 1e-8
absolute, B / sigmas / RMSEP 1e-8 relative, sharded = unsharded to 1e-12.  The prediction and the
held-out residual are compared at 1e-12 of the largest entry: a dot product of p terms in fp64
carries at most ~p u sum|x_j w_j|, about 2100 x 1.1e-16 x 40 = 1e-11 of a unit entry in the worst
case at the widest shape here and a few e-14 in practice (random signs), against references formed
in extended precision.
"""
import functools
import threading

import numpy as np
import pytest

from conftest import make_problem
from oracle import ppls_oracle as o

pytestmark = pytest.mark.gpu

E_ARG = -1


def _centred(n, p, q, r, seed=5):
    X, Y, _ = make_problem(n, p, q, r, seed=seed)
    return X - X.mean(0), Y - Y.mean(0)


def _blocks(N, K):
    """cut(seq(1:N), breaks=K, labels=F) restated on its own: right-closed equal-width intervals
    over [1, N] whose outer ends are moved out by (N - 1) / 1000."""
    dx = N - 1.0
    br = [1.0 + i * dx / K for i in range(K + 1)]
    br[0], br[K] = 1.0 - dx / 1000, N + dx / 1000
    return np.array([next(i for i in range(1, K + 1) if br[i - 1] < x <= br[i]) for x in range(1, N + 1)])


@functools.lru_cache(maxsize=None)
def cv_restated(n, p, q, a, K, steps, atol, perm_seed=3):
    """cv_PPLS (crossval_PPLS.R:40-52) in numpy for 'equal' starts: (X, Y, perm, fold label of every
    row, RMSEP K x a of every prefix of the components, Number_steps per fold)."""
    X, Y = _centred(n, p, q, a)
    perm = np.random.default_rng(perm_seed).permutation(n)
    blocks = _blocks(n, K)
    fold_of = np.empty(n, dtype=np.int32)
    fold_of[perm] = blocks - 1
    err = np.full((K, a), np.nan)
    nsteps = []
    for i in range(K):
        out = perm[blocks == i + 1]
        keep = np.ones(n, dtype=bool)
        keep[out] = False
        fit = o.ppls(X[keep], Y[keep], a, steps, atol, [o.initial_guess(p, q, "equal") for _ in range(a)])
        nsteps.append(list(fit["Other_output"]["Number_steps"]))
        for j in range(1, fit["W"].shape[1] + 1):
            pred = X[out] @ fit["W"][:, :j] @ np.diag(fit["B"][:j]) @ fit["C"][:, :j].T
            err[i, j - 1] = np.sqrt(np.mean((Y[out] - pred) ** 2))
    for arr in (X, Y, perm, fold_of, err):
        arr.setflags(write=False)
    return X, Y, perm, fold_of, err, nsteps


def _ctx(dtype=0, xprod=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", xprod)
    return c


def _fit_parts(p, q, k, seed):
    rng = np.random.default_rng(seed)
    W = np.linalg.qr(rng.standard_normal((p, k)))[0]
    C = np.linalg.qr(rng.standard_normal((q, k)))[0]
    B = rng.uniform(0.5, 1.5, size=k) * rng.choice([-1.0, 1.0], size=k)
    return W, C, B


def _relmax(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / np.abs(b).max()


# ------------------------------------------------------------------------------ 1. predict
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n,p,q", [(67, 37, 19), (1, 37, 19), (40, 2100, 5)])
def test_predict_both_directions(n, p, q, k, dtype):
    rng = np.random.default_rng(n + p + k)
    W, C, B = _fit_parts(p, q, k, seed=p + k)
    L = np.longdouble
    with _ctx(dtype) as c:
        c.set_data(rng.standard_normal((5, p)), rng.standard_normal((5, q)))   # the shape; newdata is independent
        for xory, cols in ((0, p), (1, q)):
            nd = rng.standard_normal((n, cols))
            ref = (nd.astype(L) @ W.astype(L) * B.astype(L) @ C.T.astype(L) if xory == 0
                   else nd.astype(L) @ C.astype(L) / B.astype(L) @ W.T.astype(L))
            for arr in (nd, np.asfortranarray(nd)):     # both layouts
                got = c.predict(W, C, B, arr, xory)
                assert got.shape == ref.shape
                err = _relmax(got, ref.astype(np.float64))
                print(f"predict n={n} p={p} q={q} k={k} dtype={dtype} xory={xory}: rel err {err:.3g}")
                assert err < 1e-12


def test_predict_PPLS_public():
    from ppls_amd import predict_PPLS
    p, q, k = 37, 19, 3
    W, C, B = _fit_parts(p, q, k, seed=9)
    fit = dict(W=W, C=C, B=B)
    rng = np.random.default_rng(0)
    x = rng.standard_normal(p)
    got = predict_PPLS(fit, x)                    # a vector is one row; XorY defaults to "X"
    assert got.shape == (1, q)
    assert _relmax(got, (x @ W * B @ C.T)[None, :]) < 1e-12
    Ynew = rng.standard_normal((6, q))
    assert _relmax(predict_PPLS(fit, Ynew, "Y"), Ynew @ C / B @ W.T) < 1e-12
    with pytest.raises(ValueError, match="Number of columns mismatch!"):
        predict_PPLS(fit, Ynew, "X")


# ------------------------------------------------------------------------------ 2. set_data_from
ROW_LISTS = {"four": [0, 2, 3, 66], "all": list(range(67)), "empty": []}


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("rows", list(ROW_LISTS), ids=list(ROW_LISTS))
def test_set_data_from_equals_set_data(rows, dtype):
    rows = ROW_LISTS[rows]
    X, Y = _centred(67, 37, 19, 2)
    with _ctx(dtype) as src, _ctx(0) as dst, _ctx(dtype) as fresh:
        src.set_data(X, Y)
        dst.set_data_from(src, rows)               # takes src's storage dtype
        fresh.set_data(X[rows], Y[rows])
        assert (dst.n_local, dst.n_total, dst.p, dst.q) == (len(rows), len(rows), 37, 19)
        assert dst.ssq() == fresh.ssq()
        if rows:
            gx, gy = dst.get_data()
            fx, fy = fresh.get_data()
            assert np.array_equal(gx, fx) and np.array_equal(gy, fy)
            if dtype == 0:
                assert np.array_equal(gx, X[rows]) and np.array_equal(gy, Y[rows])
            rx, ry = dst.get_data_rows()
            assert np.array_equal(rx, fx) and np.array_equal(ry, fy)


@pytest.mark.parametrize("xprod", [0, 1])
@pytest.mark.parametrize("rows,a", [("four", 1), ("all", 2)])
def test_set_data_from_fit_equals_fresh_fit(rows, a, xprod):
    from ppls_amd.api import initial_guess
    rows = ROW_LISTS[rows]
    X, Y = _centred(67, 37, 19, 2)
    inits = [initial_guess(37, 19, "equal") for _ in range(a)]
    with _ctx(0, xprod) as src, _ctx(0, xprod) as dst, _ctx(0, xprod) as fresh:
        src.set_data(X, Y)
        dst.set_data_from(src, rows)
        fresh.set_data(X[rows], Y[rows])
        f, g = dst.ppls(a, 10, -1.0, inits), fresh.ppls(a, 10, -1.0, inits)
    assert f["ncomp"] == g["ncomp"] == a
    assert np.abs(f["W"] - g["W"]).max() < 1e-8 and np.abs(f["C"] - g["C"]).max() < 1e-8
    assert _relmax(f["B"], g["B"]) < 1e-8 and _relmax(f["sig"], g["sig"]) < 1e-8
    assert _relmax(f["Other_output"]["Loglikelihoods"], g["Other_output"]["Loglikelihoods"]) < 1e-10
    assert list(f["Other_output"]["Number_steps"]) == list(g["Other_output"]["Number_steps"])


def test_set_data_from_bad_arguments():
    from ppls_amd import PplsError
    X, Y = _centred(67, 37, 19, 2)
    with _ctx() as src, _ctx() as dst, _ctx() as nodata:
        src.set_data(X, Y)
        for bad in ([0, 67], [-1, 3], [5, 4], [3, 3]):
            with pytest.raises(PplsError) as e:
                dst.set_data_from(src, bad)
            assert e.value.code == E_ARG, bad
        with pytest.raises(PplsError) as e:
            src.set_data_from(src, [0, 1])
        assert e.value.code == E_ARG
        with pytest.raises(PplsError) as e:
            dst.set_data_from(nodata, [])
        assert e.value.code == E_ARG
        gx, gy = src.get_data()                      # the refused calls left the source as it was
        assert np.array_equal(gx, X) and np.array_equal(gy, Y)


# ------------------------------------------------------------------------------ 3. xprod_downdate
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_xprod_downdate_against_direct_S(dtype):
    from ppls_amd import Theta
    n, p, q, r = 203, 37, 19, 3
    X, Y, th0 = make_problem(n, p, q, r, seed=5)
    out = np.sort(np.random.default_rng(3).permutation(n)[:51])
    keep = np.setdiff1d(np.arange(n), out)
    th = Theta(th0["W"], th0["C"], th0["B"], th0["sigE"], th0["sigF"], th0["sigH"], th0["sigT"])
    with _ctx(dtype) as src, _ctx(dtype) as dst, _ctx(dtype) as direct:
        src.set_data(X, Y)
        dst.set_data_from(src, keep)
        assert not dst.xprod_info()["ready"]
        dst.xprod_downdate(src, out)
        assert dst.xprod_info()["ready"] and src.xprod_info()["ready"]
        got = dst.xprod_stats(th)
        direct.set_data(X[keep], Y[keep])
        direct.xprod_prepare()
        ref = direct.xprod_stats(th)
    for g, r_, name in zip(got, ref, ("X'mu_T", "Y'mu_U", "Gram")):
        err = _relmax(g, r_)
        print(f"downdate dtype={dtype} {name}: rel err {err:.3g}")
        assert err < 1e-10


def test_xprod_downdate_refuses_mismatching_counts():
    from ppls_amd import PplsError
    X, Y = _centred(67, 37, 19, 2)
    rows = np.arange(67)
    with _ctx() as src, _ctx() as dst:
        src.set_data(X, Y)
        dst.set_data_from(src, rows[:50])
        with pytest.raises(PplsError) as e:          # 67 - 16 != 50
            dst.xprod_downdate(src, rows[51:])
        assert e.value.code == E_ARG
        assert not dst.xprod_info()["ready"]
        dst.xprod_downdate(src, rows[50:])           # the right count is accepted
        assert dst.xprod_info()["ready"]
        dst.set_data_from(src, rows[:30])            # more held out (37) than kept (30): form S directly
        with pytest.raises(PplsError) as e:
            dst.xprod_downdate(src, rows[30:])
        assert e.value.code == E_ARG
        with pytest.raises(PplsError) as e:
            src.xprod_downdate(src, rows[:1])
        assert e.value.code == E_ARG


# ------------------------------------------------------------------------------ 4. heldout_sse
def _sse_numpy(X, Y, W, C, B, rows):
    L = np.longdouble
    T = X[rows].astype(L) @ W.astype(L) * B.astype(L)
    return np.array([float(((Y[rows].astype(L) - T[:, :j] @ C[:, :j].T.astype(L)) ** 2).sum())
                     for j in range(1, W.shape[1] + 1)])


@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n,p,q,rows", [(67, 37, 19, "some"), (67, 37, 19, "one"), (67, 37, 19, "all"),
                                        (40, 2100, 5, "some")])
def test_heldout_sse_prefixes(n, p, q, rows, dtype):
    X, Y, _ = make_problem(n, p, q, 3, seed=5)
    W, C, B = _fit_parts(p, q, 3, seed=n)
    rows = {"some": np.sort(np.random.default_rng(1).permutation(n)[:n // 3]), "one": np.array([n - 1]),
            "all": np.arange(n)}[rows]
    if dtype:      # the stored values are the fp32 roundings
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    with _ctx(dtype) as c:
        c.set_data(X, Y)
        got = c.heldout_sse(W, C, B, rows)
        again = c.heldout_sse(W, C, B, rows)
        none = c.heldout_sse(W, C, B, [])
    ref = _sse_numpy(X, Y, W, C, B, rows)
    err = np.abs(got - ref) / ref
    print(f"heldout n={n} p={p} rows={len(rows)} dtype={dtype}: rel err {err.max():.3g}")
    assert got.shape == (3,) and np.all(err < 1e-12)
    assert np.array_equal(got, again)                # fixed-order sums: bitwise repeatable
    assert np.array_equal(none, np.zeros(3))


# ------------------------------------------------------------------------------ 5. cv_PPLS
CV_CASES = [(203, 37, 19, 3, 4), (130, 70, 5, 2, 3), (23, 9, 7, 2, 23)]


@pytest.mark.parametrize("xprod", [0, 1])
@pytest.mark.parametrize("n,p,q,a,K", CV_CASES, ids=["n203_K4", "n130_K3", "loo_n23"])
def test_cv_PPLS_per_fold_errors(n, p, q, a, K, xprod):
    from ppls_amd import cv_PPLS
    from ppls_amd.api import initial_guess
    X, Y, perm, fold_of, ref, _ = cv_restated(n, p, q, a, K, 30, -1.0)
    assert np.all(np.isfinite(ref))
    with _ctx(0, xprod) as c:
        mean, err = cv_PPLS(X, Y, a, K, folds=perm, ctx=c, per_fold=True, EMsteps=30, atol=-1.0)
        inits = [[initial_guess(p, q, "equal") for _ in range(a)]] * K
        rmsep, ncomp = c.cv_ppls(a, fold_of, np.bincount(fold_of, minlength=K), 30, -1.0, inits)
    rel = np.abs(rmsep - ref) / ref
    print(f"cv n={n} K={K} xprod={xprod}: RMSEP {ref.min():.3f}..{ref.max():.3f}, rel err {rel.max():.3g}")
    assert list(ncomp) == [a] * K
    assert np.all(rel < 1e-8)
    assert np.array_equal(err, rmsep[:, a - 1]) and mean == float(np.mean(err))


def test_cv_PPLS_with_the_stop_rule():
    """atol = 1e-4, EMsteps = 100: the RMSEPs, and a fit of every fold's training rows (gathered on
    the device) stops where the oracle's does."""
    from ppls_amd import cv_PPLS
    from ppls_amd.api import initial_guess
    n, p, q, a, K = 203, 37, 19, 3, 4
    X, Y, perm, fold_of, ref, nsteps = cv_restated(n, p, q, a, K, 100, 1e-4)
    inits = [initial_guess(p, q, "equal") for _ in range(a)]
    with _ctx() as c, _ctx() as t:
        _, err = cv_PPLS(X, Y, a, K, folds=perm, ctx=c, per_fold=True, EMsteps=100, atol=1e-4)
        got_steps = []
        for f in range(K):
            t.set_data_from(c, np.flatnonzero(fold_of != f))
            got_steps.append(list(t.ppls(a, 100, 1e-4, inits)["Other_output"]["Number_steps"]))
    rel = np.abs(err - ref[:, a - 1]) / ref[:, a - 1]
    print(f"cv stop rule: steps {nsteps}, device {got_steps}, rel err {rel.max():.3g}")
    assert got_steps == nsteps
    assert any(s < 100 for fold in nsteps for s in fold)      # the stop rule is exercised
    assert np.all(rel < 1e-8)


# ------------------------------------------------------------------------------ 6. crossval_PPLS
class SpyRng:
    """A numpy Generator that records the permutations drawn from it."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.perms = []

    def permutation(self, n):
        self.perms.append(self.rng.permutation(n))
        return self.perms[-1]


def test_crossval_PPLS_shared_folds_and_default_mode():
    from ppls_amd import crossval_PPLS, cv_PPLS
    n, p, q, K = 130, 70, 5, 3
    X, Y = _centred(n, p, q, 2)
    perm = np.random.default_rng(3).permutation(n)
    args = dict(EMsteps=30, atol=-1.0)
    with _ctx() as c:
        cv = crossval_PPLS(X, Y, [1, 2, 3], K, shared_folds=True, ctx=c, folds=perm, **args)
        single = [cv_PPLS(None, None, e, K, folds=perm, ctx=c, **args) for e in (1, 2, 3)]
        spy = SpyRng(11)
        dflt = crossval_PPLS(X, Y, [1, 2, 3], K, nr_cores=2, ctx=c, rng=spy, **args)
        spy1 = SpyRng(11)
        shared = crossval_PPLS(None, None, [1, 2, 3], K, shared_folds=True, ctx=c, rng=spy1, **args)
    assert cv["class"] == "cvPPLS" and cv["errors"].shape == (3,) and cv["time"] >= 0
    assert _relmax(cv["errors"], np.array(single)) < 1e-12
    assert cv["which_error"] == int(np.argmin(cv["errors"])) and cv["a_min"] == [1, 2, 3][cv["which_error"]]
    # default mode: one fresh permutation per entry of a (as R's cv_PPLS draws sample(N) per call)
    assert len(spy.perms) == 3 and len(spy1.perms) == 1
    assert not np.array_equal(spy.perms[0], spy.perms[1]) and not np.array_equal(spy.perms[1], spy.perms[2])
    assert np.array_equal(spy.perms[0], spy1.perms[0])
    assert abs(dflt["errors"][0] - shared["errors"][0]) < 1e-12 * shared["errors"][0]   # the same folds for the first entry
    assert dflt["which_error"] == int(np.argmin(dflt["errors"]))


# ------------------------------------------------------------------------------ 7. shards
class ThreadAllReduce:
    """Sum over k host threads in rank order (tests/test_gpu_multirank.py's pattern): every rank gets
    the bitwise-same result; a bounded barrier, so a rank that misses a collective fails the test
    instead of hanging it."""

    def __init__(self, k):
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


@pytest.mark.parametrize("xprod", [0, 1])
def test_cv_sharded_equals_unsharded(xprod):
    from ppls_amd.api import initial_guess
    n, p, q, a, K = 60, 12, 7, 2, 4
    X, Y = _centred(n, p, q, a)
    # contiguous folds (the identity permutation): rank 0 (rows 0..34) holds no row of fold 3, rank 2
    # (rows 35..59) none of folds 0 and 1, and rank 1 holds no row at all
    fold_of = (_blocks(n, K) - 1).astype(np.int32)
    fold_total = np.bincount(fold_of, minlength=K)
    bounds = [0, 35, 35, 60]
    inits = [[initial_guess(p, q, "equal") for _ in range(a)]] * K
    with _ctx(0, xprod) as c:
        c.set_data(X, Y)
        ref, ref_nc = c.cv_ppls(a, fold_of, fold_total, 30, -1.0, inits)
    assert set(fold_of[:35]) == {0, 1, 2} and set(fold_of[35:]) == {2, 3}

    red = ThreadAllReduce(3)
    out, errs = [None] * 3, []

    def body(rank):
        try:
            lo, hi = bounds[rank], bounds[rank + 1]
            with _ctx(0, xprod) as c:
                c.set_reducer(red.fn(rank))
                c.set_data(X[lo:hi], Y[lo:hi], n_total=n)
                out[rank] = c.cv_ppls(a, fold_of[lo:hi], fold_total, 30, -1.0, inits)
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
    assert red.calls > 0
    for rmsep, nc in out:
        assert np.array_equal(rmsep, out[0][0]) and np.array_equal(nc, ref_nc)
    rel = np.abs(out[0][0] - ref) / ref
    print(f"sharded cv xprod={xprod}: rel diff {rel.max():.3g}")
    assert np.all(rel < 1e-12)
