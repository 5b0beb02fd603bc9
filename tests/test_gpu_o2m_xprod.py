"""initialGuess = "o2m_xprod" (DESIGN §21): PPLSi's 'o2m' starting values (EM_W_multi.R:126-131,
meta_PPLSi :520-525) from the cross-products S on the device, wherever S is all there is.

* the pass alone (ppls_o2m_pass) against long double within the a-priori bar of tests/o2m_bar.py, both
  paths, bit for bit on a second launch;
* the Lanczos pair on blocks built from a known SVD; the sign rule;
* starts and fits against the oracle on the explicit data, with the tolerances of tests/test_gpu_o2m.py
  (loadings 1e-8 after joint sign alignment, B and sigmas 1e-8 relative, log-likelihoods 1e-10
  relative, step counts exact): resident (xprod 0 and 1), streamed, a fold selection, a resample
  destination, meta_PPLSi, a fixed non-unit W, three row shards;
* cross-validation against the loop written out with the oracle (tests/test_gpu_cv.py's 1e-8);
* refusals and state."""
import functools

import numpy as np
import pytest

import o2m_bar as ob
from conftest import make_problem
from oracle import ppls_oracle as o

pytestmark = pytest.mark.gpu

E_ARG, E_NUMERIC, E_STATE = -1, -3, -4


def _ctx(xprod=0, path=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("xprod", xprod)
    c.set_option("o2m_path", path)
    return c


def _relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _aligned(W, C, Wr):
    W, C = np.array(W, dtype=float, ndmin=2).reshape(len(W), -1), np.array(C, dtype=float).reshape(len(C), -1)
    s = np.sign(np.sum(W * np.asarray(Wr).reshape(W.shape), axis=0))
    return W * s, C * s


def _code(fn):
    from ppls_amd._lib import PplsError
    with pytest.raises(PplsError) as e:
        fn()
    return e.value.code


def _same_fit(f, ref, a):
    W, C = _aligned(f["W"], f["C"], ref["W"])
    assert W.shape == np.asarray(ref["W"]).reshape(W.shape[0], -1).shape
    assert np.abs(W - np.asarray(ref["W"]).reshape(W.shape)).max() < 1e-8
    assert np.abs(C - np.asarray(ref["C"]).reshape(C.shape)).max() < 1e-8
    assert _relerr(f["B"], ref["B"]) < 1e-8 and _relerr(f["sig"], ref["sig"]) < 1e-8
    oo = f["Other_output"]
    assert list(oo["Number_steps"]) == list(ref["Other_output"]["Number_steps"])
    assert _relerr(oo["Loglikelihoods"], ref["Other_output"]["Loglikelihoods"]) < 1e-10


@functools.lru_cache(maxsize=None)
def _oracle_fit(n, p, q, a, seed):
    X, Y, _ = make_problem(n, p, q, a, seed=seed)
    ref = o.ppls(X, Y, a, 40, 1e-6, ["o2m"] * a)
    for arr in (X, Y):
        arr.setflags(write=False)
    return X, Y, ref


# ------------------------------------------------------------------------------ 1. the pass alone
PASS_SHAPES = [
    dict(rows=30, L=20, col0=30, ld=52),             # a block at an offset
    dict(rows=25, L=18, row0=18, ld=44),             # the other side
    dict(rows=31, L=21, col0=32, ld=54),             # p = 31, q = 21: ldx = 32, ldy = 22, padding columns
    dict(rows=40, L=1), dict(rows=40, L=2), dict(rows=40, L=127, ld=130), dict(rows=40, L=128),
    dict(rows=40, L=129, ld=132),
    dict(rows=1, L=33), dict(rows=3, L=33), dict(rows=257, L=33, col0=2, ld=40),
    dict(rows=70, L=300, ld=310),                    # four column pairs per lane
    dict(rows=70, L=600, ld=610),                    # past 512: a workgroup's waves share the row, 2 chunks each
    dict(rows=37, L=1100, col0=2, ld=1110),          # ... 4 chunks each, the last step short of rows
]


@pytest.mark.parametrize("path", [1, 2], ids=["fused", "twophase"])
@pytest.mark.parametrize("shape", PASS_SHAPES, ids=lambda s: "x".join(f"{k}{v}" for k, v in s.items()))
def test_pass_against_long_double(shape, path):
    with _ctx(path=path) as c:
        for d_zero in (False, True):
            case = ob.make_case(d_zero=d_zero, **shape)
            ref_u, ref_z = ob.reference(case)
            bar_u, bar_z = ob.bars(case)
            args = (case["S"], case["row0"], case["col0"], case["rows"], case["L"], case["v"])
            u, z, took = c.o2m_pass(*args, None if d_zero else case["d"])
            ru, rz = ob.inside(u, ref_u, bar_u), ob.inside(z, ref_z, bar_z)
            print(f"{shape} path {took} d0={d_zero}: u err / bar {ru:.3g}, z err / bar {rz:.3g}")
            assert took == path
            assert ru <= 1.0 and rz <= 1.0
            u2, z2, _ = c.o2m_pass(*args, None if d_zero else case["d"])
            assert np.array_equal(u, u2) and np.array_equal(z, z2)


def test_pass_budget_and_arguments():
    case = ob.make_case(5, ob.FUSED_LMAX + 1)           # just past the fused budget
    ref_u, ref_z = ob.reference(case)
    bar_u, bar_z = ob.bars(case)
    args = (case["S"], 0, 0, case["rows"], case["L"], case["v"], case["d"])
    with _ctx(path=0) as c:
        u, z, took = c.o2m_pass(*args)
        assert took == ob.PATH_TWOPHASE
        assert ob.inside(u, ref_u, bar_u) <= 1.0 and ob.inside(z, ref_z, bar_z) <= 1.0
        c.set_option("o2m_path", 1)
        assert _code(lambda: c.o2m_pass(*args)) == E_ARG   # the fused path forced past its budget
        c.set_option("o2m_path", 0)
        at = ob.make_case(4, ob.FUSED_LMAX)               # the budget itself: 16 column pairs per lane
        u, z, took = c.o2m_pass(at["S"], 0, 0, 4, ob.FUSED_LMAX, at["v"], at["d"])
        assert took == ob.PATH_FUSED
        bu, bz = ob.bars(at)
        ru, rz = ob.reference(at)
        assert ob.inside(u, ru, bu) <= 1.0 and ob.inside(z, rz, bz) <= 1.0
        S = np.zeros((6, 8))
        assert _code(lambda: c.o2m_pass(S, 0, 1, 4, 4, np.ones(4))) == E_ARG    # an odd column start
        assert _code(lambda: c.o2m_pass(S, 4, 0, 4, 4, np.ones(4))) == E_ARG    # rows past the matrix
        assert _code(lambda: c.o2m_pass(S, 0, 6, 4, 3, np.ones(3))) == E_ARG    # columns past the row
        with pytest.raises(Exception):
            c.set_option("o2m_path", 3)


# ------------------------------------------------------------------------------ 2. the solver
def _svd_block(rows, L, ratio, seed):
    """A (rows x L) = U diag(s) V' with s = (1, ratio, 0.3 * 0.8^j ...): X = I, Y = A give X'Y = A exactly."""
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((rows, L)))[0]
    V = np.linalg.qr(rng.standard_normal((L, L)))[0]
    s = np.r_[1.0, ratio, 0.3 * 0.8 ** np.arange(L - 2)]
    return (U * s) @ V.T, s, V


@pytest.mark.parametrize("ratio", [0.5, 0.99, 0.9999, 1.0])
@pytest.mark.parametrize("rows,L", [(96, 64), (700, 333)])
def test_solver_on_a_known_svd(rows, L, ratio):
    A, s, V = _svd_block(rows, L, ratio, seed=rows + L)
    with _ctx() as c:
        c.set_data(np.eye(rows), A)
        g = c.o2m_start()
        info = c.o2m_info()
    theta = float(np.linalg.svd(A, compute_uv=False)[0] ** 2)
    y = g["C"]
    resid = float(np.linalg.norm(A.T @ (A @ y) - info["theta"] * y) / info["theta"])
    print(f"{rows}x{L} ratio {ratio}: passes {info['passes']}, theta rel err {abs(info['theta'] - theta) / theta:.3g}, "
          f"residual / theta {resid:.3g}, estimate / theta {info['resid'] / info['theta']:.3g}")
    assert info["side"] == 0 and info["path"] == ob.PATH_FUSED
    assert abs(info["theta"] - theta) <= 1e-12 * theta
    assert resid <= 4 * 2.0 ** -43
    assert info["passes"] <= 32
    if ratio <= 0.99:   # an open gap: the vector itself
        assert min(np.abs(y - V[:, 0]).max(), np.abs(y + V[:, 0]).max()) < 1e-8
    assert abs(np.linalg.norm(g["W"]) - 1) < 1e-12 and abs(np.linalg.norm(y) - 1) < 1e-12


# ------------------------------------------------------------------------------ 3. the sign rule
def test_sign_rule():
    X, Y, _ = make_problem(300, 14, 19, 2, seed=4)
    with _ctx() as c:
        c.set_data(X, Y)
        g0 = c.o2m_start()
        Wp, Cp = g0["W"].reshape(-1, 1), g0["C"].reshape(-1, 1)
        g1 = c.o2m_start(Wp, Cp)
        c.set_data(-X, Y)
        m0 = c.o2m_start()
    for g in (g0, g1, m0):
        assert g["W"][np.argmax(np.abs(g["W"]))] > 0
    assert np.abs(m0["W"] - g0["W"]).max() < 1e-10 and np.abs(m0["C"] + g0["C"]).max() < 1e-10
    assert abs(m0["B"] - g0["B"]) < 1e-10 * abs(g0["B"])    # Tt'U / Tt'Tt of the pair: the joint sign cancels


# ------------------------------------------------------------------------------ 4. starts and fits
@pytest.mark.parametrize("xprod", [0, 1], ids=["stream", "xprod"])
@pytest.mark.parametrize("n,p,q,a", [(500, 30, 20, 3), (2000, 120, 45, 2), (600, 18, 25, 3)])
def test_ppls_o2m_xprod_matches_oracle(n, p, q, a, xprod):
    from ppls_amd import PPLS
    X, Y, ref = _oracle_fit(n, p, q, a, n + p)
    with _ctx(xprod) as c:
        f = PPLS(X, Y, a, 40, 1e-6, "o2m_xprod", ctx=c)
        info = c.o2m_info()
        _same_fit(f, ref, a)
        assert np.allclose(f["W"].T @ f["W"], np.eye(a), atol=1e-10)
        assert info["fits"] == a and info["passes"] <= 32 and info["side"] == (0 if q <= p else 1)
        assert c.xprod_info()["ready"]        # S stays, as after xprod_prepare
        c.xprod_release()
        assert not c.xprod_info()["ready"]


def test_start_matches_oracle_on_deflated_data():
    n, p, q = 600, 25, 18
    for k in (0, 1, 2, 3):
        X, Y, _ = make_problem(n, p, q, 3, seed=11 + k)
        rng = np.random.default_rng(k)
        Wp = rng.standard_normal((p, k))
        Cp = rng.standard_normal((q, k))
        Wp /= np.linalg.norm(Wp, axis=0) if k else 1.0
        Cp /= np.linalg.norm(Cp, axis=0) if k else 1.0
        Xc, Yc = X.copy(), Y.copy()
        for j in range(k):
            Xc = Xc - np.outer(Xc @ Wp[:, j], Wp[:, j])
            Yc = Yc - np.outer(Yc @ Cp[:, j], Cp[:, j])
        ref = o.initial_guess_o2m(Xc, Yc)
        for path in (1, 2):
            with _ctx(path=path) as c:
                c.set_data(X, Y)
                g = c.o2m_start(Wp, Cp)
                assert c.o2m_info()["path"] == path
            W, C = _aligned(g["W"], g["C"], ref["W"])
            assert np.abs(W.ravel() - ref["W"]).max() < 1e-8 and np.abs(C.ravel() - ref["C"]).max() < 1e-8
            for key in ("B", "sigE", "sigF", "sigH", "sigT"):
                assert abs(g[key] - ref[key]) <= 1e-8 * abs(ref[key]), (k, key)


def _scale(A):
    return (A - A.mean(axis=0)) / A.std(axis=0, ddof=1)


def test_streamed_context():
    from ppls_amd import PPLS
    n, p, q, a = 500, 30, 20, 3
    X, Y, _ = make_problem(n, p, q, a, seed=21)
    X, Y = X + 0.3, Y * 2.0 - 0.1
    ref = o.ppls(_scale(X), _scale(Y), a, 40, 1e-6, ["o2m"] * a)
    with _ctx() as c:
        c.stream_begin(p, q, True, True)
        assert _code(lambda: c.o2m_start()) == E_STATE          # an open stream
        assert _code(lambda: c.ppls_o2m(1, 5, 1e-4)) == E_STATE
        for lo, hi in ((0, 170), (170, 333), (333, n)):
            c.stream_rows(X[lo:hi], Y[lo:hi])
        c.stream_end()
        f = PPLS(None, None, a, 40, 1e-6, "o2m_xprod", ctx=c)
        _same_fit(f, ref, a)
        assert c.o2m_info()["fits"] == a
        with pytest.raises(NotImplementedError, match="streamed"):   # the other spelling keeps its refusal
            PPLS(None, None, a, 40, 1e-6, "o2m", ctx=c)


def test_fold_selection_and_meta_on_a_fold_stream():
    import ppls_amd
    from ppls_amd import PPLS
    n, p, q, K, a = 300, 26, 14, 3, 2
    X, Y, _ = make_problem(n, p, q, a, seed=12)
    labels = np.random.default_rng(5).integers(0, K, n).astype(np.int32)
    with _ctx() as c:
        c.stream_begin(p, q, False, False, nr_folds=K)
        for lo, hi in ((0, 100), (100, 210), (210, n)):
            c.stream_rows(X[lo:hi], Y[lo:hi], labels[lo:hi])
        c.stream_end()
        c.stream_select(1)
        keep = labels != 1
        f = PPLS(None, None, a, 40, 1e-6, "o2m_xprod", ctx=c)
        _same_fit(f, o.ppls(X[keep], Y[keep], a, 40, 1e-6, ["o2m"] * a), a)
        # meta_PPLSi on the stream's populations: the start is o2m of all rows (selection -1)
        m = ppls_amd.meta_PPLSi(None, None, None, EMsteps=20, atol=-np.inf, initialGuess="o2m_xprod", ctx=c)
        assert c.stream_fold_info()["selected"] == -1
    order = np.argsort(labels, kind="stable")
    ref = o.meta_pplsi(X[order], Y[order], list(np.bincount(labels, minlength=K)), 20, -np.inf, o.initial_guess_o2m(X, Y))
    W, C = _aligned(m["W"], m["C"], ref["W"])
    assert np.abs(W.ravel() - np.ravel(ref["W"])).max() < 1e-8 and np.abs(C.ravel() - np.ravel(ref["C"])).max() < 1e-8
    assert _relerr(m["logvalue"], ref["logvalue"]) < 1e-10


def test_resample_destination():
    from ppls_amd import PPLS
    n, p, q, a = 400, 18, 25, 2
    X, Y, _ = make_problem(n, p, q, a, seed=31)
    count = np.random.default_rng(2).multinomial(n, np.full(n, 1.0 / n)).astype(np.int32)
    with _ctx() as src, _ctx() as dst:
        src.set_data(X, Y)
        dst.xprod_resample(src, count)
        f = PPLS(None, None, a, 40, 1e-6, "o2m_xprod", ctx=dst)
    Xr, Yr = np.repeat(X, count, axis=0), np.repeat(Y, count, axis=0)
    _same_fit(f, o.ppls(Xr, Yr, a, 40, 1e-6, ["o2m"] * a), a)


def test_pplsi_starts_at_the_oracle_values():
    from ppls_amd import PPLSi
    X, Y, _ = make_problem(800, 50, 35, 1, seed=9)
    with _ctx() as c:
        one = PPLSi(X, Y, 25, 1e-8, "o2m_xprod", ctx=c)
    r1 = o.pplsi(X, Y, 25, 1e-8, o.initial_guess_o2m(X, Y))
    assert _relerr(one["logvalue"], r1["logvalue"]) < 1e-10
    W, _ = _aligned(one["W"], one["C"], r1["W"])
    assert np.abs(W.ravel() - r1["W"]).max() < 1e-8 and one["Number_steps"] == r1["Number_steps"]


def test_meta_pplsi_resident():
    import ppls_amd
    X, Y, _ = make_problem(300, 26, 14, 1, seed=12)
    Ipopu = np.repeat([0, 1, 2], [80, 120, 100])
    with _ctx() as c:
        m = ppls_amd.meta_PPLSi(X, Y, Ipopu, EMsteps=20, atol=-np.inf, initialGuess="o2m_xprod", ctx=c)
    ref = o.meta_pplsi(X, Y, [80, 120, 100], 20, -np.inf, o.initial_guess_o2m(X, Y))
    W, C = _aligned(m["W"], m["C"], ref["W"])
    assert np.abs(W.ravel() - np.ravel(ref["W"])).max() < 1e-8 and np.abs(C.ravel() - np.ravel(ref["C"])).max() < 1e-8
    assert _relerr(m["logvalue"], ref["logvalue"]) < 1e-10


def test_fixed_non_unit_w_on_the_first_component():
    """Component 1's W is fixed to a vector of norm 1.3, so the deflation behind component 2's start
    is not an orthogonal projection: the compact T of the pass sees it."""
    from ppls_amd import PPLS, fconstraint
    n, p, q, a = 500, 30, 20, 2
    X, Y, _ = make_problem(n, p, q, a, seed=41)
    w1 = np.random.default_rng(1).standard_normal(p)
    w1 *= 1.3 / np.linalg.norm(w1)
    cons = [fconstraint(dict(W=w1)), fconstraint()]
    ref = o.ppls(X, Y, a, 40, 1e-6, ["o2m"] * a, constraints=[o.fconstraint(dict(W=w1)), o.fconstraint()])
    with _ctx() as c:
        f = PPLS(X, Y, a, 40, 1e-6, "o2m_xprod", constraints=cons, ctx=c)
    assert np.array_equal(f["W"][:, 0], w1)
    _same_fit(f, ref, a)


def test_three_shards_equal_the_unsharded_fit_bitwise():
    from test_gpu_multirank import _run_ranks
    from ppls_amd import Context
    n, p, q, a, k = 500, 30, 20, 3, 3
    X, Y, _ = make_problem(n, p, q, a, seed=n + p)
    # integer-valued data: every product and sum behind S and the sums of squares is exact in fp64, so
    # the all-reduced S of the shards is the unsharded S bit for bit, and so must be everything after it
    X, Y = np.rint(4 * X), np.rint(4 * Y)

    def fit(c, Xl, Yl):
        c.set_option("xprod", 1)
        c.set_data(Xl, Yl, n_total=n)
        f = c.ppls_o2m(a, 40, 1e-6)
        return f, c.o2m_info()

    with Context(0) as c:
        whole, winfo = fit(c, X, Y)
    assert whole["ncomp"] == a and winfo["fits"] == a

    def work(rank, c):
        r0, nl = Context.shard_range(n, k, rank)
        return fit(c, X[r0:r0 + nl], Y[r0:r0 + nl])

    for f, info in _run_ranks(k, work):
        assert info == winfo
        for key in ("W", "C", "B", "sig"):
            assert np.array_equal(f[key], whole[key]), key
        for key in ("Number_steps", "Loglikelihoods", "Last_increment"):
            assert np.array_equal(f["Other_output"][key], whole["Other_output"][key]), key


@pytest.mark.parametrize("xprod", [0, 1], ids=["stream", "xprod"])
def test_three_shards_on_ordinary_data(xprod):
    """Real-valued data: the shards' all-reduced S differs from the unsharded S in its last bits, so the
    sharded fit equals the unsharded one to the suite's 1e-12 (tests/test_gpu_multirank.py) and every
    rank holds the same bits.  With xprod = 0 the start provider itself forms S, collectively."""
    from test_gpu_multirank import _run_ranks
    from ppls_amd import Context
    n, p, q, a, k = 500, 30, 20, 3, 3
    X, Y, _ = _oracle_fit(n, p, q, a, n + p)

    def fit(c, Xl, Yl):
        c.set_option("xprod", xprod)
        c.set_data(Xl, Yl, n_total=n)
        assert not c.xprod_info()["ready"]
        f = c.ppls_o2m(a, 30, -1.0)      # a fixed number of steps: the stop rule is not what is compared
        assert c.xprod_info()["ready"]
        return f, c.o2m_info()

    with Context(0) as c:
        whole, winfo = fit(c, X, Y)

    def work(rank, c):
        r0, nl = Context.shard_range(n, k, rank)
        return fit(c, X[r0:r0 + nl], Y[r0:r0 + nl])

    res = _run_ranks(k, work)
    for f, info in res:
        assert info["fits"] == winfo["fits"] == a
        for key in ("W", "C", "B", "sig"):
            assert np.array_equal(f[key], res[0][0][key]), key              # every rank the same bits
            assert np.abs(f[key] - whole[key]).max() <= 1e-12 * max(1.0, np.abs(whole[key]).max()), key
        assert list(f["Other_output"]["Number_steps"]) == list(whole["Other_output"]["Number_steps"])
        assert _relerr(f["Other_output"]["Loglikelihoods"], whole["Other_output"]["Loglikelihoods"]) < 1e-12


# ------------------------------------------------------------------------------ 5. cross-validation
@functools.lru_cache(maxsize=None)
def _cv_reference(n, p, q, a, K):
    """cv_PPLS's loop (crossval_PPLS.R:40-52) written out with the oracle's 'o2m' starts, for seeded fold
    labels: RMSEP K x a of every prefix of the components."""
    X, Y, _ = make_problem(n, p, q, a, seed=17)
    X, Y = X - X.mean(axis=0), Y - Y.mean(axis=0)
    perm = np.random.default_rng(3).permutation(n)
    from ppls_amd import fold_labels
    labels = fold_labels(n, K, perm)
    err = np.full((K, a), np.nan)
    for i in range(K):
        out = labels == i
        fit = o.ppls(X[~out], Y[~out], a, 30, -1.0, ["o2m"] * a)
        for j in range(1, a + 1):
            pred = X[out] @ fit["W"][:, :j] @ np.diag(fit["B"][:j]) @ fit["C"][:, :j].T
            err[i, j - 1] = np.sqrt(np.mean((Y[out] - pred) ** 2))
    for arr in (X, Y, perm, labels, err):
        arr.setflags(write=False)
    return X, Y, perm, labels, err


@pytest.mark.parametrize("xprod", [0, 1], ids=["stream", "xprod"])
def test_cv_on_resident_rows(xprod):
    from ppls_amd import crossval_PPLS, cv_PPLS
    n, p, q, a, K = 240, 16, 11, 2, 3
    X, Y, perm, _, ref = _cv_reference(n, p, q, a, K)
    with _ctx(xprod) as c:
        c.set_data(X, Y)
        mean, err = cv_PPLS(None, None, a, K, folds=perm, ctx=c, per_fold=True, EMsteps=30, atol=-1.0,
                            initialGuess="o2m_xprod")
        assert np.all(np.abs(err - ref[:, a - 1]) <= 1e-8 * ref[:, a - 1]) and mean == float(np.mean(err))
        cv = crossval_PPLS(None, None, [1, 2], K, shared_folds=True, ctx=c, folds=perm, EMsteps=30, atol=-1.0,
                           initialGuess="o2m_xprod")
        assert np.all(np.abs(cv["errors"] - ref.mean(axis=0)) <= 1e-8 * ref.mean(axis=0))


def test_cv_on_a_fold_stream():
    from ppls_amd import crossval_PPLS, cv_PPLS
    n, p, q, a, K = 240, 16, 11, 2, 3
    X, Y, _, labels, ref = _cv_reference(n, p, q, a, K)
    with _ctx() as c:
        c.stream_begin(p, q, False, False, nr_folds=K)
        for lo, hi in ((0, 90), (90, 170), (170, n)):
            c.stream_rows(X[lo:hi], Y[lo:hi], labels[lo:hi])
        c.stream_end()
        mean, err = cv_PPLS(None, None, a, K, ctx=c, per_fold=True, EMsteps=30, atol=-1.0, initialGuess="o2m_xprod")
        assert np.all(np.abs(err - ref[:, a - 1]) <= 1e-8 * ref[:, a - 1])
        cv = crossval_PPLS(None, None, [1, 2], K, shared_folds=True, ctx=c, EMsteps=30, atol=-1.0,
                           initialGuess="o2m_xprod")
        assert np.all(np.abs(cv["errors"] - ref.mean(axis=0)) <= 1e-8 * ref.mean(axis=0))
        assert c.stream_fold_info()["selected"] == -1 and c.n_total == n


# ------------------------------------------------------------------------------ 6. refusals and state
def test_refusals_and_state():
    from ppls_amd import PPLS, initial_guess
    n, p, q = 60, 12, 9
    rng = np.random.default_rng(8)
    X, Y = np.zeros((n, p)), np.zeros((n, q))
    X[:30], Y[30:] = rng.standard_normal((30, p)), rng.standard_normal((30, q))   # X'Y = 0 exactly
    with _ctx() as c:
        assert _code(lambda: c.o2m_start()) == E_STATE                  # no data
        assert _code(lambda: c.ppls_o2m(1, 5, 1e-4)) == E_STATE
        c.set_data(X, Y)
        assert _code(lambda: c.o2m_start()) == E_NUMERIC                # theta = 0
        assert "vanishes" in str(pytest.raises(Exception, c.ppls_o2m, 1, 5, 1e-4).value)
        Xg, Yg, _ = make_problem(n, p, q, 2, seed=1)
        c.set_data(Xg, Yg)
        from ppls_amd._lib import PplsError
        with pytest.raises(PplsError) as e:                              # k >= PPLS_RMAX
            c.o2m_start(np.zeros((p, 16)), np.zeros((q, 16)))
        assert e.value.code == E_ARG
        c.o2m_start()
        assert c.xprod_info()["ready"]
        c.xprod_release()
        assert not c.xprod_info()["ready"]
    with pytest.raises(ValueError, match="depends on the data"):
        initial_guess(p, q, "o2m_xprod")
    assert PPLS.__defaults__[3][0] == "equal" and PPLS.__defaults__[3][-1] == "o2m_xprod"
