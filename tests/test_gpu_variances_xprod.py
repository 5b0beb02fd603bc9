"""variances.PPLS_simult from the cross-products S alone (ppls_variances_xprod): standard
errors of the loadings on contexts that hold no rows.

* The information kernel alone (ppls_varinfo) against the a-priori bar of tests/varinfo_bar.py.
* The whole entry against oracle.variances_ppls_simult on the rows, with the Expectations taken at the
  estimates (``o.expect_m``), under the tolerances of tests/test_gpu_variances.py: W 1e-10 absolute;
  relative B_exp 1e-13, SSt_exp and SSt_star 1e-11, varMatrix and seLoad 1e-8.
"""
import functools
import threading

import numpy as np
import pytest

from conftest import make_problem
from oracle import ppls_oracle as o
from test_gpu_stream import ThreadAllReduce
from varinfo_bar import bars, inside, make_case, reference

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
STREAMED = "the rows were streamed and are not resident"


def _ctx():
    from ppls_amd import Context
    return Context(0)


def _theta(th):
    from ppls_amd import Theta
    return Theta(th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _scale(A):
    return (A - A.mean(0)) / A.std(0, ddof=1)


def _refs(X, Y, est):
    """The oracle's list for "X" and "Y" on the rows X, Y with the Expectations taken at est."""
    E = o.expect_m(X, Y, est["W"], est["C"], est["B"], est["sigE"], est["sigF"], est["sigH"], est["sigT"])
    fit = dict(estimates=est, Expectations=E)
    with np.errstate(invalid="ignore"):
        return fit, {xy: o.variances_ppls_simult(fit, X if xy == "X" else Y, xy) for xy in ("X", "Y")}


@functools.lru_cache(maxsize=None)
def _case(n, p, q, r, seed, scaled=False):
    """(X, Y, th0, fit at the estimates, oracle lists), computed once and shared."""
    X, Y, th0 = make_problem(n, p, q, r, seed=seed)
    if scaled:
        X, Y = _scale(X), _scale(Y)
    f = o.ppls_simult(X, Y, r, EMsteps=20, atol=-np.inf, theta0=th0)
    fit, refs = _refs(X, Y, f["estimates"])
    for v in (X, Y):
        v.setflags(write=False)
    return X, Y, th0, fit, refs


def _stream(c, X, Y, nchunks=3, center=False, scale=False):
    b = [X.shape[0] * k // nchunks for k in range(nchunks + 1)]
    c.stream_begin(X.shape[1], Y.shape[1], center, scale)
    for lo, hi in zip(b[:-1], b[1:]):
        c.stream_rows(np.array(X[lo:hi]), np.array(Y[lo:hi]))
    c.stream_end()


def _check(got, ref, what=""):
    a = ref["W"].shape[1]
    assert np.abs(got["W"] - ref["W"]).max() < 1e-10, what
    for i in range(a):
        g, r = got["components"][i], ref["components"][i]
        assert _rel(g["B_exp"], r["B_exp"]) < 1e-13, what
        assert _rel(g["SSt_exp"], r["SSt_exp"]) < 1e-11, what
        assert _rel(g["SSt_star"], r["SSt_star"]) < 1e-11, what
        assert _rel(got["varMatrix"][i], ref["varMatrix"][i]) < 1e-8, what
    assert _rel(got["seLoad"], ref["seLoad"]) < 1e-8, what


def _same_run(a, b):
    return (all(np.array_equal(getattr(a[0], k), getattr(b[0], k)) for k in ("W", "C", "B", "sigT")) and
            (a[0].sigE, a[0].sigF, a[0].sigH) == (b[0].sigE, b[0].sigF, b[0].sigH) and np.array_equal(a[1], b[1]))


# ------------------------------------------------------------------------------ 1. the kernel alone
@pytest.fixture(scope="module")
def kctx():
    c = _ctx()
    yield c
    c.close()


@pytest.mark.parametrize("a", [1, 3, 16])
@pytest.mark.parametrize("off", [0, 38])
@pytest.mark.parametrize("p", [1, 2, 37, 64, 65, 129, 150])
def test_kernel_alone_lies_inside_the_bar(kctx, p, off, a):
    c = make_case(p, off, a)
    J, _, _ = kctx.varinfo(c["S"], off, p, c["cxt"], c["w"], c["ctt"], c["k1"], c["k2"], c["bstar"], c["sigE"], c["N"],
                           full=False)
    assert np.all(np.isfinite(J))                        # nothing outside the block was used, nothing left unwritten
    assert np.array_equal(J, J.transpose(0, 2, 1))       # symmetric bit for bit
    ok, worst = inside(J.transpose(0, 2, 1), reference(c)[0], bars(c)[0])
    print(f"varinfo p={p} off={off} a={a}: max err / bar {worst:.3g}")
    assert ok


def test_kernel_alone_sst_exp_and_star(kctx):
    p, off, a = 65, 38, 3
    c = make_case(p, off, a)
    J, SE, SS = kctx.varinfo(c["S"], off, p, c["cxt"], c["w"], c["ctt"], c["k1"], c["k2"], c["bstar"], c["sigE"], c["N"])
    rJ, rE, rS = reference(c)
    bJ, bE, bS = bars(c)
    for name, got, ref, bar in (("J", J, rJ, bJ), ("SSt_exp", SE, rE, bE), ("SSt_star", SS, rS, bS)):
        assert np.array_equal(got, got.transpose(0, 2, 1)), name
        ok, worst = inside(got.transpose(0, 2, 1), ref, bar)
        print(f"varinfo {name} p={p}: max err / bar {worst:.3g}")
        assert ok, name
    for i in range(a):   # J = SSt_exp - bstar I, from the same values
        assert np.array_equal(J[i], np.where(np.eye(p) > 0, SE[i] - c["bstar"][i], SE[i]))


# ------------------------------------------------------------------------------ 2. streamed contexts
@pytest.mark.parametrize("chol", [1, 2, 0], ids=["chol", "chol_rocsolver", "lu"])
@pytest.mark.parametrize("xy", ["X", "Y"])
def test_streamed_matches_oracle(xy, chol):
    import ppls_amd
    X, Y, th0, fit, refs = _case(700, 37, 29, 3, 61)
    with _ctx() as c:
        _stream(c, X, Y)
        c.set_option("var_chol", chol)
        got = ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True)
        _check(got, refs[xy])
        E = fit["Expectations"]
        assert _rel(got["Ctt"], E["Ctt"] if xy == "X" else E["Cuu"]) < 1e-10
        # full=False, want_var=False: the same seLoad
        lean = ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, full=False, from_xprod=True)
        assert lean["components"][0]["SSt_exp"] is None and np.array_equal(lean["seLoad"], got["seLoad"])
        out = c.variances_xprod(_theta(fit["estimates"]), 0 if xy == "X" else 1, full=False, want_var=False)
        assert out[3] is None and out[5] is None and np.array_equal(out[4], got["seLoad"])


@pytest.mark.parametrize("xy", ["X", "Y"])
def test_streamed_multi_block(xy):
    """p = 150, q = 131: three 64-blocks per side, a partial last one, the Y block starting mid-tile."""
    import ppls_amd
    X, Y, th0, fit, refs = _case(1500, 150, 131, 4, 67)
    got = {}
    with _ctx() as c:
        _stream(c, X, Y)
        for chol in (1, 2):
            c.set_option("var_chol", chol)
            got[chol] = ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True)
    _check(got[1], refs[xy])
    for i in range(4):
        assert _rel(got[1]["varMatrix"][i], got[2]["varMatrix"][i]) < 1e-9
        assert np.array_equal(got[1]["varMatrix"][i], got[1]["varMatrix"][i].T)


@pytest.mark.parametrize("n,p,q,r,seed", [(900, 130, 66, 16, 5), (300, 2, 3, 1, 9)])
def test_streamed_other_shapes(n, p, q, r, seed):
    import ppls_amd
    X, Y, th0, fit, refs = _case(n, p, q, r, seed)
    with _ctx() as c:
        _stream(c, X, Y)
        for xy in ("X", "Y"):
            _check(ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True), refs[xy], xy)


@pytest.mark.parametrize("n,p,q,r,seed", [(120, 12, 9, 2, 2), (257, 64, 64, 2, 7), (400, 70, 5, 1, 3)])
def test_centred_and_scaled_stream(n, p, q, r, seed):
    """The stream centres and scales; the oracle sees the rows scale()d on the host (ddof = 1)."""
    import ppls_amd
    X, Y, _ = make_problem(n, p, q, r, seed=seed)
    _, _, th0, fit, refs = _case(n, p, q, r, seed, scaled=True)
    with _ctx() as c:
        _stream(c, X, Y, center=True, scale=True)
        for xy in ("X", "Y"):
            _check(ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True), refs[xy], xy)


# ------------------------------------------------------------------------------ 3. resident
def test_resident_agrees_with_ppls_variances():
    X, Y, th0, fit, refs = _case(700, 37, 29, 3, 61)
    th = _theta(fit["estimates"])
    with _ctx() as c:
        c.set_data(np.array(X), np.array(Y))
        e = c.estep(th, want_mu=True)
        assert not c.xprod_info(3)["ready"]
        first = c.variances_xprod(th, 0)                 # forms S, which stays
        assert c.xprod_info(3)["ready"]
        c.xprod_prepare()
        for xory, mu, Cd in ((0, e.mu_T, e.Ctt), (1, e.mu_U, e.Cuu)):
            W0, B0, V0, se0, SE0, SS0 = c.variances(mu, Cd, th.sigE, xory)
            W, Cg, Bx, V, se, SE, SS = c.variances_xprod(th, xory)
            assert np.abs(W - W0).max() < 1e-10 and _rel(Cg, Cd) < 1e-10
            assert _rel(Bx, B0) < 1e-13 and _rel(SE, SE0) < 1e-11 and _rel(SS, SS0) < 1e-11
            assert _rel(V, V0) < 1e-8 and _rel(se, se0) < 1e-8
            if xory == 0:
                assert all(np.array_equal(u, v) for u, v in zip(first, (W, Cg, Bx, V, se, SE, SS)))


# ------------------------------------------------------------------------------ 4. fold stream
def test_fold_stream_follows_the_selection():
    import ppls_amd
    X, Y, th0, fit, refs = _case(700, 37, 29, 3, 61)
    n = X.shape[0]
    lab = (np.arange(n) * 7 % 3).astype(np.int32)
    keep = lab != 1
    _, sub = _refs(X[keep], Y[keep], fit["estimates"])
    with _ctx() as c:
        c.stream_begin(X.shape[1], Y.shape[1], False, False, nr_folds=3)
        for lo, hi in ((0, 250), (250, 251), (251, n)):
            c.stream_rows(np.array(X[lo:hi]), np.array(Y[lo:hi]), fold=lab[lo:hi])
        c.stream_end()
        c.stream_select(1)
        for xy in ("X", "Y"):
            _check(ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True), sub[xy], "fold 1 out " + xy)
        c.stream_select(-1)
        for xy in ("X", "Y"):
            _check(ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True), refs[xy], "all folds " + xy)


# ------------------------------------------------------------------------------ 5. bootstrap replicate
def test_bootstrap_replicate():
    import ppls_amd
    X, Y, th0, fit, _ = _case(700, 37, 29, 3, 61)
    counts = np.random.default_rng(3).multinomial(X.shape[0], np.full(X.shape[0], 1.0 / X.shape[0])).astype(np.int32)
    _, rep = _refs(np.repeat(X, counts, axis=0), np.repeat(Y, counts, axis=0), fit["estimates"])
    with _ctx() as src, _ctx() as work:
        src.set_data(np.array(X), np.array(Y))
        work.xprod_resample(src, counts)
        for xy in ("X", "Y"):
            _check(ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=work, from_xprod=True), rep[xy], xy)


# ------------------------------------------------------------------------------ 6. indefinite information
def test_indefinite_information_takes_the_lu_route():
    import ppls_amd
    X, Y, th0 = make_problem(300, 20, 11, 2, seed=4)
    X, Y = 0.1 * X, 0.1 * Y
    fit, refs = _refs(X, Y, th0)
    with _ctx() as c:
        _stream(c, X, Y)
        c.set_option("var_chol", 1)
        for xy in ("X", "Y"):
            ref = refs[xy]
            ev = np.concatenate([np.linalg.eigvalsh(k["SSt_exp"] - k["B_exp"]) for k in ref["components"]])
            assert ev.min() < 0 < ev.max()                # a J_i is indefinite: no Cholesky factor exists
            assert np.isnan(ref["seLoad"]).any()
            got = ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True)
            assert np.array_equal(np.isnan(got["seLoad"]), np.isnan(ref["seLoad"]))
            fin = np.isfinite(ref["seLoad"])
            assert _rel(got["seLoad"][fin], ref["seLoad"][fin]) < 1e-8
            for i in range(2):
                assert _rel(got["varMatrix"][i], ref["varMatrix"][i]) < 1e-8
            # the route itself: with var_chol = 0 the batch goes to LU at once, from the same J (the fallback
            # forms it again with the same launch), so the fallback's result is the LU route's bit for bit --
            # and not a mirrored Cholesky inverse, which would be exactly symmetric
            c.set_option("var_chol", 0)
            lu = ppls_amd.variances_PPLS_simult(fit, None, xy, ctx=c, from_xprod=True)
            c.set_option("var_chol", 1)
            assert np.array_equal(lu["seLoad"], got["seLoad"], equal_nan=True)
            for i in range(2):
                assert np.array_equal(lu["varMatrix"][i], got["varMatrix"][i])


# ------------------------------------------------------------------------------ 7. refusals and state
def test_refusals_leave_the_context_as_it_was():
    import ppls_amd
    from ppls_amd import PplsError
    X, Y, th0, fit, refs = _case(120, 12, 9, 2, 2)
    th = _theta(fit["estimates"])
    with _ctx() as c:
        with pytest.raises(PplsError) as e:                       # no data
            c.variances_xprod(th, 0)
        assert e.value.code == E_STATE
        _stream(c, X, Y)
        base = c.em_run(_theta(th0), 8, -np.inf, 0, want_mu=False)
        wide = dict(th0, W=np.eye(12, 17), C=np.eye(9, 17)[:, ::-1], B=np.ones(17), sigT=np.ones(17))
        for call in (lambda: c.variances_xprod(th, 2),            # xory = 2
                     lambda: c.variances_xprod(_theta(wide), 0)):   # r = 17
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_ARG
            assert _same_run(c.em_run(_theta(th0), 8, -np.inf, 0, want_mu=False), base)
        with pytest.raises(ValueError):
            ppls_amd.variances_PPLS_simult(fit, X, "X", ctx=c, from_xprod=True)
        norows = dict(estimates=fit["estimates"],               # a streamed context's own fit carries no mu rows
                      Expectations=dict(mu_T=np.zeros((0, 2)), mu_U=np.zeros((0, 2)), Ctt=np.eye(2), Cuu=np.eye(2)))
        with pytest.raises(PplsError, match=STREAMED) as e:       # without the keyword: ppls_variances' refusal
            ppls_amd.variances_PPLS_simult(norows, None, "X", ctx=c)
        assert e.value.code == E_STATE
        assert _same_run(c.em_run(_theta(th0), 8, -np.inf, 0, want_mu=False), base)
        got = ppls_amd.variances_PPLS_simult(fit, None, "X", ctx=c, from_xprod=True)    # a successful call
        _check(got, refs["X"])
        assert _same_run(c.em_run(_theta(th0), 8, -np.inf, 0, want_mu=False), base)
        # an open stream: refused, and the stream goes on to the same S
        c.stream_begin(12, 9, False, False)
        c.stream_rows(np.array(X[:40]), np.array(Y[:40]))
        with pytest.raises(PplsError) as e:
            c.variances_xprod(th, 0)
        assert e.value.code == E_STATE and "stream is open" in str(e.value)
        c.stream_rows(np.array(X[40:80]), np.array(Y[40:80]))
        c.stream_rows(np.array(X[80:]), np.array(Y[80:]))
        c.stream_end()
        assert _same_run(c.em_run(_theta(th0), 8, -np.inf, 0, want_mu=False), base)
    # r = 3 with p = 2
    X2, Y2, th2, _, _ = _case(300, 2, 3, 1, 9)
    three = dict(th2, W=np.eye(2, 3), C=np.eye(3), B=np.ones(3), sigT=np.ones(3))
    with _ctx() as c:
        _stream(c, X2, Y2)
        base = c.em_run(_theta(th2), 8, -np.inf, 0, want_mu=False)
        with pytest.raises(PplsError) as e:
            c.variances_xprod(_theta(three), 0)
        assert e.value.code == E_ARG
        assert _same_run(c.em_run(_theta(th2), 8, -np.inf, 0, want_mu=False), base)


# ------------------------------------------------------------------------------ 8. shards
def test_sharded_ranks_agree_without_a_collective():
    X, Y, th0, fit, _ = _case(700, 37, 29, 3, 61)
    th = fit["estimates"]
    chunks = [[(0, 1), (1, 170)], [(170, 334), (334, 335), (335, 700)], []]
    red = ThreadAllReduce(3)
    out, errs, calls = [None] * 3, [], [0, 0, 0]

    def body(rank):
        try:
            with _ctx() as c:
                inner = red.fn(rank)

                def counted(buf):
                    calls[rank] += 1
                    inner(buf)
                c.set_reducer(counted)
                c.stream_begin(X.shape[1], Y.shape[1], False, False)
                for lo, hi in chunks[rank]:
                    c.stream_rows(np.array(X[lo:hi]), np.array(Y[lo:hi]))
                c.stream_end()
                before = calls[rank]
                res = [c.variances_xprod(_theta(th), xory) for xory in (0, 1)]
                out[rank] = (res, calls[rank] - before)
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
    with _ctx() as one:
        _stream(one, X, Y)
        want =[one.variances_xprod(_theta(th), xory) for xory in (0, 1)]
    for res, ncalls in out:
        assert ncalls == 0                               # S is global: no reducer call
        for xory in (0, 1):
            assert all(np.array_equal(u, v) for u, v in zip(res[xory], out[0][0][xory]))   # the same bits on every rank
            W, Cd, Bx, V, se, SE, SS = res[xory]
            W1, Cd1, Bx1, V1, se1, SE1, SS1 = want[xory]
            assert np.abs(W - W1).max() < 1e-10 and _rel(Bx, Bx1) < 1e-13
            assert _rel(SE, SE1) < 1e-11 and _rel(SS, SS1) < 1e-11 and _rel(V, V1) < 1e-8 and _rel(se, se1) < 1e-8
