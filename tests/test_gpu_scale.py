"""R's scale() on the resident data: ppls_scale_data / ppls_get_scaling, Context.scale_data,
scale_data and predict_PPLS(rescale=True).

The comparison target is ``oracle.r_rng.r_scale`` (R's scale with long-double sums); the
``center`` / ``scale`` combinations it lacks are restated below the same way (``scale_ref``).  For
fp32 storage the target is applied to ``X.astype(float32).astype(float64)``: what the device holds.

Element-wise bound (derived, not tuned) for a fixed-order fp64 sum of n terms followed by one
subtraction and one division, with u = 2^-53:

    |z_dev - z_ref| <= 2 (n + 4) u (max_i |x_ij| / sd_j + |z_ij|)      (+ 2^-24 |z_ij| for fp32 storage:
                                                                        the single store rounding)
    centre, scale:  |got - ref| <= (n + 4) u max_i |x_ij|              (relative (n + 4) u max|x| / |value|)

A real indexing or padding bug is off by >= 1e-6.
"""
import os
import threading

import numpy as np
import pytest

from conftest import make_problem
from oracle import ppls_oracle as o
from oracle.r_rng import RRNG, r_scale

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
E_ARG, E_STATE = -1, -4
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (n, p, q, column offset)
SHAPES = {
    "odd_p": (67, 37, 19, 0.0),            # one padding column in fp64, three in fp32
    "row_blocks": (1031, 5, 3, 0.0),       # several row blocks, a ragged last one, fewer columns than a wave
    "ld2560": (40, 2100, 5, 0.0),          # fp64 rows padded to 4 KB
    "ld320": (67, 301, 19, 0.0),           # fp32 rows padded to 128 B
    "tiny": (2, 1, 1, 0.0),
    "offset1000": (67, 37, 19, 1000.0),    # |mean| >> sd: needs the centred second pass
}
COMBOS = [(True, True), (True, False), (False, True)]


def _ctx(dtype=0, xprod=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", xprod)
    return c


def _data(n, p, q, offset=0.0, seed=None):
    rng = np.random.default_rng(1000 * n + 10 * p + q if seed is None else seed)

    def block(m):
        j = np.arange(m)
        return rng.standard_normal((n, m)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7 + offset
    return block(p), block(q)


def _held(A, dtype):
    """What the device holds of A."""
    return A.astype(np.float32).astype(np.float64) if dtype else np.asarray(A, dtype=np.float64)


def scale_ref(x, center, scale):
    """R's scale(x, center, scale) with long-double column sums, as oracle.r_rng.r_scale forms them:
    (z, centre, scale); centre 0 / scale 1 where not requested, scale = sqrt(sum(xc^2) / (n - 1))."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    L = np.longdouble
    cen = np.array([float(np.sum(x[:, j].astype(L), dtype=L) / L(n)) for j in range(x.shape[1])]) if center \
        else np.zeros(x.shape[1])
    xc = x - cen
    sd = np.array([np.sqrt(float(np.sum((xc[:, j] * xc[:, j]).astype(L), dtype=L)) / max(1, n - 1))
                   for j in range(x.shape[1])]) if scale else np.ones(x.shape[1])
    return xc / sd, cen, sd


def _check_block(tag, got, x, center, scale, dtype, got_cen=None, got_scl=None):
    """got against scale_ref(x) under the module's bound; prints the figures before asserting."""
    n = x.shape[0]
    z, cen, sd = scale_ref(x, center, scale)
    if center and scale:
        assert np.array_equal(z, r_scale(x))          # the restatement is r_scale where r_scale applies
    xmax = np.abs(x).max(axis=0)
    bound = 2 * (n + 4) * U * (xmax / sd + np.abs(z)) + (2.0 ** -24 * np.abs(z) if dtype else 0.0)
    err = np.abs(got - z)
    print(f"{tag}: data err max {err.max():.3g}, max err/bound {np.max(err / bound):.3g}")
    assert got.shape == z.shape
    assert np.all(err <= bound)
    sbound = (n + 4) * U * xmax
    if got_cen is not None:
        print(f"{tag}: centre err/bound {np.max(np.abs(got_cen - cen) / sbound):.3g}, "
              f"scale err/bound {np.max(np.abs(got_scl - sd) / sbound):.3g}")
        assert np.all(np.abs(got_cen - cen) <= sbound)
        assert np.all(np.abs(got_scl - sd) <= sbound)


# ------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("center,scale", COMBOS, ids=["center_scale", "center", "scale"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scale_matches_r_scale(shape, center, scale, dtype):
    n, p, q, off = SHAPES[shape]
    X, Y = _data(n, p, q, off)
    with _ctx(dtype) as c:
        c.set_data(X, Y)
        c.scale_data(center, scale)
        gX, gY = c.get_data()
        rX, rY = c.get_data_rows()
        sc = c.scaling()
    assert np.array_equal(rX, gX) and np.array_equal(rY, gY)      # both download paths see the same rows
    tag = f"{shape} {'fp32' if dtype else 'fp64'} center={center} scale={scale}"
    _check_block(tag + " X", gX, _held(X, dtype), center, scale, dtype, sc["centerX"], sc["scaleX"])
    _check_block(tag + " Y", gY, _held(Y, dtype), center, scale, dtype, sc["centerY"], sc["scaleY"])


def test_module_scale_data_returns_r_attributes():
    from ppls_amd import scale_data
    X, Y = _data(67, 37, 19)
    with _ctx() as c:
        out = scale_data(X, Y, ctx=c)
        assert set(out) == {"centerX", "scaleX", "centerY", "scaleY"}
        gX, gY = c.get_data()
        _check_block("module X", gX, X, True, True, 0, out["centerX"], out["scaleX"])
        _check_block("module Y", gY, Y, True, True, 0, out["centerY"], out["scaleY"])
        again = scale_data(None, None, center=False, scale=False, ctx=c)     # resident data, a no-op
        assert all(np.array_equal(again[k], out[k]) for k in out)


# ------------------------------------------------------------------------------ 2. padding stays zero
def _theta(th):
    from ppls_amd import Theta
    return Theta(th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])


def _relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("shape,dtype", [("ld2560", 0), ("ld320", 1)], ids=["ld2560_fp64", "ld320_fp32"])
def test_padding_stays_zero(shape, dtype):
    """Both shapes take the panel sweep, which reads the padding columns of every row: had the apply
    pass written (0 - m) / sd there, ||X||^2 (summed over whole rows) and the streaming fit would
    differ from those of a context freshly loaded with the same values.  Tolerances against the
    oracle: tests/test_gpu_parity.py's."""
    n, p, q, _ = SHAPES[shape]
    r, steps = 2, 5
    X, Y = _data(n, p, q)
    th0 = make_problem(n, p, q, r, seed=3)[2]
    runs = {}
    with _ctx(dtype) as c, _ctx(dtype) as fresh:
        c.set_data(X, Y)
        c.scale_data()
        Xs, Ys = c.get_data()
        rX, rY = c.get_data_rows()
        assert np.array_equal(rX, Xs) and np.array_equal(rY, Ys)
        fresh.set_data(Xs, Ys)                     # fp32 storage: Xs are floats already, stored exactly
        assert c.ssq() == fresh.ssq()
        for xprod in (0, 1):
            c.set_option("xprod", xprod)
            runs[xprod] = c.em_run(_theta(th0), steps, -1.0)
        fresh.set_option("xprod", 0)
        est_f, ll_f, _, _ = fresh.em_run(_theta(th0), steps, -1.0)
    ref = o.ppls_simult(Xs, Ys, r, EMsteps=steps, atol=-1.0, theta0=th0)
    rest = ref["estimates"]
    for xprod, (est, ll, eout, neg) in runs.items():
        print(f"{shape} xprod={xprod}: loglik rel err {_relerr(ll, ref['loglik']):.3g}, "
              f"W err {np.abs(est.W - rest['W']).max():.3g}")
        assert len(ll) == len(ref["loglik"])
        assert _relerr(ll, ref["loglik"]) < 1e-10
        assert np.abs(est.W - rest["W"]).max() < 1e-8
        assert np.abs(est.C - rest["C"]).max() < 1e-8
        assert _relerr(est.B, np.diag(rest["B"])) < 1e-8
        assert _relerr(est.sigT, np.diag(rest["sigT"])) < 1e-8
        assert _relerr([est.sigE, est.sigF, est.sigH], [rest["sigE"], rest["sigF"], rest["sigH"]]) < 1e-8
    # the streaming sweep of the scaled context = that of the freshly loaded one, bit for bit
    assert np.array_equal(runs[0][1], ll_f) and np.array_equal(runs[0][0].W, est_f.W)


# ------------------------------------------------------------------------------ 3. context state
def test_context_state_after_scaling():
    from ppls_amd import PplsError
    n, p, q, _ = SHAPES["odd_p"]
    X, Y = _data(n, p, q)
    th0 = make_problem(n, p, q, 2, seed=4)[2]
    with _ctx(0, 1) as c, _ctx(0, 1) as fresh:
        c.set_data(X, Y)
        c.xprod_prepare()                          # S of the unscaled data: must not survive
        c.scale_data()
        Xs, Ys = c.get_data()
        fresh.set_data(Xs, Ys)
        assert c.ssq() == fresh.ssq()
        est, ll, _, _ = c.em_run(_theta(th0), 5, -1.0)
        est_f, ll_f, _, _ = fresh.em_run(_theta(th0), 5, -1.0)
        assert np.array_equal(ll, ll_f)
        assert np.array_equal(est.W, est_f.W) and np.array_equal(est.C, est_f.C)
        assert np.array_equal(est.B, est_f.B)
        for xprod in (0, 1):                        # an ppls_em_begin session ends with the data change
            c.set_option("xprod", xprod)
            c.em_begin(_theta(th0))
            c.em_iterate(1)
            c.scale_data()
            with pytest.raises(PplsError) as ei:
                c.em_iterate(1)
            assert ei.value.code == E_STATE
            c.em_begin(_theta(th0))                 # and a new one starts
            c.em_iterate(1)
            c.synchronize()


def test_no_data_is_a_state_error():
    from ppls_amd import PplsError
    with _ctx() as c:
        with pytest.raises(PplsError) as ei:
            c.scale_data()
        assert ei.value.code == E_STATE


# ------------------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_two_calls_compose(dtype):
    n, p, q, _ = SHAPES["odd_p"]
    X, Y = _data(n, p, q)
    with _ctx(dtype) as c, _ctx(dtype) as d:
        c.set_data(X, Y)
        c.scale_data(True, False)
        mid = c.scaling()
        assert np.all(mid["scaleX"] == 1.0) and np.all(mid["scaleY"] == 1.0)
        c.scale_data(False, True)
        gX, gY = c.get_data()
        sc = c.scaling()
        assert np.array_equal(sc["centerX"], mid["centerX"])      # centre + 1 * 0
        # scaling() maps resident values back to loaded ones.  Per call the stored value is
        # fl((x - c) / s) for the c, s that scaling() reports, so back = x up to a few u |x| in fp64
        # (12 (n + 4) u max|x| is generous) and, in fp32 storage, one float rounding of the resident
        # value per call: 2^-24 |x - c| <= 2^-24 * 2 max|x| each.
        xmax = np.abs(X).max()
        back = gX * sc["scaleX"] + sc["centerX"]
        assert np.abs(back - _held(X, dtype)).max() <= (12 * (n + 4) * U + (2 * 2 * 2.0 ** -24 if dtype else 0)) * xmax
        if dtype == 0:
            # fp64: within the bound of one scale_data(True, True)
            _check_block("composed X", gX, X, True, True, 0, sc["centerX"], sc["scaleX"])
            _check_block("composed Y", gY, Y, True, True, 0, sc["centerY"], sc["scaleY"])
        # a third call composes on: centre <- centre + scale * centre2, scale <- scale * scale2
        c.scale_data(True, True)
        sc3 = c.scaling()
        hX, _ = c.get_data()
        back = hX * sc3["scaleX"] + sc3["centerX"]
        assert np.abs(back - _held(X, dtype)).max() <= (12 * (n + 4) * U + (3 * 2 * 2.0 ** -24 if dtype else 0)) * xmax
        # set_data_from copies the transform, set_data resets it
        d.set_data_from(c, [0, 5, 6, 66])
        sd = d.scaling()
        assert all(np.array_equal(sd[k], sc3[k]) for k in sc3)
        c.set_data(X, Y)
        ident = c.scaling()
        assert not ident["centerX"].any() and not ident["centerY"].any()
        assert np.all(ident["scaleX"] == 1.0) and np.all(ident["scaleY"] == 1.0)


# ------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("block,col", [("X", 3), ("Y", 1)])
def test_constant_column_is_refused_and_data_untouched(block, col, dtype):
    from ppls_amd import PplsError
    X, Y = _data(64, 9, 4)
    (X if block == "X" else Y)[:, col] = 2.0       # the sum is exact, so sd is exactly 0
    with _ctx(dtype) as c:
        c.set_data(X, Y)
        before = c.get_data()
        ssq = c.ssq()
        with pytest.raises(PplsError) as ei:
            c.scale_data()
        assert ei.value.code == E_ARG
        assert f"{block} column {col + 1} " in str(ei.value)
        after = c.get_data()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert c.ssq() == ssq
        sc = c.scaling()
        assert not sc["centerX"].any() and np.all(sc["scaleY"] == 1.0)
        c.scale_data(True, False)                  # centring alone is fine
        assert not c.get_data()[0 if block == "X" else 1][:, col].any()


def test_single_row_and_noop():
    from ppls_amd import PplsError
    X, Y = _data(1, 5, 3)
    with _ctx() as c:
        c.set_data(X, Y)
        for center in (True, False):
            with pytest.raises(PplsError) as ei:
                c.scale_data(center, True)
            assert ei.value.code == E_ARG
        c.scale_data(False, False)                 # a no-op
        gX, gY = c.get_data()
        assert np.array_equal(gX, X) and np.array_equal(gY, Y)
        sc = c.scaling()
        assert not sc["centerX"].any() and np.all(sc["scaleX"] == 1.0)
        c.scale_data(True, False)                  # n = 1: every column minus itself
        gX, gY = c.get_data()
        assert not gX.any() and not gY.any()
        assert np.array_equal(c.scaling()["centerX"], X[0])


# ------------------------------------------------------------------------------ 6. shards
class ThreadAllReduce:
    """Sum over k host threads in rank order: every rank gets the bitwise-same result; a bounded
    barrier, so a rank that misses a collective fails the test instead of hanging it."""

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


def _run_ranks(X, Y, bounds, work):
    """work(ctx, rank) on 3 contexts of GPU 0 that hold the row ranges ``bounds`` of X, Y."""
    n = X.shape[0]
    red = ThreadAllReduce(3)
    out, errs = [None] * 3, []

    def body(rank):
        try:
            lo, hi = bounds[rank], bounds[rank + 1]
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.set_data(X[lo:hi], Y[lo:hi], n_total=n)
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
    return out, red


def test_sharded_scaling_equals_unsharded():
    n, p, q, _ = SHAPES["odd_p"]
    X, Y = _data(n, p, q)
    bounds = [0, 30, 67, 67]                       # 30 / 37 / 0 rows

    def work(c, rank):
        c.scale_data()                             # the zero-row rank joins and returns PPLS_OK
        return c.scaling(), c.get_data(), c.ssq()

    out, red = _run_ranks(X, Y, bounds, work)
    assert red.calls > 0
    for sc, _, ssq in out[1:]:
        assert all(np.array_equal(sc[k], out[0][0][k]) for k in sc)
        assert ssq == out[0][2]
    assert out[2][1][0].shape == (0, p)
    gX = np.vstack([o_[1][0] for o_ in out])
    gY = np.vstack([o_[1][1] for o_ in out])
    sc = out[0][0]
    _check_block("sharded X", gX, X, True, True, 0, sc["centerX"], sc["scaleX"])
    _check_block("sharded Y", gY, Y, True, True, 0, sc["centerY"], sc["scaleY"])


def test_sharded_refusal_is_the_same_on_every_rank():
    from ppls_amd import PplsError
    X, Y = _data(67, 9, 4)
    Y[:, 2] = 2.0
    bounds = [0, 30, 67, 67]

    def work(c, rank):
        before = c.get_data()
        try:
            c.scale_data()
        except PplsError as e:
            after = c.get_data()
            return e.code, str(e), np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        return 0, "", False

    out, _ = _run_ranks(X, Y, bounds, work)
    for code, msg, same in out:
        assert code == E_ARG and "Y column 3 " in msg and same


# ------------------------------------------------------------------------------ 7. the reference's example
def _assert_table(got, want):
    """tests/test_reference_examples.py's check of a print.PPLS table, restated."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 5], want[:, 5]), f"#steps {got[:, 5]} != printed {want[:, 5]}"
    assert np.abs(got[:, :5] - want[:, :5]).max() < 1e-9, f"\n{got}\n!=\n{want}"
    assert np.abs(got[:, 6]).max() < 5e-4


@pytest.mark.parametrize("xprod", [0, 1], ids=["stream", "xprod"])
def test_reference_example_scaled_on_the_device(xprod):
    """PPLS-Ex.R:39-43 with scale() done on the device: exX = scale(matrix(rnorm(100*10),100,10)),
    exY = scale(matrix(rnorm(100*12),100,12)) after set.seed(1), PPLS(exX, exY, 3, 1e4, 1e-4,
    'equal'); the printed table (#steps 729 / 811 / 87) is reproduced."""
    from ppls_amd import PPLS, print_PPLS, scale_data
    G = np.load(os.path.join(GOLD, "rcheck_ppls_ex.npz"))
    rng = RRNG(1)
    X = rng.matrix_rnorm(100, 10)
    Y = rng.matrix_rnorm(100, 12)
    with _ctx(0, xprod) as ctx:
        scale_data(X, Y, ctx=ctx)
        fit = PPLS(None, None, 3, 10000, 1e-4, "equal", ctx=ctx)
    rows, _ = print_PPLS(fit)
    assert list(G["table_equal"][:, 5]) == [729, 811, 87]
    _assert_table(rows, G["table_equal"])


# ------------------------------------------------------------------------------ 8. predict(rescale=True)
@pytest.mark.parametrize("xy", ["X", "Y"])
def test_predict_rescale(xy):
    from ppls_amd import PPLS, predict_PPLS, scale_data
    n, p, q = 80, 11, 6
    X, Y = _data(n, p, q, seed=8)
    Y += X[:, :q] * 0.8
    rng = np.random.default_rng(9)
    with _ctx() as ctx:
        sc = scale_data(X, Y, ctx=ctx)
        fit = PPLS(None, None, 2, 30, 1e-4, "equal", ctx=ctx)
        W, C, B = fit["W"], fit["C"], np.asarray(fit["B"])
        cX, sX, cY, sY = sc["centerX"], sc["scaleX"], sc["centerY"], sc["scaleY"]
        if xy == "X":
            new = rng.standard_normal((7, p)) * 3 + 1
            want = ((new - cX) / sX) @ W @ np.diag(B) @ C.T * sY + cY
            plain = new @ W @ np.diag(B) @ C.T
        else:
            new = rng.standard_normal((7, q)) * 3 + 1
            want = ((new - cY) / sY) @ C @ np.diag(1 / B) @ W.T * sX + cX
            plain = new @ C @ np.diag(1 / B) @ W.T
        got = predict_PPLS(fit, new, xy, ctx=ctx, rescale=True)
        assert got.shape == want.shape
        assert _relerr(got, want) < 1e-12
        assert np.array_equal(predict_PPLS(fit, new, xy, ctx=ctx), predict_PPLS(fit, new, xy, ctx=ctx, rescale=False))
        assert _relerr(predict_PPLS(fit, new, xy, ctx=ctx), plain) < 1e-12
        ctx.set_data(X, Y)                         # identity scaling: rescale changes nothing
        assert np.array_equal(predict_PPLS(fit, new, xy, ctx=ctx, rescale=True), predict_PPLS(fit, new, xy, ctx=ctx))
