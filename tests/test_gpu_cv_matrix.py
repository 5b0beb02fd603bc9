"""Every instantiation of the cross-validation kernels against long double: the scoring kernel
(ppls_heldout_sse, ppls_predict) inside the a-priori bars of tests/cv_bar.py at every tile, trip count, row-group
residue and grid regime; the streamed-fold error (ppls_heldout_sse_fold) against direct long-double residuals;
the row gather (ppls_set_data_from) bitwise in every row-length class and past one grid pass; the downdate
(ppls_xprod_downdate) beyond one grid pass against the long-double Gram of the kept rows.

Instantiations of ppls_cv_score_kernel<T, KT, PRED> and what reaches them:
  <double,  8, false>  test_heldout_sse[fp64-k1 .. k8-*], test_row_count_residues[k3], test_wide_reduce_and_grid_stride[fp64-k8]
  <double, 16, false>  test_heldout_sse[fp64-k9 .. k16-*], test_row_count_residues[k12], test_wide_reduce_and_grid_stride[fp64-k16]
  <float,   8, false>  test_heldout_sse[fp32-k1 .. k8-*]
  <float,  16, false>  test_heldout_sse[fp32-k9 .. k16-*], test_wide_reduce_and_grid_stride[fp32-k16]
  <double,  8, true>   test_predict[*-k1, *-k8]
  <double, 16, true>   test_predict[*-k9, *-k16]
(ppls_predict stages its rows in fp64, so there is no <float, KT, true>.)
"""
import ctypes as ct
import functools

import numpy as np
import pytest

import cv_bar as cb
from test_stream_host import split_rows

pytestmark = pytest.mark.gpu

HIP_ATTR_MULTIPROCESSOR_COUNT = 63     # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


def _ctx(dtype=0, xprod=0):
    from ppls_amd import Context
    c = Context(0)
    c.set_option("dtype", dtype)
    c.set_option("xprod", xprod)
    return c


@functools.lru_cache(maxsize=None)
def _cus():
    """The compute units of device 0 as the library reads them (hipDeviceProp_t::multiProcessorCount), asked of
    the HIP runtime the library is linked to."""
    from ppls_amd import _lib
    _lib.lib()
    hip = ct.CDLL("libamdhip64.so")
    v = ct.c_int(0)
    rc = hip.hipDeviceGetAttribute(ct.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, 0)
    assert rc == 0 and 1 <= v.value <= 4096, (rc, v.value)
    return v.value


@functools.lru_cache(maxsize=None)
def _data(n, p, q):
    X, Y = cb.make_data(n, p, q)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def _check_sse(tag, c, X, Y, W, C, B, rows, f32):
    """One ppls_heldout_sse against the long-double reference inside the bar; returns err / bar."""
    got = c.heldout_sse(W, C, B, rows)
    ref = cb.reference(X, Y, W, C, B, rows, f32, residuals=False)
    bar = cb.bars(X, Y, W, C, B, rows, f32, num_cus=_cus())
    ok, ratio = cb.inside(got, ref["sse"], bar["sse"])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = float(np.max(bar["sse"] / np.asarray(ref["sse"], dtype=np.float64)))
    print(f"{tag}: err / bar {ratio:.3g}, bar / SSE {rel:.3g}")
    assert got.shape == (W.shape[1],) and ok, (tag, ratio)
    assert np.array_equal(c.heldout_sse(W, C, B, rows), got), tag          # fixed-order sums: the same bits
    return ratio


# ------------------------------------------------------------------------------ a. held-out SSE
@pytest.mark.parametrize("shape", cb.SSE_SHAPES, ids=lambda s: "n%d_p%d_q%d" % s)
@pytest.mark.parametrize("k", cb.SSE_RANKS, ids=lambda k: f"k{k}")
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_heldout_sse(dtype, k, shape):
    n, p, q = shape
    f32 = bool(dtype)
    X, Y = _data(n, p, q)
    W, C, B = cb.fit_parts(p, q, k)
    worst = 0.0
    with _ctx(dtype) as c:
        for fit, Yf in (("random", Y), ("exact", cb.exact_fit(X, W, C, B, f32))):
            c.set_data(X, Yf)
            for kind in cb.ROW_KINDS:
                worst = max(worst, _check_sse(f"{fit} {kind}", c, X, Yf, W, C, B, cb.row_list(kind, n), f32))
            assert np.array_equal(c.heldout_sse(W, C, B, []), np.zeros(k))
    print(f"worst err / bar {worst:.3g}")


# ------------------------------------------------------------------------------ b. row-count residues
@pytest.mark.parametrize("k", [3, 12], ids=lambda k: f"k{k}")
def test_row_count_residues(k):
    """Row lists of every length 1 .. 17: every nvalid of RW = 8 and RW = 4, a full group followed by one row."""
    X, Y = _data(40, 37, 19)
    W, C, B = cb.fit_parts(37, 19, k)
    with _ctx() as c:
        c.set_data(X, Y)
        worst = max(_check_sse(f"{len(rows)} rows", c, X, Y, W, C, B, rows, False) for rows in cb.residue_rows())
    print(f"worst err / bar {worst:.3g}")


# ------------------------------------------------------------------------------ c. wide reduce, grid-stride
@pytest.mark.parametrize("dtype,k", [(0, 8), (0, 16), (1, 16)], ids=["fp64-k8", "fp64-k16", "fp32-k16"])
def test_wide_reduce_and_grid_stride(dtype, k):
    p, q, cus, rw = 12, 9, _cus(), cb.rows_per_wave(k)
    W, C, B = cb.fit_parts(p, q, k)
    n1, n2 = cb.wide_rows(k, cus)
    assert cb.cv_grid(n1, k, cus) * cb.WAVES > 256                        # per = 2 in the reduce kernel
    assert -(-n2 // rw) > cb.cv_grid(n2, k, cus) * cb.WAVES               # more row groups than waves: g += nw runs
    with _ctx(dtype) as c:
        for n in ((n2,) if dtype else (n1, n2)):
            X, Y = _data(n, p, q)
            c.set_data(X, Y)
            _check_sse(f"{n} rows", c, X, Y, W, C, B, np.arange(n), bool(dtype))


# ------------------------------------------------------------------------------ d. predict
@pytest.mark.parametrize("shape", cb.PREDICT_SHAPES, ids=lambda s: "n%d_p%d_q%d" % s)
@pytest.mark.parametrize("k", cb.PREDICT_RANKS, ids=lambda k: f"k{k}")
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
def test_predict(dtype, k, shape):
    """Both directions and layouts; the new rows are staged in fp64 whatever the context stores, so the
    reference never rounds them to fp32."""
    n, p, q = shape
    W, C, B = cb.fit_parts(p, q, k)
    rng = np.random.default_rng(5)
    with _ctx(dtype) as c:
        c.set_data(rng.standard_normal((5, p)), rng.standard_normal((5, q)))    # the shape; newdata is independent
        for xory in (0, 1):
            nd = _data(n, p, q)[xory]
            ref, bar = cb.reference_predict(nd, W, C, B, xory)["pred"], cb.bars_predict(nd, W, C, B, xory)
            got = c.predict(W, C, B, nd, xory)
            ok, ratio = cb.inside(got, ref, bar)
            print(f"xory={xory}: err / bar {ratio:.3g}, bar / max|pred| {bar.max() / float(np.abs(ref).max()):.3g}")
            assert got.shape == ref.shape and ok, (xory, ratio)
            assert np.array_equal(c.predict(W, C, B, np.asfortranarray(nd), xory), got), xory    # either layout


# ------------------------------------------------------------------------------ e. streamed-fold SSE
@functools.lru_cache(maxsize=None)
def _stream_case(n, p, q, K):
    X, Y = _data(n, p, q)
    labels = cb.seeded_labels(n, K, seed=n)
    Z = cb.scale_ref(np.hstack([X, Y]), True, True)[0]
    Z.setflags(write=False)
    return X, Y, labels, Z


@pytest.mark.parametrize("n,p,q,K", cb.STREAM_SHAPES)
@pytest.mark.parametrize("k", cb.STREAM_RANKS, ids=lambda k: f"k{k}")
def test_heldout_sse_fold(k, n, p, q, K):
    X, Y, labels, Z = _stream_case(n, p, q, K)
    bounds = split_rows(n)
    worst = 0.0
    with _ctx() as c:
        c.stream_begin(p, q, True, True, nr_folds=K)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            c.stream_rows(np.array(X[lo:hi]), np.array(Y[lo:hi]), np.array(labels[lo:hi]))
        c.stream_end()
        for f in range(K):
            ho = Z[labels == f]
            Sf, _, nf = c.stream_fold_get(f)
            assert nf == ho.shape[0]
            for name, (W, C, B) in cb.stream_triples(Z, labels, f, p, k).items():
                sse, mag = c.heldout_sse_fold(W, C, B, f)
                sse2, mag2 = c.heldout_sse_fold(W, C, B, f)
                assert np.array_equal(sse, sse2) and np.array_equal(mag, mag2)
                ref = cb.sse_direct(ho[:, :p], ho[:, p:], W, C, B)           # long double, on the rows themselves
                bar = cb.sse_bar(mag, nf, p, q, k, cb.K_SSE)
                ratio = float(np.max(np.abs(sse - ref) / bar))
                host, _ = cb.sse_quadratic(Sf, p, W, C, B)                    # the device's own S, another order
                order = float(np.max(np.abs(host - sse) / (cb.gamma(2 * p + q + k * k + 8) * mag)))
                print(f"fold {f} {name}: err / bar {ratio:.3g}, mag / sse {float(np.max(mag / sse)):.3g}, "
                      f"order / bar {order:.3g}")
                assert sse.shape == (k,) and np.all(np.abs(sse - ref) <= bar), (f, name, ratio)
                assert np.all(mag >= np.abs(sse))
                assert order <= 1.0, (f, name, order)
                worst = max(worst, ratio)
    print(f"worst err / bar {worst:.3g}")


# ------------------------------------------------------------------------------ f. gather
def _gather_equals_fresh(dtype, X, Y, rows):
    """set_data_from(rows) leaves what set_data(X[rows], Y[rows]) leaves: the rows, the sums of squares and,
    through the formed S over the padded layout, zeroed padding."""
    with _ctx(dtype) as src, _ctx(0) as dst, _ctx(dtype) as fresh:
        src.set_data(X, Y)
        dst.set_data_from(src, rows)                    # takes src's storage dtype
        fresh.set_data(X[rows], Y[rows])
        assert (dst.n_local, dst.p, dst.q) == (len(rows), X.shape[1], Y.shape[1])
        assert dst.ssq() == fresh.ssq()
        gx, gy = dst.get_data()
        fx, fy = fresh.get_data()
        assert np.array_equal(gx, fx) and np.array_equal(gy, fy)
        assert np.array_equal(gx, cb.stored(X[rows], bool(dtype))) and np.array_equal(gy, cb.stored(Y[rows], bool(dtype)))
        rx, ry = dst.get_data_rows()
        assert np.array_equal(rx, fx) and np.array_equal(ry, fy)
        dst.xprod_prepare()
        fresh.xprod_prepare()
        Sd, ldd = dst.xprod_matrix(padded=True)
        Sf, ldf = fresh.xprod_matrix(padded=True)
        assert ldd == ldf and Sd.shape == Sf.shape and np.array_equal(Sd, Sf)
        return Sd.shape[0], ldd


# 16-byte units of a row of X and of Y per (dtype, p, q): <= 16, 17 - 32 | 33 - 64, 65 - 128 | 129 - 256, > 256
# (there a thread copies more than one unit of a row)
GATHER = [(0, 3, 40, (2, 20)), (0, 100, 200, (50, 100)), (0, 300, 1030, (150, 515)),
          (1, 5, 100, (2, 25)), (1, 200, 500, (50, 128)), (1, 900, 2100, (232, 528))]


@pytest.mark.parametrize("dtype,p,q,units", GATHER, ids=[f"{'fp32' if g[0] else 'fp64'}-p{g[1]}-q{g[2]}" for g in GATHER])
def test_gather_row_classes(dtype, p, q, units):
    n = 50
    X, Y = _data(n, p, q)
    rows = np.sort(np.random.default_rng(4).permutation(n)[:30])
    P, ldx = _gather_equals_fresh(dtype, X, Y, rows)
    es = 4 if dtype else 8
    assert (ldx * es // 16, (P - ldx) * es // 16) == units            # the classes the widths were chosen for


def test_gather_row_stride():
    """70,000 rows of one unit: 4375 workgroups' worth of 16 rows, more than the 4096 launched."""
    n = 70001
    X, Y = _data(n, 2, 2)
    rows = np.delete(np.arange(n), n // 2)
    assert -(-len(rows) // 16) > 4096
    _gather_equals_fresh(0, X, Y, rows)


# ------------------------------------------------------------------------------ g. downdate
def test_downdate_beyond_one_grid_pass():
    """P = 1060: 561,800 double2 of S, more than the 2048 x 256 of one grid pass.  Entrywise against the
    long-double Gram of the kept rows; the downdate carries the rounding of the Gram of all rows:
    the stages of a formed S (test_stream_host.K_STAGES) and the subtraction.  (p and q are even, so this layout
    has no padding column; the padding check is written for the layout in general, and the gather tests above
    compare S over padded layouts bitwise.)"""
    n, p, q, n_out = 300, 1000, 60, 60
    X, Y = _data(n, p, q)
    out = np.sort(np.random.default_rng(3).permutation(n)[:n_out])
    keep = np.setdiff1d(np.arange(n), out)
    with _ctx() as src, _ctx() as dst:
        src.set_data(X, Y)
        dst.set_data_from(src, keep)
        dst.xprod_downdate(src, out)
        S = dst.xprod_matrix()
        Sp, ldx = dst.xprod_matrix(padded=True)
    assert Sp.shape[0] >= 1060 and (Sp.size // 2) > 2048 * 256
    D = np.hstack([X, Y]).astype(cb.L)
    G_keep = D[keep].T @ D[keep]
    G_all = G_keep + D[out].T @ D[out]
    bar = cb.gram_bar(G_all, n, cb.K_STAGES + 1)
    err = np.asarray(np.abs(S.astype(cb.L) - G_keep), dtype=np.float64)
    print(f"downdate: max err / bar {float(np.max(err / bar)):.3g}, bar / sqrt(S_jj S_ll) {cb.K_STAGES + 1} gamma({n})")
    assert S.shape == (p + q, p + q) and np.all(err <= bar)
    assert np.array_equal(Sp, Sp.T)
    live = np.zeros(Sp.shape[0], dtype=bool)
    live[:p] = True
    live[ldx:ldx + q] = True
    assert not Sp[~live].any() and not Sp[:, ~live].any()
