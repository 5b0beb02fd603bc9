"""The cross-validation scoring kernel without a GPU: the host model of tests/cv_bar.py lies inside
the a-priori bars on every shape of tests/test_gpu_cv_matrix.py, each of the six seeded defects falls outside
them where its path exists and stays inside where it does not, the exact fit has an absolute bar, the
streamed-fold quadratic form meets its bar at the shapes of group e, and the launch geometry restated in
cv_bar is the library's."""
import ctypes as ct
import functools

import numpy as np
import pytest

import cv_bar as cb

CUS = 256          # the compute units the GPU run sees; the row lists of groups a and b never reach the cap
SMALL_CUS = 2      # a pretend device: the grid-stride of group c at 8 workgroups instead of 1024


@functools.lru_cache(maxsize=None)
def _data(n, p, q):
    X, Y = cb.make_data(n, p, q)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def _ratio(X, Y, W, C, B, rows, f32, num_cus=CUS, defect=None):
    """(inside, worst err / bar, bar / SSE of the reference) of the model's prefix sums."""
    ref = cb.reference(X, Y, W, C, B, rows, f32, residuals=False)
    bar = cb.bars(X, Y, W, C, B, rows, f32, num_cus=num_cus)
    got = cb.model(X, Y, W, C, B, rows, f32, num_cus=num_cus, defect=defect)
    ok, ratio = cb.inside(got, ref["sse"], bar["sse"])
    return ok, ratio, bar["sse"] / np.asarray(ref["sse"], dtype=np.float64)


# ------------------------------------------------------------------------------ 1. the model inside the bars
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("k", cb.SSE_RANKS)
@pytest.mark.parametrize("shape", cb.SSE_SHAPES, ids=lambda s: "n%d_p%d_q%d" % s)
def test_model_inside_bars_group_a(shape, k, f32):
    n, p, q = shape
    X, Y = _data(n, p, q)
    W, C, B = cb.fit_parts(p, q, k)
    Yx = cb.exact_fit(X, W, C, B, f32)
    worst = 0.0
    for kind in cb.ROW_KINDS:
        rows = cb.row_list(kind, n)
        ok, ratio, rel = _ratio(X, Y, W, C, B, rows, f32)
        print(f"{kind}: err / bar {ratio:.3g}, bar / SSE {rel.min():.3g} .. {rel.max():.3g}")
        assert ok, (kind, ratio)
        assert np.all(rel < 1e-11), (kind, rel)                     # a bar, not a blanket
        okx, ratiox, _ = _ratio(X, Yx, W, C, B, rows, f32)
        print(f"{kind}, exact fit: err / bar {ratiox:.3g}")
        assert okx, (kind, ratiox)
        worst = max(worst, ratio, ratiox)
    print(f"worst err / bar {worst:.3g}")
    assert worst < 1.0


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", cb.SSE_SHAPES, ids=lambda s: "n%d_p%d_q%d" % s)
def test_exact_fit_has_an_absolute_bar(shape, f32):
    """Y = X W diag(B) C' to rounding: the reference SSE is rounding noise, the bar absolute and far below
    ||Y||^2: the residual is formed directly and nothing cancels."""
    n, p, q = shape
    X, _ = _data(n, p, q)
    for k in (3, 16):
        W, C, B = cb.fit_parts(p, q, k)
        Y = cb.exact_fit(X, W, C, B, f32)
        rows = np.arange(n)
        ref = cb.reference(X, Y, W, C, B, rows, f32, residuals=False)
        bar = cb.bars(X, Y, W, C, B, rows, f32, num_cus=CUS)["sse"]
        ssy = float((cb.stored(Y, f32) ** 2).sum())
        got = cb.model(X, Y, W, C, B, rows, f32, num_cus=CUS)
        ok, ratio = cb.inside(got, ref["sse"], bar)
        print(f"k={k}: SSE_k {float(ref['sse'][-1]):.3g}, bar {bar[-1]:.3g}, ||Y||^2 {ssy:.3g}, err / bar {ratio:.3g}")
        assert ok, ratio
        assert bar[-1] < 1e-20 * ssy and float(ref["sse"][-1]) < 1e-12 * ssy


@pytest.mark.parametrize("k", [3, 12])
def test_model_inside_bars_group_b(k):
    X, Y = _data(40, 37, 19)
    W, C, B = cb.fit_parts(37, 19, k)
    worst = 0.0
    for rows in cb.residue_rows():
        ok, ratio, _ = _ratio(X, Y, W, C, B, rows, False)
        assert ok, (len(rows), ratio)
        worst = max(worst, ratio)
    print(f"worst err / bar {worst:.3g}")


@pytest.mark.parametrize("k,f32", [(8, False), (16, False), (16, True)])
def test_model_inside_bars_group_c(k, f32):
    """nrows_1 as on the device (more than 256 partials, per = 2); nrows_2 cut to a pretend device of SMALL_CUS
    compute units: the smallest row count with one grid-stride trip and a ragged tail."""
    p, q = 12, 9
    W, C, B = cb.fit_parts(p, q, k)
    rw = cb.rows_per_wave(k)
    n1, _ = cb.wide_rows(k, CUS)
    _, n2 = cb.wide_rows(k, SMALL_CUS)
    assert cb.cv_grid(n1, k, CUS) * cb.WAVES > 256
    assert -(-n2 // rw) > cb.cv_grid(n2, k, SMALL_CUS) * cb.WAVES
    for n, cus in ((n1, CUS), (n2, SMALL_CUS)):
        X, Y = _data(n, p, q)
        ok, ratio, rel = _ratio(X, Y, W, C, B, np.arange(n), f32, num_cus=cus)
        print(f"n={n} cus={cus}: err / bar {ratio:.3g}, bar / SSE {rel.max():.3g}")
        assert ok, (n, ratio)


@pytest.mark.parametrize("xory", [0, 1])
@pytest.mark.parametrize("k", cb.PREDICT_RANKS)
@pytest.mark.parametrize("shape", cb.PREDICT_SHAPES, ids=lambda s: "n%d_p%d_q%d" % s)
def test_model_inside_bars_group_d(shape, k, xory):
    n, p, q = shape
    W, C, B = cb.fit_parts(p, q, k)
    nd = _data(n, p, q)[xory]
    ref, bar = cb.reference_predict(nd, W, C, B, xory), cb.bars_predict(nd, W, C, B, xory)
    got = cb.model_predict(nd, W, C, B, xory)
    assert got.shape == ref["pred"].shape == bar.shape == (n, p if xory else q)
    ok, ratio = cb.inside(got, ref["pred"], bar)
    print(f"err / bar {ratio:.3g}")
    assert ok, ratio
    assert np.all(bar <= 1e-12 * (1 + np.abs(np.asarray(ref["pred"], dtype=np.float64)).max()))
    for defect in (1, 2, 6):      # the defects that reach the prediction rows, where their path exists
        bad = not cb.inside(cb.model_predict(nd, W, C, B, xory, defect=defect), ref["pred"], bar)[0]
        want = {1: (p if xory else q) > 128, 2: k > 8 and n > 1, 6: n > 1}[defect]
        assert bad == want, (defect, bad)


# ------------------------------------------------------------------------------ 2. the seeded defects
def _outside(n, p, q, k, rows, f32, defect, num_cus=CUS):
    X, Y = _data(n, p, q)
    W, C, B = cb.fit_parts(p, q, k)
    assert _ratio(X, Y, W, C, B, rows, f32, num_cus)[0]             # the model itself is inside
    ok, ratio, _ = _ratio(X, Y, W, C, B, rows, f32, num_cus, defect)
    if not ok:
        assert ratio > 1e6, (defect, ratio)                          # a miss is never a near miss
    return not ok


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_defect_1_needs_more_than_64_units(f32):
    assert _outside(70, 261, 259, 3, np.arange(70), f32, 1)          # 130 (fp64), 65 (fp32) units of Y
    assert _outside(70, 261, 259, 16, cb.row_list("last", 70), f32, 1)
    q64 = 256 if f32 else 128                                        # exactly 64 units: one trip
    assert cb.lane_terms(q64, f32)[2] == 64
    assert not _outside(40, 6, q64, 16, np.arange(40), f32, 1)
    assert _outside(40, 6, q64 + 1, 16, np.arange(40), f32, 1)       # one unit more
    assert _outside(40, 6, 256, 16, np.arange(40), f32, 1) == (not f32)     # 128 units in fp64, 64 in fp32


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_defect_2_needs_the_wide_tile_and_a_second_row(f32):
    for k in (9, 15, 16):
        assert _outside(67, 37, 19, k, np.arange(67), f32, 2)
    for k in (1, 7, 8):
        assert not _outside(67, 37, 19, k, np.arange(67), f32, 2)    # KT = 8: lane rr * 8 + m is the right one
    assert not _outside(67, 37, 19, 16, cb.row_list("last", 67), f32, 2)   # row 0 of a group: lane m either way


def test_defect_3_needs_a_partial_group():
    for k, rw in ((3, 8), (12, 4)):
        assert cb.rows_per_wave(k) == rw
        for rows in cb.residue_rows():
            assert _outside(40, 37, 19, k, rows, False, 3) == (len(rows) % rw != 0), (k, len(rows))


def test_defect_4_needs_more_groups_than_waves():
    for k in (8, 16):
        n1, _ = cb.wide_rows(k, CUS)
        _, n2 = cb.wide_rows(k, SMALL_CUS)
        assert _outside(n2, 12, 9, k, np.arange(n2), False, 4, SMALL_CUS)
        assert not _outside(n1, 12, 9, k, np.arange(n1), False, 4, CUS)     # 66 workgroups of 1024: no stride
        assert _outside(n1, 12, 9, k, np.arange(n1), False, 4, SMALL_CUS)


def test_defect_5_needs_more_than_256_partials():
    for k in (8, 16):
        rw = cb.rows_per_wave(k)
        n1, _ = cb.wide_rows(k, CUS)
        assert _outside(n1, 12, 9, k, np.arange(n1), False, 5)
        nfull = 64 * cb.WAVES * rw                                   # exactly 256 partials
        assert cb.cv_grid(nfull, k, CUS) * cb.WAVES == 256
        assert not _outside(nfull, 12, 9, k, np.arange(nfull), False, 5)
        assert _outside(nfull + 1, 12, 9, k, np.arange(nfull + 1), False, 5)


def test_defect_6_needs_a_second_row():
    for k in (3, 12):
        for rows in cb.residue_rows():
            assert _outside(40, 37, 19, k, rows, False, 6) == (len(rows) > 1), (k, len(rows))


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_what_the_old_shapes_could_see(f32):
    """(67, 37, 19) at k = 3 with a third of the rows, all rows and the last row, the shape every test of
    heldout_sse had: 10 units of Y at most, KT = 8, at most 3 workgroups and 12 partials.  Defects 1, 2, 4 and 5
    are invisible on every row list: their paths do not exist there.  Defect 6 is invisible on the one-row list
    and visible on the others (that is how the first version's bug was found); defect 3 is visible on all three,
    none of 22, 67 and 1 being a multiple of 8."""
    lists = {kind: cb.row_list(kind, 67) for kind in cb.ROW_KINDS}
    assert [len(lists[kind]) for kind in cb.ROW_KINDS] == [22, 67, 1]
    for kind, rows in lists.items():
        for defect in (1, 2, 4, 5):
            assert not _outside(67, 37, 19, 3, rows, f32, defect), (kind, defect)
        assert _outside(67, 37, 19, 3, rows, f32, 3), kind
        assert _outside(67, 37, 19, 3, rows, f32, 6) == (len(rows) > 1), kind


# ------------------------------------------------------------------------------ 3. the streamed-fold form
@pytest.mark.parametrize("k", cb.STREAM_RANKS)
@pytest.mark.parametrize("n,p,q,K", cb.STREAM_SHAPES)
def test_streamed_fold_form_meets_its_bar(n, p, q, K, k):
    X, Y = _data(n, p, q)
    labels = cb.seeded_labels(n, K, seed=n)
    refs, _, _ = cb.fold_refs(X, Y, labels, K, True, True)
    Z = np.asarray(cb.scale_ref(np.hstack([X, Y]), True, True)[0], dtype=np.float64)
    for f in range(K):
        ho = Z[labels == f]
        for name, (W, C, B) in cb.stream_triples(Z, labels, f, p, k).items():
            sse, mag = cb.sse_quadratic(refs[f], p, W, C, B)
            direct = cb.sse_direct(ho[:, :p], ho[:, p:], W, C, B)
            bar = cb.sse_bar(mag, ho.shape[0], p, q, k, cb.K_SSE)
            print(f"fold {f} {name}: err / bar {np.max(np.abs(sse - direct) / bar):.3g}, mag / sse {np.max(mag / sse):.3g}")
            assert np.all(np.abs(sse - direct) <= bar) and np.all(mag >= np.abs(sse))


# ------------------------------------------------------------------------------ 4. launch geometry
def test_grid_helpers_are_the_librarys():
    from ppls_amd import _lib
    lib = _lib.lib()
    lib.ppls_cv_rows_per_wave.restype, lib.ppls_cv_rows_per_wave.argtypes = ct.c_int, [ct.c_int]
    lib.ppls_cv_grid.restype, lib.ppls_cv_grid.argtypes = ct.c_int, [ct.c_int64, ct.c_int, ct.c_int]
    for k in range(1, 17):
        assert cb.rows_per_wave(k) == lib.ppls_cv_rows_per_wave(k)
        for cus in (0, 1, 2, 64, 256, 304):
            for n in (0, 1, 7, 8, 9, 31, 32, 33, 2048, 2083, 4096, 16403, 32803, 70001, 10 ** 7, 2 ** 33 + 5):
                assert cb.cv_grid(n, k, cus) == lib.ppls_cv_grid(n, k, cus), (n, k, cus)
    assert cb.wide_rows(8, 256) == (2083, 32803) and cb.wide_rows(16, 256) == (1043, 16403)
    assert cb.n_sum(67, 19, 3, False, 3) == 1 + 16 + 1 + 6 + 1 + 256
    assert cb.n_sum(70, 259, 16, True, 5) == 1 + 16 + 2 + 6 + 1 + 256
    assert cb.n_sum(32803, 9, 8, False, 1024) == 1 + 16 + 2 + 6 + 16 + 256
