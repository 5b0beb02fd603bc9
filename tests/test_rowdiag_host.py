"""Row diagnostics without a GPU: the host model of the kernel lies inside the a-priori bars of
tests/rowdiag_bar.py on every shape of the GPU test, four seeded defects fall outside them, the closed form
agrees with the dense covariance of the oracle, and the p-value / flag logic on hand-made distances."""
import numpy as np
import pytest

import rowdiag_bar as rb
from oracle import ppls_oracle as o


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", rb.cases(), ids=lambda s: "n%d_p%d_q%d_r%d" % s)
def test_host_model_inside_bars(shape, f32):
    X, Y, th = rb.make_case(*shape)
    ref, bar, got = rb.reference(X, Y, th, f32), rb.bars(X, Y, th, f32), rb.host_model(X, Y, th, f32)
    for key in rb.OUTPUTS:
        ok, ratio = rb.inside(got[key], ref[key], bar[key])
        print(f"{key}: error / bar = {ratio:.3g}")
        assert ok, (key, ratio)
        assert np.all(bar[key] <= 1e-9 * (1 + np.abs(np.asarray(ref[key], dtype=np.float64)))), key   # a bar, not a blanket


def _outside(X, Y, th, f32, defect):
    ref, bar, got = rb.reference(X, Y, th, f32), rb.bars(X, Y, th, f32), rb.host_model(X, Y, th, f32, defect=defect)
    return [key for key in rb.OUTPUTS if not rb.inside(got[key], ref[key], bar[key])[0]]


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_seeded_defects_fall_outside(f32):
    X, Y, th = rb.make_case(37, 41, 37, 5)
    assert _outside(X, Y, th, f32, None) == []
    bad = _outside(X, Y, th, f32, "drop_unit")           # 41 and 37 columns: a partial last unit in either dtype
    assert "odx2" in bad and "ody2" in bad, bad
    Xg, Yg, thg = rb.make_case(39, 41, 37, 9)            # 39 rows, 4 per group at r = 9: rows 37, 38 take row 36
    assert _outside(Xg, Yg, thg, f32, None) == []
    bad = _outside(Xg, Yg, thg, f32, "group_first")
    assert set(bad) == set(rb.OUTPUTS), bad
    bad = _outside(X, Y, th, f32, "s12_sign")
    assert "sd2" in bad and "d2" in bad and "loglik" in bad and "odx2" not in bad, bad
    Xs, Ys, ths = rb.make_case(37, 41, 37, 5, sigE=1e-4)   # a good fit: ||x||^2 - ||a||^2 cancels
    assert _outside(Xs, Ys, ths, f32, None) == []
    bad = _outside(Xs, Ys, ths, f32, "expand_x")
    assert "odx2" in bad, bad


def test_group_first_defect_needs_a_partial_group():
    assert rb.rows_per_wave(5, 41, 37, False) == 2 and rb.rows_per_wave(9, 41, 37, False) == 4
    assert rb.rows_per_wave(1, 2051, 3, False) == 4 and rb.rows_per_wave(1, 2051, 3, True) == 2
    assert rb.rows_per_wave(1, 4101, 3, True) == 4
    X, Y, th = rb.make_case(33, 261, 130, 16)            # 4 rows per group at r = 16: row 32 is alone, and first
    assert _outside(X, Y, th, False, "group_first") == []
    X, Y, th = rb.make_case(6, 2051, 3, 1)               # long rows: 4 per group, row 5 takes row 4
    assert "odx2" in _outside(X, Y, th, False, "group_first")
    X, Y, th = rb.make_case(67, 131, 9, 9)               # rows 64 .. 66; q = r: ody2 is rounding noise in every row
    assert set(_outside(X, Y, th, False, "group_first")) >= set(rb.OUTPUTS) - {"ody2"}


def test_closed_form_against_the_dense_covariance():
    n, p, q, r = 40, 13, 7, 3
    X, Y, th = rb.make_case(n, p, q, r, seed=3)
    S = o.sse_xy_w(th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])
    Z = np.hstack([X, Y])
    d2_dense = np.einsum("ij,ij->i", Z, np.linalg.solve(S, Z.T).T)
    got = rb.host_model(X, Y, th)
    cond = np.linalg.cond(S)
    # solve() is backward stable: the quadratic form is off by at most ~ (p + q) cond u relative; 8 for the
    # closed form's own stages and the orthonormality of a QR's Q (both a few u)
    bar = 8 * (p + q) * cond * np.finfo(np.float64).eps * np.abs(d2_dense)
    err = np.abs(got["d2"] - d2_dense)
    print("d2 relative difference", float((err / d2_dense).max()), "bar", float((bar / d2_dense).max()))
    assert np.all(err <= bar)
    ll = o.logl_w(X, Y, th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])
    total = float(got["loglik"].sum())
    bar_ll = 8 * (p + q) * cond * np.finfo(np.float64).eps * float(np.abs(got["loglik"]).sum())
    print("loglik", total, float(ll), "bar", bar_ll)
    assert abs(total - float(ll)) <= bar_ll
    # and the dense log-density itself, term by term
    _, logdet = np.linalg.slogdet(S)
    ll_dense = -0.5 * ((p + q) * np.log(2 * np.pi) + logdet + d2_dense)
    assert np.all(np.abs(got["loglik"] - ll_dense) <= 8 * (p + q) * cond * np.finfo(np.float64).eps * np.abs(ll_dense))


def test_pvalues_flags_and_df():
    from ppls_amd.api import chisq_upper, diagnostics_df, diagnostics_summary
    import scipy.stats
    p, q, r = 12, 7, 3
    assert diagnostics_df(p, q, r) == dict(odx2=9, ody2=4, sd2=6, d2=19)
    sE, sF = 0.5, 2.0
    stat = dict(odx2=np.array([9.0, 40.0, 0.0, 9.0, 2000.0]), ody2=np.array([4.0, 3.0, 30.0, 4.0, 1e5]),
                sd2=np.array([6.0, 5.0, 7.0, 45.0, 3e4]))
    res = dict(odx2=stat["odx2"] * sE * sE, ody2=stat["ody2"] * sF * sF, sd2=stat["sd2"])
    res["d2"] = stat["odx2"] + stat["ody2"] + stat["sd2"]
    s = diagnostics_summary(res, p, q, r, sE, sF, alpha=0.01)
    for key, df in s["df"].items():
        x = res["d2"] if key == "d2" else stat[key]
        want = scipy.stats.chi2.sf(x, df)
        assert np.allclose(s["pvalue"][key], want, rtol=1e-12, atol=0), key
        assert np.all(np.isfinite(s["pvalue"][key])) and np.array_equal(s["flag"][key], want < 0.01)
    assert s["pvalue"]["odx2"][2] == 1.0 and s["pvalue"]["d2"][4] == 0.0        # 0 and far beyond: 1 and 0, never NaN
    assert list(s["flag"]["odx2"]) == [False, True, False, False, True]
    assert list(s["flag"]["ody2"]) == [False, False, True, False, True]
    assert list(s["flag"]["sd2"]) == [False, False, False, True, True]
    assert list(s["outliers"]) == list(np.flatnonzero(s["flag"]["d2"])[np.argsort(s["pvalue"]["d2"][s["flag"]["d2"]])])
    assert s["outliers"][0] == 4
    # Bonferroni: alpha / n with n the rows of the call
    x = np.array([scipy.stats.chi2.isf(0.01 / 4, 19), scipy.stats.chi2.isf(0.01 / 6, 19), 1.0, 2.0, 3.0])
    res_b = dict(odx2=np.zeros(5), ody2=np.zeros(5), sd2=np.zeros(5), d2=x)
    assert list(diagnostics_summary(res_b, p, q, r, sE, sF, alpha=0.01)["flag"]["d2"]) == [True, True, False, False, False]
    sb = diagnostics_summary(res_b, p, q, r, sE, sF, alpha=0.01, adjust="bonferroni")   # 0.01 / 5
    assert list(sb["flag"]["d2"]) == [False, True, False, False, False]
    assert np.all(chisq_upper(np.array([0.0, 5.0]), 0) == 1.0)                  # p = r: no degrees of freedom
    with pytest.raises(ValueError):
        diagnostics_summary(res_b, p, q, r, sE, sF, adjust="holm")
    empty = {k: np.zeros(0) for k in ("odx2", "ody2", "sd2", "d2")}
    assert diagnostics_summary(empty, p, q, r, sE, sF, adjust="bonferroni")["outliers"].shape == (0,)


def test_planted_outliers_in_the_reference():
    """The recipe of the GPU test holds for the reference alone (seed 20261020)."""
    from ppls_amd.api import diagnostics_summary
    X, Y, th, rows = rb.planted()
    ref = rb.reference(X, Y, th)
    s = diagnostics_summary({k: np.asarray(ref[k], dtype=np.float64) for k in ("odx2", "ody2", "sd2", "d2")},
                            37, 21, 3, th["sigE"], th["sigF"])
    for key, row in rows.items():
        pv = s["pvalue"][key]
        print(key, row, pv[row], np.delete(pv, row).min())
        assert int(np.argmin(pv)) == row and pv[row] < 1e-12 and np.delete(pv, row).min() > 1e-6
    assert set(s["outliers"][:3]) == {5, 77, 150}


def test_python_refusals_without_a_device():
    from ppls_amd import diagnostics_PPLS
    X, Y, th = rb.make_case(3, 5, 3, 1)
    seq = dict(W=th["W"], C=th["C"], B=np.array([1.0]), sig=np.ones((1, 4)))     # a sequential PPLS fit's shape
    with pytest.raises(ValueError, match="PPLS_simult"):
        diagnostics_PPLS(seq, X, Y)
    with pytest.raises(ValueError, match="adjust"):
        diagnostics_PPLS(dict(estimates=th), X, Y, adjust="fdr")
    with pytest.raises(ValueError, match="columns"):
        diagnostics_PPLS(dict(estimates=th), X[:, :4], Y)
    with pytest.raises(ValueError, match="columns"):
        diagnostics_PPLS(rb.theta_of(th), X, Y[:, :2], new=True)
