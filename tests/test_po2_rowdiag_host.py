"""The algebra, the bars and the host model of the PO2PLS row diagnostics (tests/po2_rowdiag_bar.py), and the
t-model loop on the contaminated recovery problem, all on the CPU."""
import numpy as np
import pytest

import po2_bar
import po2_rowdiag_bar as prb
import rowdiag_bar

L = prb.L
CASES = prb.cases()
SMALL = [c for c in CASES if c[1] + c[2] <= prb.DENSE_MAX]


@pytest.mark.parametrize("case", SMALL, ids=prb.case_id)
def test_closed_form_is_the_dense_form(case):
    """d2, loglik and mu by QR and Sigma_c agree with the dense (p+q) x (p+q) inverse in long double."""
    X, Y, th = prb.make_case(*case)
    ref, den = prb.reference(X, Y, th), prb.dense_reference(X, Y, th)
    kC = np.linalg.cond(np.asarray(ref["Sc"], dtype=np.float64))
    tol = float(np.finfo(L).eps) * 64 * (X.shape[1] + Y.shape[1]) * kC
    for key in ("d2", "loglik", "mu"):
        scale = np.maximum(np.abs(den[key]), 1)
        assert float(np.max(np.abs(ref[key] - den[key]) / scale)) <= tol, key


@pytest.mark.parametrize("case", [c for c in SMALL if c[0] >= 33], ids=prb.case_id)
def test_loglik_sums_to_the_s_form(case):
    """sum_i loglik_i = po2_bar.dense_loglik on S = Z'Z."""
    X, Y, th = prb.make_case(*case)
    ref = prb.reference(X, Y, th)
    Z = np.hstack([X, Y]).astype(L)
    want = po2_bar.dense_loglik(th, Z.T @ Z, X.shape[0])
    assert abs(ref["loglik"].sum() - want) <= float(np.finfo(L).eps) * 1e4 * abs(want)


@pytest.mark.parametrize("shape", rowdiag_bar.SHAPES[:5], ids=str)
def test_shared_only_is_section_23(shape):
    """rx = ry = 0 with orthonormal W, C: the closed form is rowdiag_bar.reference's."""
    n, p, q = shape
    r = min(3, p, q)
    X, Y, th = rowdiag_bar.make_case(n, p, q, r)
    W, C, b, t, sE, sF, sH = rowdiag_bar.theta_parts(th)
    th2 = dict(W=W, Wo=W[:, :0], C=C, Co=C[:, :0], B=b, sigT=t, sigTo=np.zeros(0), sigUo=np.zeros(0), sigE=sE, sigF=sF, sigH=sH)
    a, b23 = prb.reference(X, Y, th2), rowdiag_bar.reference(X, Y, th)
    for key in ("odx2", "ody2", "sd2", "d2", "loglik"):
        # the fp64 W is orthonormal to rounding only: Q of its QR differs from it by that much
        assert np.allclose(np.asarray(a[key], dtype=np.float64), np.asarray(b23[key], dtype=np.float64), rtol=1e-12, atol=1e-12), key
    mu23 = np.hstack([b23["mu_T"], b23["mu_U"]])
    assert np.allclose(np.asarray(a["mu"], dtype=np.float64), np.asarray(mu23, dtype=np.float64), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=prb.case_id)
def test_host_model_inside_every_bar(case, f32):
    X, Y, th = prb.make_case(*case)
    ref = prb.reference(X, Y, th, f32)
    br = prb.bars(X, Y, th, f32, ref)
    got = prb.host_model(X, Y, th, f32)
    for key in prb.OUTPUTS:
        ok, worst = prb.inside(got[key], ref[key], br[key])
        assert ok, (key, worst)
        assert np.all(br[key] <= 1e-6 * (1 + np.abs(np.asarray(ref[key], dtype=np.float64)))), key   # the bars are not loose


DEFECTS = [("gram_forgotten", (37, 41, 37, 2, 2, 1, False), "odx2", None),
           ("coupling_sign", (37, 41, 37, 2, 2, 1, True), "sd2", None),
           ("y_offset", (37, 41, 37, 2, 2, 1, True), "sd2", None),
           ("drop_unit", (37, 41, 37, 2, 2, 1, True), "odx2", None),
           # the cancellation loses about u ||x||^2; the bar's host-QR term, 4 eps ||e|| ||x|| with eps growing as
           # p kx^1.5, reaches that at p = 41: the narrow shape is where the a-priori bar can tell the two apart
           ("expand_x", (3, 5, 3, 1, 1, 0, True), "odx2", 1e-4)]


@pytest.mark.parametrize("defect,case,key,sigE", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_seeded_defects_fall_outside(defect, case, key, sigE):
    X, Y, th = prb.make_case(*case, sigE=sigE)
    ref = prb.reference(X, Y, th)
    br = prb.bars(X, Y, th, False, ref)
    good, bad = prb.host_model(X, Y, th), prb.host_model(X, Y, th, defect=defect)
    assert prb.inside(good[key], ref[key], br[key])[0]
    assert not prb.inside(bad[key], ref[key], br[key])[0]
    assert not prb.inside(bad["d2"], ref["d2"], br["d2"])[0]


@pytest.mark.parametrize("seed", po2_bar.HOST_SEEDS)
def test_t_model_loop_recovers_the_contaminated_problem(seed):
    """16 of 400 rows replaced by 4 N(0, 1): the Gaussian PO2PLS fit loses W, the t-model loop does not."""
    X, Y, tr, bad = prb.contaminated(seed)
    s = po2_bar.HOST_SHAPE
    Z = np.hstack([X, Y])
    th = po2_bar.cast(tr, np.float64)
    S = Z.T @ Z
    for _ in range(200):
        th = po2_bar.ecm_update(th, po2_bar.sform(th, S, s["N"], s["p"], s["q"], np.float64), s["p"], np.float64)
    dist_gauss = po2_bar.projector_distance(th["W"], tr["W"])
    rob, w = prb.robust_loop(X, Y, th, 4.0, 30, 5)
    dist_rob = po2_bar.projector_distance(rob["W"], tr["W"])
    good = np.setdiff1d(np.arange(s["N"]), bad)
    print(f"seed {seed}: gaussian {dist_gauss:.3f}, robust {dist_rob:.3f}, sigE {float(rob['sigE']):.4f}, "
          f"max planted weight {w[bad].max():.3f}, median other {np.median(w[good]):.3f}")
    assert dist_gauss >= 0.9
    assert dist_rob <= 0.35
    assert 0.45 <= float(rob["sigE"]) <= 0.55
    assert np.all(w[bad] <= 0.1)
    assert 0.9 <= np.median(w[good]) <= 1.1
