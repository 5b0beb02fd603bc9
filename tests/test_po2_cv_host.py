"""PO2PLS prediction and the choice of (r, rx, ry) on the host (no GPU): the prediction map
against the dense conditional mean in long double within a priori bars (tests/po2_cv_bar.py), its reduction
to predict_PPLS's map, the grid selection rule, and the cross-validated error's answer on the recovery
problem of tests/po2_bar.py."""
import numpy as np
import pytest

import po2_bar as B
import po2_cv_bar as CV
from sweep_bar import LD

SHAPES = [(13, 9, 2, 2, 1), (13, 9, 2, 0, 0), (37, 21, 8, 8, 3)]   # p, q, r, rx, ry


def _theta(p, q, r, rx, ry, orthonormal):
    return B.make_theta(np.random.default_rng(100 * p + 10 * r + rx + int(orthonormal)), p, q, r, rx, ry, orthonormal, scale=2.0)


def _ratio(got, ref, bar):
    return float(CV._fro(np.asarray(got).astype(LD) - ref) / bar)


@pytest.mark.parametrize("orthonormal", [True, False])
@pytest.mark.parametrize("p,q,r,rx,ry", SHAPES)
@pytest.mark.parametrize("xory", [0, 1])
def test_predict_map_against_the_dense_conditional_mean(p, q, r, rx, ry, orthonormal, xory):
    """L within bar_L = (8 k^2 u kappa_2(Lambda) ||G||_F ||X||_F + gamma_k || |G| |X| ||_F) / sigma^2 x SLACK of the
    long-double formula, and the composed map within bar_A of the dense Sigma_yx Sigma_xx^-1 (po2_cv_bar's
    docstring has every constant).  Plain fp64 numpy of the same formula lies inside the same bars."""
    from ppls_amd import po2_predict_map
    th = _theta(p, q, r, rx, ry, orthonormal)
    L, Bp = po2_predict_map(th, "XY"[xory])
    Lref, bar_L = CV.map_bar(th, xory)
    A_ref, bar_A = CV.dense_conditional(th, xory), CV.composed_bar(th, xory)
    L64, Bp64, _, _ = CV.predict_map(th, xory, np.float64)
    got = dict(L=_ratio(L, Lref, bar_L), A=_ratio(CV.composed(th, xory, L, Bp), A_ref, bar_A),
               L_numpy=_ratio(L64, Lref, bar_L), A_numpy=_ratio(CV.composed(th, xory, L64, Bp64), A_ref, bar_A))
    print(f"p={p} q={q} ({r},{rx},{ry}) orthonormal={orthonormal} xory={xory}: err / bar {got}")
    assert L.shape == ((q if xory else p), r) and Bp.shape == (r,)
    assert max(got.values()) <= 1.0, got
    if xory == 0:
        assert np.array_equal(Bp, th["B"])


@pytest.mark.parametrize("orthonormal", [True, False])
@pytest.mark.parametrize("p,q,r,rx,ry", SHAPES)
def test_predict_map_bar_rejects_seeded_defects(p, q, r, rx, ry, orthonormal):
    """Wo left out of Lambda_x, the joint Sigma_z^-1 block instead of the X-marginal one, and 1 / sigE^2 forgotten:
    each lies outside bar_L and outside bar_A.  Leaving Wo out is a defect only with rx > 0 and W'Wo != 0: with
    orthonormal [W Wo] Lambda_x is block diagonal and its first r columns do not see Wo at all."""
    th = _theta(p, q, r, rx, ry, orthonormal)
    Lref, bar_L = CV.map_bar(th, 0)
    A_ref, bar_A = CV.dense_conditional(th, 0), CV.composed_bar(th, 0)
    for defect in ("no_specific", "joint", "no_scale"):
        if defect == "no_specific" and (rx == 0 or orthonormal):
            continue
        Ld, Bd, _, _ = CV.predict_map(th, 0, np.float64, defect)
        rl, ra = _ratio(Ld, Lref, bar_L), _ratio(CV.composed(th, 0, Ld, Bd), A_ref, bar_A)
        print(f"({r},{rx},{ry}) orthonormal={orthonormal} {defect}: err / bar L {rl:.3g} A {ra:.3g}")
        assert rl > 1.0 and ra > 1.0, (defect, rl, ra)


def test_predict_map_without_specific_parts_is_predict_ppls_shrunk():
    """rx = ry = 0 with orthonormal W: L = W diag(sigT^2 / (sigT^2 + sigE^2)), so the prediction is
    predict_PPLS's x W diag(B) C' with every component shrunk by that factor."""
    from ppls_amd import po2_predict_map
    th = _theta(13, 9, 2, 0, 0, True)
    L, Bp = po2_predict_map(th, "X")
    t = B.cast(th, LD)
    want = t["W"] * (t["sigT"] ** 2 / (t["sigT"] ** 2 + t["sigE"] ** 2))
    _, bar_L = CV.map_bar(th, 0)
    assert _ratio(L, want, bar_L) <= 1.0
    ppls = (t["C"] * t["B"]) @ t["W"].T
    shrunk = (t["C"] * (t["B"] * t["sigT"] ** 2 / (t["sigT"] ** 2 + t["sigE"] ** 2))) @ t["W"].T
    assert _ratio(CV.composed(th, 0, L, Bp), shrunk, CV.composed_bar(th, 0)) <= 1.0
    assert CV._fro(shrunk - ppls) > 0.05 * CV._fro(ppls)        # the factor is no rounding matter here


def test_predict_map_refusals():
    from ppls_amd import PplsError, po2_predict_map
    th = _theta(13, 9, 2, 2, 1, True)
    for bad in (dict(th, sigE=-1.0), dict(th, sigTo=np.array([1.0, np.nan])), B.make_theta(np.random.default_rng(0), 13, 9, 2, 12, 1, orthonormal=False)):
        with pytest.raises(PplsError) as ei:
            po2_predict_map(bad, "X")
        assert ei.value.code == -1
    with pytest.raises(PplsError) as ei:                         # 1 / beta does not exist
        po2_predict_map(dict(th, B=np.array([1.0, 0.0])), "Y")
    assert ei.value.code == -3
    with pytest.raises(PplsError) as ei:                         # Lambda not positive definite: its Gram overflows
        po2_predict_map(dict(th, W=th["W"] * 1e160), "X")
    assert ei.value.code == -3
    with pytest.raises(ValueError):
        po2_predict_map(th, "Z")


def test_grid_selection_rule():
    from ppls_amd.po2 import GRID_TIE, select_grid_PO2PLS
    K, shape = 3, (2, 2, 2)
    base = np.full((K,) + shape, 1.0)
    none = np.zeros((K,) + shape, dtype=bool)
    # a plain minimum
    pf = base.copy()
    pf[:, 1, 0, 1] = [0.5, 0.6, 0.7]
    err, which = select_grid_PO2PLS(pf, none)
    assert which == (1, 0, 1) and err[1, 0, 1] == np.mean([0.5, 0.6, 0.7]) and err[0, 0, 0] == 1.0
    # an exact tie, and a cell within rounding of it, go to the first cell in grid order
    pf = base.copy()
    pf[:, 0, 1, 0] = 0.5
    pf[:, 1, 1, 1] = 0.5
    assert select_grid_PO2PLS(pf, none)[1] == (0, 1, 0)
    pf[:, 0, 1, 0] = 0.5 * (1 + GRID_TIE / 4)                   # the later cell is lower by less than the tie width
    assert select_grid_PO2PLS(pf, none)[1] == (0, 1, 0)
    pf[:, 0, 1, 0] = 0.5 * (1 + 1e-9)                           # a real difference is respected
    assert select_grid_PO2PLS(pf, none)[1] == (1, 1, 1)
    # a cell with one failed fold is NaN and never wins while a finite cell exists
    pf = base.copy()
    pf[:, 0, 0, 1] = 0.1
    failed = none.copy()
    failed[2, 0, 0, 1] = True
    pf[:, 1, 0, 0] = [0.9, np.nan, 0.9]                         # a NaN error counts as failed too
    err, which = select_grid_PO2PLS(pf, failed)
    assert np.isnan(err[0, 0, 1]) and np.isnan(err[1, 0, 0]) and which == (0, 0, 0) and np.isfinite(err[0, 0, 0])
    # all cells NaN
    err, which = select_grid_PO2PLS(pf, np.ones((K,) + shape, dtype=bool))
    assert which is None and np.all(np.isnan(err))
    with pytest.raises(ValueError):
        select_grid_PO2PLS(pf[0], failed[0])


def test_cross_validated_error_prefers_the_true_sizes_to_the_shared_only_model():
    """The host loop on seed 0 of the recovery problem (N = 400, p = 13, q = 9, truth (2, 2, 1)), folds i % 4,
    fp64 po2_bar.em_loop from start_theta(seed=7), 200 steps, atol 1e-4: mean RMSEP at (2, 2, 1) below 0.95 x
    that at (2, 0, 0).  Measured ratios 0.924, 0.919, 0.808 on seeds 0, 1, 2; 0.95 leaves room for another start
    without letting the shared-only model pass."""
    X, Y, _ = B.host_problem(0)
    labels = np.arange(X.shape[0]) % 4
    full = CV.host_cv(X, Y, labels, 2, 2, 1).mean()
    shared = CV.host_cv(X, Y, labels, 2, 0, 0).mean()
    print(f"mean RMSEP (2,2,1) {full:.4f}  (2,0,0) {shared:.4f}  ratio {full / shared:.3f}")
    assert full < 0.95 * shared
