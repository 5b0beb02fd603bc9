"""meta_PPLSi from per-population cross-products, the parts that need no GPU: the error bar of
tests/meta_xprod_bar.py judged on plain fp64 numpy and on seeded defects, population_labels against
_populations, and the algebra itself -- the oracle's meta_EMstep on rows against the same step
computed from numpy cross-products."""
import numpy as np
import pytest

from conftest import make_problem
from meta_xprod_bar import MetaReference, emstep_from_xprod, mu_coefficients_fp64, pop_params, stats_fp64
from oracle import ppls_oracle as o
from sweep_bar import sweep_problem

SHAPES = [(1, 1), (3, 2), (9, 12), (127, 130)]


def _pop_matrices(p, q, K, seed):
    sizes = [2, 37, 11, 64, 36][:K - 1] + [150 - sum([2, 37, 11, 64, 36][:K - 1])]
    X, Y, th = sweep_problem(150, p, q, 1, seed)
    D = np.hstack([X, Y])
    ends = np.cumsum(sizes)
    return [D[e - s:e].T @ D[e - s:e] for s, e in zip(sizes, ends)], th["W"][:, 0], th["C"][:, 0]


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("p,q", SHAPES)
def test_bar_holds_for_fp64_and_catches_defects(p, q, K):
    S, w, c = _pop_matrices(p, q, K, seed=100 * p + q + K)
    coef = mu_coefficients_fp64(pop_params(K))
    ref = MetaReference(S, p, q, w, c, coef)
    good = ref.ratios(*stats_fp64(S, p, w, c, coef))
    print(f"({p},{q}) K={K}: fp64 numpy err / bar {good}")
    assert max(good.values()) <= 1.0
    # one dropped column: the largest |w_k| of X (Y where X has one column); SX, SY and G all move
    drop = int(np.argmax(np.abs(w))) if p > 1 else p + int(np.argmax(np.abs(c)))
    bad = ref.ratios(*stats_fp64(S, p, w, c, coef, drop=drop))
    assert bad["SX"] > 1.0 and bad["SY"] > 1.0 and bad["G"] > 1.0
    bad = ref.ratios(*stats_fp64(S, p, w, c, coef, swap=True))      # alpha_j <-> beta_j: SX alone
    assert bad["SX"] > 1.0 and bad["SY"] <= 1.0 and bad["G"] <= 1.0
    bad = ref.ratios(*stats_fp64(S, p, w, c, coef, pop0=True))      # population 0's scalars everywhere
    assert bad["SX"] > 1.0 and bad["SY"] > 1.0 and bad["G"] <= 1.0
    # and population 0 itself is untouched by that defect
    SX, SY, _ = stats_fp64(S, p, w, c, coef, pop0=True)
    assert MetaReference._ratio(SX[0], ref.SX[0], ref.bar_SX[0]) <= 1.0


def test_mu_coefficients_match_the_oracle():
    """EMstepC_fast's form of alpha .. delta (what the library stages) against the oracle's
    mu_coefficients (EM_W_multi.R:691-694) at the well-conditioned scalars the bar tests use."""
    P = pop_params(5)
    got = mu_coefficients_fp64(P)
    for j, (B, sX, sY, sH, sT) in enumerate(P):
        cf = o.mu_coefficients(np.array([B]), sX, sY, sH, np.array([sT]))
        want = np.array([cf[k][0] for k in ("alpha", "beta", "gamma", "delta")])
        assert np.all(np.abs(got[j] - want) <= 1e-14 * np.abs(want))


@pytest.mark.parametrize("Ipopu", [np.array(["b"] * 5 + ["a"] * 3 + ["c"] * 2), np.array([7, 3, 3, 9, 7, 3]),
                                   np.array([2.5, -1.0, 2.5, 0.0]), np.array(["x10", "x9", "x10", "x1"])],
                         ids=["strings", "integers", "unsorted_floats", "lexicographic"])
def test_population_labels_follow_populations(Ipopu):
    from ppls_amd.api import _populations, population_labels
    labels, levels = population_labels(Ipopu)
    lv, counts = _populations(Ipopu, len(Ipopu))
    assert labels.dtype == np.int32 and labels.shape == Ipopu.shape
    assert np.array_equal(levels, lv)
    assert np.array_equal(np.bincount(labels, minlength=len(lv)), counts)
    assert np.array_equal(levels[labels], Ipopu)
    with pytest.raises(ValueError):
        population_labels(np.zeros((2, 2)))


@pytest.mark.parametrize("sizes", [[300, 250, 200, 247], [3, 500, 2, 492], [40] * 5], ids=["K4", "tiny_pops", "K5"])
def test_emstep_from_cross_products_equals_the_oracle_on_rows(sizes):
    n, p, q = sum(sizes), 37, 29
    X, Y, _ = make_problem(n, p, q, 1, seed=n)
    init = o.initial_guess(p, q, "equal")
    params = [dict(B_T=1.0 + 0.1 * j, sigX=0.9 + 0.05 * j, sigY=0.8 + 0.02 * j, sigH=0.3 + 0.01 * j, sigT=1.1 - 0.05 * j)
              for j in range(len(sizes))]
    ref = o.meta_emstep(X, Y, init["W"], init["C"], sizes, params)
    D = np.hstack([X, Y])
    ends = np.cumsum(sizes)
    S = [D[e - s:e].T @ D[e - s:e] for s, e in zip(sizes, ends)]
    got = emstep_from_xprod(S, sizes, p, q, init["W"], init["C"], params)

    def rel(a, b):
        return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))
    assert rel(got["W"], ref["W"]) < 1e-12 and rel(got["C"], ref["C"]) < 1e-12
    for g, r in zip(got["pops"], ref["pops"]):
        assert rel(g["B"], r["B"]) < 1e-12
        assert rel(g["sighat"], r["sighat"]) < 1e-12 and rel(g["siglathat"], r["siglathat"]) < 1e-12
        assert rel(g["Cxt"], r["Cxt"]) < 1e-12 and rel(g["Cyu"], r["Cyu"]) < 1e-12
