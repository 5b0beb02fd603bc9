"""Host side of the robust fit: no GPU.

The bars of tests/robust_bar.py are shown to admit a plain fp64 evaluation in the kernels' order and to reject
seeded defects: for the real-weighted Gram the weight on both operands, the weights shifted by one row and the
weight truncated to an integer; for the sum of log1p(d2 / nu) the plain log of d2 / nu; for the loop the divisor
sum u in place of N, seen as a different fit.  l_t is checked against a dense evaluation on the oracle's
covariance, and the loop written out with the oracle's Expect_M and Maximiz_M reproduces what the robust fit is
for: on contaminated rows it recovers the loading spaces the Gaussian fit loses, and l_t never decreases.
"""
import numpy as np
import pytest

import robust_bar as rob
import rowdiag_bar as rb
from robust_bar import K_W, gram_inside, kernel_order, weighted_ref

SHAPES = [(1, 3, 2), (5, 3, 2), (27, 5, 3), (257, 13, 3), (64, 7, 6)]
NU = 4.0


def _rows(n, P, seed=0):
    rng = np.random.default_rng(100 * n + P + seed)
    j = np.arange(P)
    return rng.standard_normal((n, P)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7


@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("n,p,q", SHAPES)
def test_weighted_gram_kernel_order_lies_inside_the_bar(n, p, q, nsplit):
    D = _rows(n, p + q)
    w = rob.draw_weights(n, p + q, NU, seed=nsplit)
    ok, worst = gram_inside(kernel_order(D, w, nsplit), weighted_ref(D, w), n)
    print(f"n={n} P={p + q} nsplit={nsplit}: max err / bar {worst:.3g} (K_W = {K_W})")
    assert ok


@pytest.mark.parametrize("n,p,q", [s for s in SHAPES if s[0] > 1])
def test_weighted_gram_defects_lie_outside_the_bar(n, p, q):
    D = _rows(n, p + q)
    w = rob.draw_weights(n, p + q, NU, seed=n)
    w[0], w[1] = 2.75, 0.25            # (so that w^2 != w, a shift moves something and truncation drops something)
    ref = weighted_ref(D, w)
    assert gram_inside(kernel_order(D, w, 2), ref, n)[0]
    assert not gram_inside(kernel_order(D, w, 2, both=True), ref, n)[0]       # weight on both operands
    assert not gram_inside(kernel_order(D, np.roll(w, 1), 2), ref, n)[0]      # weights shifted by one row
    assert not gram_inside(kernel_order(D, np.trunc(w), 2), ref, n)[0]        # weight truncated to an integer


def test_unit_and_integer_weights_are_the_other_kernels_sums():
    D = _rows(27, 8)
    assert np.array_equal(kernel_order(D, np.ones(27), 3), kernel_order(D, np.ones(27, dtype=np.int32), 3))
    c = np.arange(27) % 4
    assert np.array_equal(kernel_order(D, c.astype(np.float64), 3), kernel_order(D, c.astype(np.int32), 3))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("n,p,q,r", [(300, 12, 9, 2), (70, 130, 5, 3), (2500, 5, 3, 2)])
def test_weights_and_sums_in_kernel_order_lie_inside_the_bars(n, p, q, r, f32):
    X, Y, th = rb.make_case(n, p, q, r, seed=3)
    nus = rob.nu_grid(1.0, 1000.0)
    hm = rb.host_model(X, Y, th, f32, want_mu=False)
    got = rob.host_model(hm["odx2"], hm["ody2"], hm["sd2"], th, nus, 5, p + q)
    assert np.array_equal(got["d2"], hm["d2"])                  # the bits the diagnostics report
    ref, bar = rob.reference(X, Y, th, nus, 5, f32), rob.bars(X, Y, th, nus, 5, f32)
    ok_w, worst_w = rob.inside(got["w"], ref["w"], bar["w"])
    ok_s, worst_s = rob.inside(got["sums"], ref["sums"], bar["sums"])
    ll = rob.loglik_t_from(got["sums"], th, nus, p, q, n)
    ok_l, worst_l = rob.inside(ll, ref["loglik_t"], bar["loglik_t"])
    print(f"n={n} p={p} q={q} r={r} f32={f32}: err / bar  w {worst_w:.3g}  sums {worst_s:.3g}  l_t {worst_l:.3g}")
    assert ok_w and ok_s and ok_l
    # the seeded defect: log(d2 / nu) in place of log1p(d2 / nu)
    bad = rob.host_model(hm["odx2"], hm["ody2"], hm["sd2"], th, nus, 5, p + q, defect="log")
    assert not rob.inside(bad["sums"], ref["sums"], bar["sums"])[0]
    # and a weight taken for another nu of the list
    other = rob.host_model(hm["odx2"], hm["ody2"], hm["sd2"], th, nus, 6, p + q)
    assert not rob.inside(other["w"], ref["w"], bar["w"])[0]


def test_sum_order_depends_on_n_alone():
    t = np.random.default_rng(1).chisquare(3, 5000)
    assert rob.model_sum(t) == rob.model_sum(t.copy())
    assert abs(rob.model_sum(t) - float(np.sum(t.astype(np.longdouble)))) <= rob.gamma(rob.depth(5000)) * t.sum()


def test_loglik_t_against_the_dense_covariance():
    n, p, q, r = 40, 6, 5, 2
    X, Y, th = rb.make_case(n, p, q, r, seed=1)
    for nu in (1.5, 4.0, 30.0):
        ref = rob.reference(X, Y, th, [nu])
        dense = rob.dense_loglik_t(X, Y, th, nu)
        print(f"nu={nu}: l_t {float(ref['loglik_t'][0]):.12g}  dense {dense:.12g}")
        assert abs(float(ref["loglik_t"][0]) - dense) <= 1e-10 * abs(dense)
        d2, logdet = rob.dense_d2_logdet(X, Y, th)
        assert np.abs(d2 - np.asarray(ref["d2"], dtype=np.float64)).max() <= 1e-10 * d2.max()
        assert abs(logdet - float(rob.logdet_parts(th, p, q)[0])) <= 1e-10 * abs(logdet)


@pytest.fixture(scope="module")
def loops():
    """The Gaussian fit (60 EM steps) and the nu = 4 loop on the three contaminated problems, computed once."""
    out = {}
    for seed in (1, 2, 3):
        X, Y, th0, Wt, Ct = rob.contaminated(seed)
        g = rob.em_steps(X, Y, dict(th0), 60)
        out[seed] = (X, Y, g, rob.oracle_loop(X, Y, dict(g), NU, outer=40, inner=5, atol=-np.inf), Wt, Ct)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_loop_recovers_what_the_gaussian_fit_loses(loops, seed):
    X, Y, g, fit, Wt, Ct = loops[seed]
    th = fit["theta"]
    ew_g, ew_r = rob.space_error(g["W"], Wt), rob.space_error(th["W"], Wt)
    ec_g, ec_r = rob.space_error(g["C"], Ct), rob.space_error(th["C"], Ct)
    inc = np.diff(fit["loglik"])
    print(f"seed {seed}: W error Gaussian {ew_g:.3f} robust {ew_r:.3f}; C error {ec_g:.3f} / {ec_r:.3f}; sigE "
          f"{float(g['sigE']):.3f} / {float(th['sigE']):.3f}; least l_t increment {inc.min():.3e}")
    assert ew_r <= 0.3 and ew_g >= 1.0
    assert ec_r < ec_g
    assert np.all(inc >= 0)
    assert abs(float(th["sigE"]) - 0.5) < 0.05 < abs(float(g["sigE"]) - 0.5)


def test_loop_with_estimated_nu_never_decreases(loops):
    X, Y, g, _, Wt, _ = loops[1]
    fit = rob.oracle_loop(X, Y, dict(g), "estimate", outer=15, inner=5, atol=-np.inf)
    print(f"nu = {fit['nu']:.3f}, W error {rob.space_error(fit['theta']['W'], Wt):.3f}")
    assert np.all(np.diff(fit["loglik"]) >= 0)
    assert 1.0 <= fit["nu"] <= 1000.0


def test_divisor_sum_u_is_a_different_fit(loops):
    X, Y, g, _, _, _ = loops[1]
    a = rob.oracle_loop(X, Y, dict(g), NU, outer=1, inner=5, atol=-np.inf)
    b = rob.oracle_loop(X, Y, dict(g), NU, outer=1, inner=5, atol=-np.inf, divisor="sum_u")
    N, su = X.shape[0], a["weights"].sum()
    rel = abs(float(b["theta"]["sigE"]) - float(a["theta"]["sigE"])) / float(a["theta"]["sigE"])
    print(f"sum u / N = {su / N:.4f}; sigE after one outer iteration: {float(a['theta']['sigE']):.6f} (N) "
          f"{float(b['theta']['sigE']):.6f} (sum u), relative difference {rel:.3e}")
    # S_u / sum u = (N / sum u) S_u / N: every variance moves by that factor, far above any rounding
    assert abs(su / N - 1.0) > 1e-3
    assert rel > 1e-4


def test_loop_stops_on_atol_and_counts_steps(loops):
    X, Y, g, _, _, _ = loops[2]
    fit = rob.oracle_loop(X, Y, dict(g), NU, outer=50, inner=5, atol=1e-2)   # (EM's linear rate: 1e-4 takes > 50)
    assert fit["converged"] and 1 <= fit["steps"] < 50 and len(fit["loglik"]) == fit["steps"] + 1
    assert fit["loglik"][-1] - fit["loglik"][-2] < 1e-2 <= fit["loglik"][-2] - fit["loglik"][-3]
    cap = rob.oracle_loop(X, Y, dict(g), NU, outer=2, inner=5, atol=1e-2)
    assert not cap["converged"] and cap["steps"] == 2 and len(cap["loglik"]) == 3


def test_entry_points_are_declared():
    import os
    from conftest import ROOT
    import ppls_amd
    from ppls_amd import _lib
    with open(os.path.join(ROOT, "include", "ppls.h")) as f:
        h = f.read()
    for decl in ("int ppls_robust_weights(ppls_ctx* ctx, const ppls_theta* th, int r, const double* nu, int m, int keep,",
                 "int ppls_robust_get(ppls_ctx* ctx, double* w, double* d2);",
                 "int ppls_xprod_weighted(ppls_ctx* dst, ppls_ctx* src, const double* weight"):
        assert decl in h
    with open(os.path.join(ROOT, "include", "ppls_debug.h")) as f:
        dbg = f.read()
    assert "int ppls_gram_weighted_real(" in dbg and "int ppls_gram_occupancy_real(int f32);" in dbg
    for name in ("ppls_robust_weights", "ppls_robust_get", "ppls_xprod_weighted", "ppls_gram_weighted_real",
                 "ppls_gram_occupancy_real"):
        assert name in _lib.SIGNATURES
    assert callable(ppls_amd.robust_PPLS_simult)
    with pytest.raises(ValueError):
        ppls_amd.robust_PPLS_simult(None, None, 2, nu=-1.0)
    with pytest.raises(ValueError):
        ppls_amd.robust_PPLS_simult(None, None, 2, nu="auto")
