"""PO2PLS on the host (no GPU): the algebra of tests/po2_bar.py against the dense restatement of the
reference's EMstepC / loglC and against the oracle's Expect_M, the bars against plain fp64 numpy and
against six seeded defects, the recovery the model is for, and the summary and canonical form."""
import numpy as np
import pytest

import po2_bar as B
from oracle import ppls_oracle as o
from sweep_bar import LD

MOMENTS = ("Cxt", "Cxto", "Cyu", "Cyuo", "Ctt", "Ctoto", "Ctto", "Cuu", "Cuouo", "Cuuo", "Cut", "Chh", "Cee", "Cff")


def _problem(p, q, r, rx, ry, orthonormal, seed, N=50):
    rng = np.random.default_rng(seed)
    th = B.make_theta(rng, p, q, r, rx, ry, orthonormal, scale=1.3)
    D = rng.standard_normal((N, p + q)) @ (np.eye(p + q) + 0.3 * rng.standard_normal((p + q, p + q)))
    return th, D, D.T @ D, N


@pytest.mark.parametrize("p,q,r,rx,ry,orthonormal", [(13, 9, 2, 2, 1, True), (13, 9, 2, 2, 1, False), (7, 5, 1, 0, 3, False),
                                                     (7, 5, 2, 3, 0, False), (6, 6, 3, 0, 0, False)])
def test_s_form_equals_the_dense_form_in_long_double(p, q, r, rx, ry, orthonormal):
    th, _, S, N = _problem(p, q, r, rx, ry, orthonormal, seed=p + r)
    dense, sf = B.dense_estep(th, S, N), B.sform(th, S, N, p, q)
    for k in MOMENTS:
        a, b = np.asarray(dense[k], dtype=LD), np.asarray(sf[k], dtype=LD)
        assert a.shape == b.shape, k
        if a.size:
            assert np.max(np.abs(a - b)) <= 1e-15 * max(np.max(np.abs(a)), 1e-300), k
    ll = B.dense_loglik(th, S, N)
    assert abs(ll - sf["loglik"]) <= 1e-15 * abs(ll)


def test_without_specific_parts_it_is_expect_m():
    """rx = ry = 0 at orthonormal loadings: the moments' diagonals, Cee, Cff, Chh and the
    log-likelihood are oracle.expect_m_dense's and logl_w's."""
    p, q, r = 11, 8, 3
    th, D, S, N = _problem(p, q, r, 0, 0, True, seed=4)
    X, Y = D[:, :p], D[:, p:]
    sf = B.sform(th, S, N, p, q)
    ref = o.expect_m_dense(X, Y, th["W"], th["C"], np.diag(th["B"]), th["sigE"], th["sigF"], th["sigH"], np.diag(th["sigT"]))
    f = lambda A: np.asarray(A, dtype=np.float64)
    for k in ("Ctt", "Cuu", "Cut"):
        assert np.allclose(np.diag(f(sf[k])), np.diag(ref[k]), rtol=1e-9, atol=0)
    assert np.allclose(np.abs(f(sf["Chh"])), ref["Chh"], rtol=1e-9, atol=1e-12)
    assert np.isclose(float(sf["Cee"]), ref["Cee"][0, 0], rtol=1e-9) and np.isclose(float(sf["Cff"]), ref["Cff"][0, 0], rtol=1e-9)
    ll = o.logl_w(X, Y, th["W"], th["C"], np.diag(th["B"]), th["sigE"], th["sigF"], th["sigH"], np.diag(th["sigT"]))
    assert np.isclose(float(sf["loglik"]), ll, rtol=1e-11)


def _all_ratios(th, S, N, p, q, defect=None):
    """err / bar of plain fp64 numpy (with an optional seeded defect) for every checked quantity."""
    r, rx, ry, kx, ky, k = B.shape(th)
    Gx, Gy = B.loadings(th)
    pr = B.PassReference(S, p, q, Gx, Gy)
    ref = B.sform(th, S, N, p, q)
    got = B.sform(th, S, N, p, q, np.float64, defect)
    ssqX, ssqY = float(np.trace(S[:p, :p])), float(np.trace(S[p:, p:]))
    bars = B.small_bars(ref, th, N, p, q, ssqX, ssqY, e_Q=np.sqrt(np.sum(pr.bar_Q ** 2)),
                        e_G=np.sqrt(np.sum(pr.bar_GGx ** 2) + np.sum(pr.bar_GGy ** 2)))
    out = pr.ratios(got["M"], got["Q"], got["GGx"], got["GGy"])
    out.update(B.small_ratios(got, ref, bars))
    thL = B.cast(th, LD)
    for side in (0, 1):
        raw_ref = B.raw_updates(thL, ref, p, side, 0)
        raw_got = B.raw_updates(B.cast(th, np.float64), got, p, side, 0, defect=defect)
        out[f"raw{side}"] = B.ratio(raw_got, raw_ref, B.raw_update_bar(ref, th, bars, pr.bar_M, N, p, side, 0))
        if (ry if side else rx):
            Wn = B.orth(raw_ref)
            ref2 = B.raw_updates(thL, ref, p, side, 1, Wn)
            got2 = B.raw_updates(B.cast(th, np.float64), got, p, side, 1, np.asarray(Wn, dtype=np.float64))
            out[f"raw{side}o"] = B.ratio(got2, ref2, B.raw_update_bar(ref, th, bars, pr.bar_M, N, p, side, 1, Wn)
                                         + np.abs(np.asarray(ref["Cuuo" if side else "Ctto"], dtype=LD)).sum() * 2.0 ** -52)
    return out


@pytest.mark.parametrize("orthonormal", [True, False])
def test_plain_fp64_numpy_lies_inside_every_bar(orthonormal):
    th, _, S, N = _problem(13, 9, 2, 2, 1, orthonormal, seed=8)
    r = _all_ratios(th, S, N, 13, 9)
    print(r)
    assert max(r.values()) <= 1.0, r


DEFECTS = {  # defect -> a quantity whose bar it must break
    "ctto_transposed": "raw0", "sigE_on_y": "Czz", "gg_identity": "Czz", "drop_column": "M", "chh_no_cross": "Chh",
    "ll_no_sigz": "loglik",
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defects_lie_outside(defect):
    th, _, S, N = _problem(13, 9, 2, 2, 1, False, seed=8)     # non-orthonormal: G'G is far from the identity
    r = _all_ratios(th, S, N, 13, 9, defect)
    print(defect, r[DEFECTS[defect]])
    assert r[DEFECTS[defect]] > 1.0, (defect, r)


@pytest.mark.parametrize("seed", B.HOST_SEEDS)
def test_the_specific_components_recover_what_the_shared_only_model_loses(seed):
    """The fp64 written-out loop: every increment of l over 300 steps is >= -1e-9 |l|, and the
    loading-space error with the specific parts is below half of that with rx = ry = 0."""
    X, Y, tr = B.host_problem(seed)
    s = B.HOST_SHAPE
    D = np.hstack([X, Y])
    S = D.T @ D
    t0 = B.start_theta(S, s["N"], s["p"], s["q"], s["r"], s["rx"], s["ry"], seed)
    th1, ll1, _ = B.em_loop(t0, S, s["N"], s["p"], s["q"], 300, -np.inf, np.float64)
    th0, ll0, _ = B.em_loop(B.without_specific(t0), S, s["N"], s["p"], s["q"], 300, -np.inf, np.float64)
    assert len(ll1) == 301
    for ll in (ll1, ll0):
        assert np.all(np.diff(ll) >= -1e-9 * np.abs(ll[-1]))
    P0 = tr["W"] @ tr["W"].T
    e1, e0 = np.linalg.norm(th1["W"] @ th1["W"].T - P0), np.linalg.norm(th0["W"] @ th0["W"].T - P0)
    print(f"seed {seed}: {e1:.3f} with the specific parts, {e0:.3f} shared only; b {th1['B']} vs {th0['B']}")
    assert e1 < 0.5 * e0


def test_stop_rule_and_history_length():
    X, Y, _ = B.host_problem(B.HOST_SEEDS[0])
    s = B.HOST_SHAPE
    D = np.hstack([X, Y])
    S = D.T @ D
    t0 = B.start_theta(S, s["N"], s["p"], s["q"], s["r"], s["rx"], s["ry"], 1)
    th, ll, mom = B.em_loop(t0, S, s["N"], s["p"], s["q"], 40, 5.0, np.float64)
    assert len(ll) < 41 and ll[-1] - ll[-2] < 5.0 and np.all(np.diff(ll)[:-1] >= 5.0)
    again = B.sform(th, S, s["N"], s["p"], s["q"], np.float64)          # the moments belong to the returned theta
    assert np.array_equal(again["Czz"], mom["Czz"]) and again["loglik"] == ll[-1]


def test_summary_and_canonical_form_on_hand_made_estimates():
    from ppls_amd import canonical_PO2PLS, simulate_PO2PLS, summary_PO2PLS
    e1, e2, e3 = np.eye(4)[:, 0], np.eye(4)[:, 1], np.eye(4)[:, 2]
    est = dict(W=np.column_stack([e1, e2]), Wo=np.column_stack([-e3, np.eye(4)[:, 3]]), C=np.column_stack([e1[:3], e2[:3]]),
               Co=e3[:3].reshape(3, 1) * -1.0, B=np.diag([-2.0, 0.5]), sigT=np.diag([1.0, 1.0]), sigTo=np.diag([1.0, 3.0]),
               sigUo=np.diag([2.0]), sigE=1.0, sigF=2.0, sigH=1.0)
    can = canonical_PO2PLS(est)
    # joint, signs: sign(sigT b) flips the first component so that b > 0
    assert np.array_equal(can["W"], np.column_stack([-e1, e2])) and np.array_equal(can["C"], np.column_stack([-e1[:3], e2[:3]]))
    assert np.array_equal(np.diag(can["B"]), [2.0, 0.5]) and np.array_equal(np.diag(can["sigT"]), [1.0, 1.0])
    # joint, order: decreasing |sigT b|
    swapped = canonical_PO2PLS(dict(est, B=np.diag([0.5, 2.0]), sigT=np.diag([1.0, 1.5])))
    assert np.array_equal(swapped["W"], np.column_stack([e2, e1])) and np.array_equal(np.diag(swapped["B"]), [2.0, 0.5])
    assert np.array_equal(np.diag(swapped["sigT"]), [1.5, 1.0])
    # specific: decreasing sigma, column sums >= 0
    assert np.array_equal(can["Wo"], np.column_stack([np.eye(4)[:, 3], e3])) and np.array_equal(np.diag(can["sigTo"]), [3.0, 1.0])
    assert np.array_equal(can["Co"], e3[:3].reshape(3, 1)) and np.array_equal(np.diag(can["sigUo"]), [2.0])
    assert np.array_equal(canonical_PO2PLS(can)["W"], can["W"])          # idempotent
    bar = B.canonical({k: (np.diag(v) if np.ndim(v) == 2 and k in ("B", "sigT", "sigTo", "sigUo") else v) for k, v in est.items()})
    assert np.array_equal(bar["W"], can["W"]) and np.array_equal(bar["Wo"], can["Wo"])
    # shares: var X = (1 + 1) + (1 + 9) + 4 * 1 = 16; var Y = (0.25 + 1) + (4 + 1) + 4 + 3 * 4 = 22.25
    sm = summary_PO2PLS(dict(estimates=est))
    assert np.isclose(sm["X"]["total"], 16.0) and np.isclose(sm["X"]["joint"], 2 / 16) and np.isclose(sm["X"]["specific"], 10 / 16)
    assert np.isclose(sm["Y"]["total"], 22.25) and np.isclose(sm["Y"]["specific"], 4 / 22.25) and np.isclose(sm["Y"]["noise"], 12 / 22.25)
    assert np.isclose(sm["predictable"], 4.25 / 6.25)
    for blk in ("X", "Y"):
        assert np.isclose(sm[blk]["joint"] + sm[blk]["specific"] + sm[blk]["noise"], 1.0)
    # the generator: shapes, all r columns of U, and the second moments of the model
    rng = np.random.default_rng(0)
    X, Y = simulate_PO2PLS(20000, est["W"], est["C"], est["Wo"], est["Co"], est["B"], 1.0, 2.0, 1.0, est["sigT"], est["sigTo"],
                           est["sigUo"], rng)
    assert X.shape == (20000, 4) and Y.shape == (20000, 3)
    Sig, _ = B.dense_cov(B.cast({k: (np.diag(v) if np.ndim(v) == 2 and k in ("B", "sigT", "sigTo", "sigUo") else np.asarray(v, dtype=float))
                                 for k, v in est.items()}, np.float64))
    D = np.hstack([X, Y])
    assert np.max(np.abs(D.T @ D / 20000 - Sig)) < 0.35                  # 5 sigma of the largest entry's sampling error
    assert abs((D.T @ D / 20000)[1, 5] - Sig[1, 5]) < 0.1 and Sig[1, 5] == 0.5   # the second column of U is there
