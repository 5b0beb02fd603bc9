"""The covariate adjustment's bars and host models on the CPU (tests/adjust_bar.py): plain fp64
in the kernels' stated order lies inside each a-priori bar against long double, seeded defects lie outside,
and the algebra (lstsq residuals, the Schur complement, the record) holds.  No GPU."""
import numpy as np
import pytest

import adjust_bar as ab
from adjust_bar import L, U


def _problem(n, p, k, seed=0, intercept=True):
    rng = np.random.default_rng([seed, n, p, k])
    Z = rng.standard_normal((n, k)) * (1.0 + np.arange(k) % 3) + (np.arange(k) % 4 - 1.5)
    B = rng.standard_normal((k, p))
    D = Z @ B + rng.standard_normal((n, p)) * (0.5 + np.arange(p) % 5) + (np.arange(p) % 3 - 1) * 2.0
    return Z, D


CASES = [(7, 3, 1), (40, 5, 4), (257, 6, 8), (600, 4, 15)]


@pytest.mark.parametrize("n,p,k", CASES)
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_models_inside_bars(n, p, k, f32):
    Z, D = _problem(n, p, k)
    if f32:
        D = D.astype(np.float32).astype(np.float64)
    q = ab.design_q(Z)
    Q = q["Q"]
    nb = ab.scale_plan(n, p, f32)["nblocks"]
    G = ab.coef_model(Q, D, nb)
    gbar = ab.coef_bar(Q, D, nb)
    rg = ab.inside(G, ab.ld_coef(Q, D), gbar)
    R = ab.apply_model(Q, G, D, f32)
    ref = np.asarray(D, dtype=L) - np.asarray(Q, dtype=L) @ ab.ld_coef(Q, D)      # with the Q as held
    rbar = ab.resid_bar(Q, G, D, gbar, f32, ref.astype(np.float64))
    rr = ab.inside(R, ref, rbar)
    # against the exact least-squares residual: the design's terms join
    exact, _ = ab.ld_resid(Z, D)
    kap = ab.design_kappa(Z)
    re = ab.inside(R, exact, rbar + ab.design_terms(Q, G, D, kap))
    print(f"n={n} p={p} k1={k + 1}: G err/bar {rg:.3g}, resid err/bar {rr:.3g}, against lstsq-exact {re:.3g}, kappa {kap:.3g}")
    assert rg <= 1.0 and rr <= 1.0 and re <= 1.0
    # lstsq itself agrees (its own error is of the design terms' kind)
    Zt = np.hstack([np.ones((n, 1)), Z])
    ls = D - Zt @ np.linalg.lstsq(Zt, D, rcond=None)[0]
    assert ab.inside(ls, exact, 2 * ab.design_terms(Q, G, D, kap) + rbar) <= 1.0


def test_seeded_defects_outside_bars():
    n, p, k = 257, 6, 8
    Z, D = _problem(n, p, k, seed=3)
    q = ab.design_q(Z)
    Q = q["Q"]
    k1 = Q.shape[1]
    nb = ab.scale_plan(n, p, 0)["nblocks"]
    assert nb > 1
    gref = ab.ld_coef(Q, D)
    gbar = ab.coef_bar(Q, D, nb)
    G = ab.coef_model(Q, D, nb)
    ref = np.asarray(D, dtype=L) - np.asarray(Q, dtype=L) @ gref
    rbar = ab.resid_bar(Q, G, D, gbar)
    # a skipped row block
    assert ab.inside(ab.coef_model(Q, D, nb, skip_block=nb - 1), gref, gbar) > 1e6
    # a dropped last design column
    assert ab.inside(ab.apply_model(Q[:, :-1], G[:-1], D), ref, rbar) > 1e6
    # the pad slot of KT read as a real column: slot k1 of a row holds what follows it in memory
    kt = ab.kt_of(k1)
    assert kt > k1
    Qp = np.zeros((n + 1, kt))
    Qp[:n, :k1] = Q
    flat = Qp.ravel()
    leak = np.hstack([Q, flat[np.arange(n) * kt + kt][:, None]])        # the next row's first value
    Gl = ab.coef_model(leak, D, nb)
    assert ab.inside(ab.apply_model(leak, Gl, D), ref, rbar) > 1e6
    # the residual accumulated in fp32
    assert ab.inside(ab.apply_model(Q, G, D, acc32=True), ref, rbar) > 1e3


@pytest.mark.parametrize("k", [1, 3, 16])
def test_schur_complement_is_the_gram_of_the_residuals(k):
    n, p, qy = 300, 5, 4
    Z, D = _problem(n, p + qy, k, seed=7)
    Zc, Dc = Z - Z.mean(axis=0), D - D.mean(axis=0)
    ldx, ldy_src, ldy = p + 1, (qy + k + 1) & ~1, (qy + 1) & ~1
    ldy_src += 2
    src_live = ab.joint_live(p, ldx, qy + k, ldy_src)
    M = np.zeros((n, ldx + ldy_src))
    M[:, :p] = Dc[:, :p]
    M[:, ldx:ldx + qy] = Dc[:, p:]
    M[:, ldx + qy:ldx + qy + k] = Zc
    S = M.T @ M
    live = ab.joint_live(p, ldx, qy, ldy)
    f, piv = ab.schur_f(S, ldx + qy, k, live)
    assert piv == 0
    got = ab.schur_model(S, f["Ft"], live)
    ref = ab.ld_schur(S, ldx + qy, k, live)
    bar = ab.schur_bar(S, f, live)
    r = ab.inside(got, ref, bar)
    print(f"k={k}: Schur model err/bar {r:.3g}, kappa(C) {f['kappa']:.3g}")
    assert r <= 1.0 and np.array_equal(got, got.T) and not got[~np.outer(live, live)].any()
    # = the Gram of the residualised rows (both from fp64 Grams of n rows: gamma(n + 2) |M|'|M| apart)
    res, _ = ab.ld_resid(Z, D)
    Rm = np.zeros((n, ldx + ldy), dtype=L)
    Rm[:, :p] = res[:, :p]
    Rm[:, ldx:ldx + qy] = res[:, p:]
    gram = Rm.T @ Rm
    aM = np.abs(M)
    gbar = ab.gamma(n + 2) * (aM.T @ aM)[: ldx + ldy, : ldx + ldy]
    kap2 = f["kappa"]
    fz = np.abs(f["Ft"]).T @ np.abs(f["Ft"])
    assert ab.inside(got, gram, bar + gbar * (1 + kap2) + ab.gamma(n + 2) * kap2 * fz * 4) <= 1.0
    # the mirror taken from the upper triangle of a deliberately asymmetric input
    Sa = S.copy()
    Sa[np.triu_indices_from(Sa, 1)] *= 1.0 + 1e-9
    assert ab.inside(ab.schur_model(Sa, f["Ft"], live), ref, bar) <= 1.0
    assert ab.inside(ab.schur_model(Sa, f["Ft"], live, mirror_upper=True), ref, bar) > 1e3
    # scale = 1: a unit diagonal
    Rs, sbar = ab.schur_scaled(ref, bar, live)
    gs, _ = ab.schur_scaled(got, bar, live)
    assert ab.inside(gs, Rs, sbar) <= 1.0
    assert np.allclose(np.diag(gs)[live], 1.0, rtol=0, atol=4 * U)


def test_pivot_rule():
    rng = np.random.default_rng(11)
    n, k = 400, 5
    Z = rng.standard_normal((n, k))
    for n_, k_ in ((40, 15), (400, 5)):
        Zb = rng.standard_normal((n_, k_))
        Zc = Zb - Zb.mean(axis=0)
        # the last column = a combination of the others + a remainder of relative norm eps
        e = rng.standard_normal(n_)
        e -= e.mean()
        for m in range(k_ - 1):
            e -= Zc[:, m] * (Zc[:, m] @ e) / (Zc[:, m] @ Zc[:, m])
        comb = Zc[:, : k_ - 1] @ rng.standard_normal(k_ - 1)
        for eps, ok in ((2e-7, True), (3e-8, False)):
            Zb[:, -1] = comb + e * (eps * np.linalg.norm(comb) / np.linalg.norm(e)) + 0.3
            q = ab.design_q(Zb)
            if ok:
                Q = q["Q"]
                defect = np.abs(Q.T @ Q - np.eye(k_ + 1)).max()
                print(f"n={n_} k1={k_ + 1} pivot {eps:g}: max|Q'Q - I| = {defect:.3g}, bar {ab.eq_of(n_, k_ + 1):.3g}")
                assert defect <= ab.eq_of(n_, k_ + 1)
            else:
                assert q.get("refused") == k_
    Z[:, 3] = Z[:, 1]                       # a duplicated column
    assert ab.design_q(Z).get("refused") == 4
    Z[:, 3] = 2.5                           # a constant column beside the intercept
    assert ab.design_q(Z).get("refused") == 4
    assert "Q" in ab.design_q(Z, intercept=False)   # ... which is a fair column without one


def test_sharded_design_equals_unsharded_to_rounding():
    Z, _ = _problem(101, 2, 4, seed=5)
    a = ab.design_q(Z)
    b = ab.design_q(Z, shards=[(0, 40), (40, 40), (40, 101)])
    assert np.abs(a["Q"] - b["Q"]).max() <= 1e-13


class _Record:
    """The two records of a context, for adjust_new."""

    def __init__(self, p, sc, ad):
        self.p, self._sc, self._ad = p, sc, ad

    def scaling(self):
        return self._sc

    def adjustment(self):
        return self._ad


def test_adjust_new_inverts_the_record():
    from ppls_amd.api import adjust_new
    n, p, qy, k = 60, 4, 3, 2
    Z, D = _problem(n, p + qy, k, seed=9)
    q = ab.design_q(Z)
    G = ab.coef_model(q["Q"], D, 1)
    gam, cen = ab.gamma_from(G, q)
    R = ab.apply_model(q["Q"], G, D)
    sd = R.std(axis=0, ddof=1)
    resident = R / sd                       # adjust, then scale(center = FALSE-like: the residuals' means are 0)
    rec = _Record(p, dict(centerX=cen[:p], scaleX=sd[:p], centerY=cen[p:], scaleY=sd[p:]),
                  dict(k=k, zcenter=q["zc"], coefX=gam[:, :p], coefY=gam[:, p:]))
    gX, gY = adjust_new(rec, D[:, :p], D[:, p:], Z)
    assert np.abs(gX - resident[:, :p]).max() <= 1e-11 and np.abs(gY - resident[:, p:]).max() <= 1e-11
    # the record's formula gives the loaded rows back
    back = resident * sd + cen + (Z - q["zc"]) @ gam
    assert np.abs(back - D).max() <= 1e-11 * np.abs(D).max()
    # Gamma is lm's slope
    Zt = np.hstack([np.ones((n, 1)), Z])
    coef = np.linalg.lstsq(Zt, D, rcond=None)[0][1:]
    assert ab.inside(gam, ab.ld_gamma(Z, D), ab.gamma_bar(Z, D)) <= 1.0
    assert ab.inside(coef, ab.ld_gamma(Z, D), ab.gamma_bar(Z, D)) <= 1.0
    # either block alone, one row, and the refusal without Z
    assert adjust_new(rec, None, D[:1, p:], Z[:1])[0] is None
    assert np.allclose(adjust_new(rec, D[0, :p], None, Z[0])[0], gX[:1], rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        adjust_new(rec, D[:, :p], None, None)
    plain = _Record(p, rec.scaling(), dict(k=0, zcenter=np.zeros(0), coefX=np.zeros((0, p)), coefY=np.zeros((0, qy))))
    assert np.array_equal(adjust_new(plain, D[:, :p], None)[0], (D[:, :p] - cen[:p]) / sd[:p])
