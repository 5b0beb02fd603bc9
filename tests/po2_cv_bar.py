"""Long-double references and a priori bars for PO2PLS prediction and cross-validation.

The prediction map (ppls_po2_predict_map).  For the X side, with Gx = [W Wo] (p x kx), d = 1 / sigE^2:
    Lambda = diag(sigT, sigTo)^-2 + d Gx'Gx,   X = Lambda^-1 E_r,   L = d Gx X   (p x r),
and E[y | x] = C diag(B) L'x.  The Y side is the same with Gy = [C Co], d = 1 / sigF^2 and the MARGINAL
variances sigT^2 b^2 + sigH^2, sigUo^2 of (u, uo); E[x | y] = W diag(beta) L'y with
beta_j = sigT_j^2 b_j / (sigT_j^2 b_j^2 + sigH^2), returned as Bp = 1 / beta.

The bar on L is normwise (Frobenius) and built like po2_bar.small_bars:
    bar_L = (8 k^2 u kappa_2(Lambda) ||Gx||_F ||X||_F  +  gamma_k || |Gx| |X| ||_F) d  x  SLACK
  * 8 k^2 u kappa_2(Lambda): the Cholesky factorisation and the two triangular solves of a k x k system
    (Higham, Accuracy and Stability, Thm 10.4 with the constant of small_bars' rho); it also covers the
    three roundings of d and of the final scaling by d (8 k^2 >= 8 > 3);
  * gamma_k: the k-term inner products of the product Gx X;
  * SLACK = 1 + 2^-10 (sweep_bar): the bars themselves are evaluated in floating point.
kappa_2(Lambda) comes from the long-double Lambda.  The composed map A = C diag(Bp) L' (or W diag(1/Bp) L')
is formed in long double from the returned (L, Bp) and compared with the dense conditional mean
Sigma_yx Sigma_xx^-1 (Sigma_xy Sigma_yy^-1) of po2_bar.dense_cov in long double:
    bar_A = ||C diag(B)||_2 bar_L                                  (X side: Bp = B is copied, no rounding)
    bar_A = ||W diag(beta)||_2 bar_L + 8 u || |W diag(beta)| |L|' ||_F   (Y side: 1 / beta takes 6 roundings)
"""
import numpy as np

import po2_bar as B
from finalize_bar import inverse
from sweep_bar import LD, SLACK, U, gamma


def _fro(A):
    return np.sqrt(np.sum(np.asarray(A, dtype=LD) ** 2))


def side_parts(th, xory, dt=LD):
    """(G, var, d, r): the side's loadings [joint | specific], the marginal variances of its latent variables,
    1 / sigma_noise^2 and r, in dtype dt."""
    th = B.cast(th, dt)
    r = th["W"].shape[1]
    if xory == 0:
        return np.hstack([th["W"], th["Wo"]]), np.concatenate([th["sigT"] ** 2, th["sigTo"] ** 2]), 1 / th["sigE"] ** 2, r
    return (np.hstack([th["C"], th["Co"]]), np.concatenate([th["sigT"] ** 2 * th["B"] ** 2 + th["sigH"] ** 2, th["sigUo"] ** 2]),
            1 / th["sigF"] ** 2, r)


def predict_map(th, xory, dt=LD, defect=None):
    """(L, Bp, Lambda, X) by the formula of the module docstring in dtype dt.  defect (X side, seeded wrong
    formulas a correct bar must reject): 'no_specific' leaves Wo out of Lambda, 'joint' takes the (t, to)
    block of the joint Sigma_z^-1 instead of the marginal diag(sigT, sigTo)^-2, 'no_scale' forgets 1 / sigE^2."""
    G, var, d, r = side_parts(th, xory, dt)
    k = G.shape[1]
    prior = np.diag(1 / var)
    if defect == "joint":
        prior = B.sigma_z_inv(B.cast(th, dt))[:k, :k]
    Gl = G.copy()
    if defect == "no_specific":
        Gl[:, r:] = 0
    Lam = prior + d * (Gl.T @ Gl)
    X = (inverse(Lam) if dt == LD else np.linalg.inv(Lam))[:, :r]
    L = G @ X * (1 if defect == "no_scale" else d)
    t = B.cast(th, dt)
    Bp = t["B"] if xory == 0 else (t["sigT"] ** 2 * t["B"] ** 2 + t["sigH"] ** 2) / (t["sigT"] ** 2 * t["B"])
    return L, Bp, Lam, X


def map_bar(th, xory):
    """(L_ref, bar_L) of the module docstring."""
    L, _, Lam, X = predict_map(th, xory, LD)
    G, _, d, _ = side_parts(th, xory, LD)
    k = G.shape[1]
    kap = LD(np.linalg.cond(np.asarray(Lam, dtype=np.float64)))
    bar = (8 * k * k * U * kap * _fro(G) * _fro(X) + gamma(k) * _fro(np.abs(G) @ np.abs(X))) * d * SLACK
    return L, bar


def composed(th, xory, L, Bp, dt=LD):
    """The q x p (p x q) matrix of the prediction from a returned (L, Bp), formed in dt."""
    t = B.cast(th, dt)
    L, Bp = np.asarray(L).astype(dt), np.asarray(Bp).astype(dt)
    return (t["C"] * Bp) @ L.T if xory == 0 else (t["W"] / Bp) @ L.T


def dense_conditional(th, xory):
    """Sigma_yx Sigma_xx^-1 (xory 0) or Sigma_xy Sigma_yy^-1 (1) in long double."""
    t = B.cast(th, LD)
    Sig, _ = B.dense_cov(t)
    p = t["W"].shape[0]
    if xory == 0:
        return Sig[p:, :p] @ inverse(Sig[:p, :p])
    return Sig[:p, p:] @ inverse(Sig[p:, p:])


def composed_bar(th, xory):
    """bar_A of the module docstring."""
    t = B.cast(th, LD)
    L, bar_L = map_bar(th, xory)
    if xory == 0:
        F = t["C"] * t["B"]
        return LD(np.linalg.norm(np.asarray(F, dtype=np.float64), 2)) * SLACK * bar_L
    beta = t["sigT"] ** 2 * t["B"] / (t["sigT"] ** 2 * t["B"] ** 2 + t["sigH"] ** 2)
    F = t["W"] * beta
    return (LD(np.linalg.norm(np.asarray(F, dtype=np.float64), 2)) * SLACK * bar_L + 8 * U * _fro(np.abs(F) @ np.abs(L).T)) * SLACK


def rmsep_rows(th, X, Y):
    """sqrt(mean((Y - E[y | x])^2)) over the given rows, in long double, for estimates th (po2_bar's dict)."""
    L, Bp, _, _ = predict_map(th, 0, LD)
    A = composed(th, 0, L, Bp, LD)
    R = np.asarray(Y).astype(LD) - np.asarray(X).astype(LD) @ A.T
    return np.sqrt(np.sum(R * R) / LD(R.size))


def host_cv(X, Y, labels, r, rx, ry, steps=200, atol=1e-4, seed=7):
    """The host loop of the issue: per fold the fp64 EM loop of po2_bar from start_theta(seed) on the training
    rows' cross-products, the RMSEP of the prediction map on the held-out rows.  Returns the per-fold errors."""
    labels = np.asarray(labels)
    p, q = X.shape[1], Y.shape[1]
    out = []
    for f in range(int(labels.max()) + 1):
        tr = labels != f
        D = np.hstack([X[tr], Y[tr]])
        S, N = D.T @ D, float(tr.sum())
        t0 = B.start_theta(S, N, p, q, r, rx, ry, seed)
        th, _, _ = B.em_loop(t0, S, N, p, q, steps, atol, np.float64)
        out.append(float(rmsep_rows(th, X[~tr], Y[~tr])))
    return np.array(out)
