"""Long-double references and a-priori error bars for PO2PLS from the cross-products (ppls_po2.hip).

Shared by tests/test_po2_host.py (the algebra and the bars themselves, no GPU) and
tests/test_gpu_po2.py (the HIP kernels against them).

The model (the reference's simulC, loglC, EMstepC; Package/PPLS/src/loglC.cpp:268-315, :36-113, :116-250):
    x = W t + Wo to + e,  y = C u + Co uo + f,  u = B t + h,
theta = dict(W, Wo, C, Co, B (r), sigT (r), sigTo (rx), sigUo (ry), sigE, sigF, sigH), sigmas standard
deviations.  Latent order z = (t, to | u, uo), kx = r + rx, ky = r + ry, k = kx + ky.

Two restatements, both generic in the dtype (np.longdouble for the reference, np.float64 for "plain
numpy in the kernels' order"):

* ``dense_estep`` / ``dense_loglik``: EMstepC and loglC through the dense (p+q) x (p+q) covariance and
  its inverse (Gauss-Jordan in long double: numpy's linalg has no long double).
* ``sform``: the same from S alone -- M = S G, Q = G'M, G'G, Lambda = Sigma_z^-1 + D G'G, K = D Lambda^-1,
  C_dz = M K / N, C_zz = Lambda^-1 + K'QK / N, Cee, Cff, Chh and the log-likelihood.
* ``ecm_update`` / ``em_loop``: the ECM cycle and the loop as the issue states them.

Bars.  u = 2^-53, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms,
3.1 and 3.5: a dot product of n terms, any order, with or without FMA, errs by at most gamma_n |a|'|b|).
Nothing below is measured; every constant is listed here.

  M, entrywise:    gamma_{ld + 2} (|S| |G|)          ld = the padded panel width; + 2 to spare
  G'G, entrywise:  gamma_{ld + 2} |G|'|G|
  Q, entrywise:    gamma_{ld + 2} |G|'|M| + (1 + gamma_{ld + 2}) |G|' bar_M

  The small algebra is bounded normwise (Frobenius norms, so every entry obeys the bar of its matrix).
  e_Q = ||bar_Q||_F, e_G = ||bar_GG||_F are the pass's bars carried in; with kL = kappa_2(Lambda),
  kS = kappa_2(Sigma_z), d = max(sigE^-2, sigF^-2):
    e_L   = d e_G + 8 u kS ||Lambda||_F
            (Lambda's entries are a closed form of Sigma_z^-1 -- at most 6 roundings each, 8 to spare,
            times kS because the closed form's terms are as large as ||Sigma_z^-1|| while Lambda's
            small eigenvalues are as small as 1 / ||Sigma_z|| -- plus d times the Gram's own error)
    rho   = c(k) u kL kS + kL e_L / ||Lambda||_2,    c(k) = 8 k^2
            (relative error of Lambda^-1.  Higham Thm 10.3/10.4: Cholesky's backward error is
            gamma_{3k+1} |L||L'| and || |L||L'| ||_2 <= k ||Lambda||_2, so a solve errs by at most
            (3k + 1) k u kL <= 4 k^2 u kL relatively; the explicit inverse is two triangular solves
            per column and a mirror: twice that.  kS as the issue states the bar; it only widens it.)
    e_I   = rho ||Lambda^-1||_F
    e_K   = d e_I + u ||K||_F
    e_T   = e_Q ||K||_F + ||Q||_F e_K + gamma_{k+1} ||Q||_F ||K||_F            (T = Q K)
    e_Z   = e_I + (e_K ||T||_F + ||K||_F e_T + gamma_{k+1} ||K||_F ||T||_F) / N + 2 u ||Czz||_F
    e_Cee = (2 sqrt(kx) e_T / N + e_G ||Czz||_F + ||GGx||_F e_Z
             + gamma_{kx^2 + 6} (ssqX / N + 2 |tr T_xx| / N + |GGx| . |Czz_xx|)) / p       (Cff alike)
    e_Chh = (1 + max|b|)^2 e_Z + 8 u (1 + max|b|)^2 max|Czz|
    e_ll  = N/2 (k (rho + 4 u) + gamma_{3k + 8} (|p log sE^2| + |q log sF^2| + sum |log sigma^2| + |logdet Lambda|))
            + 1/2 (d sqrt(k) e_T + gamma_{k + 8} (ssqX / sE^2 + ssqY / sF^2 + d sum |T_aa|))
            + 4 u |ll|
            (log det Lambda moves by at most k times the relative perturbation of its eigenvalues)
  A raw loading update R = (M K_cols) / N - L_other Coef (stage 1: K's t columns, Coef = Ctto'):
    entrywise  (bar_M |K_cols| + rowsum|M| e_K + gamma_{k+2} |M||K_cols|) / N
               + rowsum|L_other| e_Z + gamma_{c+2} |L_other||Coef|
each times 1 + 2^-10 for the reference's own rounding.
"""
import math

import numpy as np

from finalize_bar import householder_qr, inverse, polar_small
from sweep_bar import LD, SLACK, U, gamma, padded_width


# ------------------------------------------------------------------------------------------- model
def shape(th):
    r, rx, ry = th["W"].shape[1], th["Wo"].shape[1], th["Co"].shape[1]
    return r, rx, ry, r + rx, r + ry, 2 * r + rx + ry


def cast(th, dt):
    out = {}
    for k, v in th.items():
        out[k] = np.asarray(v, dtype=np.float64).astype(dt) if np.ndim(v) else dt(v)
    return out


def make_theta(rng, p, q, r, rx, ry, orthonormal=True, scale=1.0):
    """A well-conditioned theta.  orthonormal: [W Wo] and [C Co] have orthonormal columns; else plain
    normal draws times `scale` (custom starts need not be orthonormal)."""
    def load(n, c):
        A = rng.standard_normal((n, c))
        return np.linalg.qr(A)[0] if orthonormal and c else A * scale / math.sqrt(n)
    Gx, Gy = load(p, r + rx), load(q, r + ry)
    return dict(W=Gx[:, :r], Wo=Gx[:, r:], C=Gy[:, :r], Co=Gy[:, r:],
                B=1.2 - 0.15 * np.arange(r), sigT=1.5 - 0.1 * np.arange(r), sigTo=1.1 - 0.1 * np.arange(rx),
                sigUo=0.9 - 0.1 * np.arange(ry), sigE=0.7, sigF=0.8, sigH=0.5)


def loadings(th):
    return np.hstack([th["W"], th["Wo"]]), np.hstack([th["C"], th["Co"]])


def sigma_z(th):
    """The prior covariance of z = (t, to | u, uo)."""
    r, rx, ry, kx, ky, k = shape(th)
    dt = th["W"].dtype
    Sz = np.zeros((k, k), dtype=dt)
    b, t2 = th["B"], th["sigT"] ** 2
    for j in range(r):
        Sz[j, j] = t2[j]
        Sz[j, kx + j] = Sz[kx + j, j] = t2[j] * b[j]
        Sz[kx + j, kx + j] = t2[j] * b[j] ** 2 + th["sigH"] ** 2
    for j in range(rx):
        Sz[r + j, r + j] = th["sigTo"][j] ** 2
    for j in range(ry):
        Sz[kx + r + j, kx + r + j] = th["sigUo"][j] ** 2
    return Sz


def sigma_z_inv(th):
    """Its inverse in closed form (the kernel's)."""
    r, rx, ry, kx, ky, k = shape(th)
    dt = th["W"].dtype
    Si = np.zeros((k, k), dtype=dt)
    b, iH = th["B"], 1 / th["sigH"] ** 2
    for j in range(r):
        Si[j, j] = 1 / th["sigT"][j] ** 2 + b[j] ** 2 * iH
        Si[j, kx + j] = Si[kx + j, j] = -b[j] * iH
        Si[kx + j, kx + j] = iH
    for j in range(rx):
        Si[r + j, r + j] = 1 / th["sigTo"][j] ** 2
    for j in range(ry):
        Si[kx + r + j, kx + r + j] = 1 / th["sigUo"][j] ** 2
    return Si


def _inv(A):
    return inverse(A) if A.dtype == LD else np.linalg.inv(A)


def _logdet_spd(A):
    """log det of a symmetric positive definite matrix by Cholesky (raises when it is not)."""
    A = np.array(A)
    n = A.shape[0]
    s = A.dtype.type(0)
    for j in range(n):
        d = A[j, j] - A[j, :j] @ A[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        A[j, j] = np.sqrt(d)
        A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
        s = s + 2 * np.log(A[j, j])
    return s


def blocks_of(Czz, th):
    r, rx, ry, kx, ky, k = shape(th)
    t, to, u, uo = slice(0, r), slice(r, kx), slice(kx, kx + r), slice(kx + r, k)
    return dict(Ctt=Czz[t, t], Ctoto=Czz[to, to], Ctto=Czz[t, to], Cuu=Czz[u, u], Cuouo=Czz[uo, uo], Cuuo=Czz[u, uo],
                Cut=Czz[u, t])


# ------------------------------------------------------------------------------------- dense form
def dense_cov(th):
    Gx, Gy = loadings(th)
    p, q = Gx.shape[0], Gy.shape[0]
    r, rx, ry, kx, ky, k = shape(th)
    G = np.zeros((p + q, k), dtype=Gx.dtype)
    G[:p, :kx], G[p:, kx:] = Gx, Gy
    Sig = G @ sigma_z(th) @ G.T
    Sig[np.arange(p), np.arange(p)] += th["sigE"] ** 2
    Sig[p + np.arange(q), p + np.arange(q)] += th["sigF"] ** 2
    return Sig, G


def dense_estep(th, S, N, dt=LD):
    """EMstepC (loglC.cpp:116-250) restated: every moment through invS = Sigma^-1 (dense)."""
    th = cast(th, dt)
    S = np.asarray(S).astype(dt)
    Sig, G = dense_cov(th)
    p = th["W"].shape[0]
    q = th["C"].shape[0]
    r, rx, ry, kx, ky, k = shape(th)
    invS = _inv(Sig)
    Cd = S / dt(N)
    covZ = G @ sigma_z(th)                       # cov(d, z): the columns are covT, covTo, covU, covUo
    delZ = invS @ covZ
    Czz = sigma_z(th) - covZ.T @ invS @ covZ + delZ.T @ Cd @ delZ
    Cdz = Cd @ delZ
    out = blocks_of(Czz, th)
    out.update(Cxt=Cdz[:p, :r], Cxto=Cdz[:p, r:kx], Cyu=Cdz[p:, kx:kx + r], Cyuo=Cdz[p:, kx + r:], Czz=Czz)
    A = invS @ Cd @ invS
    sE2, sF2, sH2 = th["sigE"] ** 2, th["sigF"] ** 2, th["sigH"] ** 2
    out["Cee"] = np.trace(sE2 * np.eye(p, dtype=dt) - sE2 * sE2 * invS[:p, :p] + sE2 * sE2 * A[:p, :p]) / p   # :219-220
    out["Cff"] = np.trace(sF2 * np.eye(q, dtype=dt) - sF2 * sF2 * invS[p:, p:] + sF2 * sF2 * A[p:, p:]) / q
    SH0 = np.vstack([np.zeros((p, r), dtype=dt), th["C"] * sH2])                                              # :215-216
    out["Chh"] = sH2 * np.eye(r, dtype=dt) - SH0.T @ invS @ SH0 + SH0.T @ A @ SH0                             # :223-224
    return out


def dense_loglik(th, S, N, dt=LD):
    """loglC (:36-88) with the constant -N (p+q)/2 log 2 pi (loglC_fast's)."""
    th = cast(th, dt)
    S = np.asarray(S).astype(dt)
    Sig, _ = dense_cov(th)
    P = Sig.shape[0]
    return -dt(0.5) * N * P * _log2pi(dt) - dt(0.5) * N * _logdet_spd(Sig) - dt(0.5) * np.sum(_inv(Sig) * S)


_PI_LO = LD("1.2246467991473531772e-16") if np.finfo(LD).eps < 1e-17 else LD(0)   # pi - fp64(pi)


def _log2pi(dt):
    return np.log(2 * (LD(math.pi) + _PI_LO)) if dt == LD else dt(math.log(2 * math.pi))


# ----------------------------------------------------------------------------------------- S form
def sform(th, S, N, p, q, dt=LD, defect=None):
    """Every statistic of one E-step from S (P x P in the joint layout of p and q real columns, no
    padding here).  defect: one of the seeded defects of the host test (None: none)."""
    th = cast(th, dt)
    S = np.asarray(S).astype(dt)
    N = dt(N)
    r, rx, ry, kx, ky, k = shape(th)
    Gx, Gy = loadings(th)
    Mx, My = S[:, :p] @ Gx, S[:, p:] @ Gy
    if defect == "drop_column":          # 4: the last column of a panel dropped
        Mx = S[:, :p - 1] @ Gx[:p - 1]
    M = np.hstack([Mx, My])
    G = np.zeros((p + q, k), dtype=dt)
    G[:p, :kx], G[p:, kx:] = Gx, Gy
    Q = G.T @ M
    Q = (Q + Q.T) / 2 if dt == LD else np.triu(Q) + np.triu(Q, 1).T
    GGx, GGy = Gx.T @ Gx, Gy.T @ Gy
    if defect == "gg_identity":          # 3: G'G taken as the identity
        GGx, GGy = np.eye(kx, dtype=dt), np.eye(ky, dtype=dt)
    return small(th, Q, GGx, GGy, N, p, q, np.trace(S[:p, :p]), np.trace(S[p:, p:]), dt, defect, M=M)


def small(th, Q, GGx, GGy, N, p, q, ssqX, ssqY, dt=LD, defect=None, M=None):
    """The k x k algebra on given Q, G'G blocks and theta's scalars (the small kernel's job)."""
    th = cast(th, dt)
    Q, GGx, GGy = (np.asarray(A).astype(dt) for A in (Q, GGx, GGy))
    N, ssqX, ssqY = dt(N), dt(ssqX), dt(ssqY)
    r, rx, ry, kx, ky, k = shape(th)
    dE, dF = 1 / th["sigE"] ** 2, 1 / th["sigF"] ** 2
    d = np.concatenate([np.full(kx, dE), np.full(ky, dE if defect == "sigE_on_y" else dF)]).astype(dt)   # 2
    GG = np.zeros((k, k), dtype=dt)
    GG[:kx, :kx], GG[kx:, kx:] = GGx, GGy
    Lam = sigma_z_inv(th) + d[:, None] * GG
    logdetL = _logdet_spd(Lam)
    Li = _inv(Lam)
    Li = (Li + Li.T) / 2
    K = d[:, None] * Li
    T = Q @ K
    Czz = Li + K.T @ T / N
    Czz = (Czz + Czz.T) / 2
    out = blocks_of(Czz, th)
    out.update(Q=Q, GGx=GGx, GGy=GGy, K=K, Czz=Czz, T=T, Lam=Lam, Li=Li, logdetL=logdetL, d=d, M=M)
    if M is not None:
        Cdz = M @ K / N
        out.update(Cxt=Cdz[:p, :r], Cxto=Cdz[:p, r:kx], Cyu=Cdz[p:, kx:kx + r], Cyuo=Cdz[p:, kx + r:])
    out["Cee"] = (ssqX / N - 2 * np.trace(T[:kx, :kx]) / N + np.sum(GGx * Czz[:kx, :kx])) / p
    out["Cff"] = (ssqY / N - 2 * np.trace(T[kx:, kx:]) / N + np.sum(GGy * Czz[kx:, kx:])) / q
    B = np.diag(th["B"])
    Ctt, Cuu, Cut = out["Ctt"], out["Cuu"], out["Cut"]
    out["Chh"] = Cuu.copy() if defect == "chh_no_cross" else Cuu - B @ Cut.T - Cut @ B + B @ Ctt @ B      # 5
    lds = 2 * (np.sum(np.log(th["sigT"])) + r * np.log(th["sigH"]) + np.sum(np.log(th["sigTo"])) + np.sum(np.log(th["sigUo"])))
    if defect == "ll_no_sigz":           # 6
        lds = dt(0)
    trd = np.sum(d * np.diag(T))
    out["loglik"] = (-dt(0.5) * N * (p + q) * _log2pi(dt)
                     - dt(0.5) * N * (p * 2 * np.log(th["sigE"]) + q * 2 * np.log(th["sigF"]) + lds + logdetL)
                     - dt(0.5) * (ssqX * dE + ssqY * dF - trd))
    return out


# ------------------------------------------------------------------------------------------- ECM
def orth(A, type="SVD"):
    """orth of a tall matrix: the polar factor (type = "SVD"), or sign_e qr.Q(qr(A)) with
    sign_e = sign(R_11) (type = "QR"; Householder, R's and LAPACK's sign convention)."""
    if type == "QR":
        if A.dtype == LD:
            Qh, R = householder_qr(A)
        else:
            Qh, R = np.linalg.qr(A)
        return Qh * (-1 if R[0, 0] < 0 else 1)
    if A.dtype == LD:
        Qh, R = householder_qr(A)
        return Qh @ polar_small(R)
    Uu, _, Vt = np.linalg.svd(A, full_matrices=False)
    return Uu @ Vt


def raw_updates(th, mom, p, side, stage, W_new=None, defect=None):
    """The matrix orth() is applied to: side 0 (X) / 1 (Y), stage 0 (joint) / 1 (specific)."""
    if side == 0:
        Cd, Cdo, Cto, Lo = mom["Cxt"], mom["Cxto"], mom["Ctto"], th["Wo"]
    else:
        Cd, Cdo, Cto, Lo = mom["Cyu"], mom["Cyuo"], mom["Cuuo"], th["Co"]
    if stage == 0:
        bad = defect == "ctto_transposed" and side == 0     # the X side, where r = rx makes it go unnoticed
        return Cd - Lo @ (Cto if bad else Cto.T)                                                          # 1
    return Cdo - W_new @ Cto


def ecm_update(th, mom, p, dt=LD, type="SVD"):
    """One ECM cycle from the E-step moments `mom` of theta (already of dtype dt)."""
    th = cast(th, dt)
    r, rx, ry, kx, ky, k = shape(th)
    new = dict(th)
    new["W"] = orth(raw_updates(th, mom, p, 0, 0), type)
    new["C"] = orth(raw_updates(th, mom, p, 1, 0), type)
    if rx:
        new["Wo"] = orth(raw_updates(th, mom, p, 0, 1, new["W"]), type)
    if ry:
        new["Co"] = orth(raw_updates(th, mom, p, 1, 1, new["C"]), type)
    new["B"] = np.diag(mom["Cut"]) / np.diag(mom["Ctt"])
    new["sigT"] = np.sqrt(np.diag(mom["Ctt"]))
    new["sigTo"] = np.sqrt(np.diag(mom["Ctoto"])) if rx else th["sigTo"]
    new["sigUo"] = np.sqrt(np.diag(mom["Cuouo"])) if ry else th["sigUo"]
    new["sigE"], new["sigF"] = np.sqrt(mom["Cee"]), np.sqrt(mom["Cff"])
    new["sigH"] = np.sqrt(np.trace(mom["Chh"]) / r)
    return new


def em_loop(th0, S, N, p, q, steps, atol, dt=LD, type="SVD"):
    """The loop of the issue: returns (theta, [l_0 .. l_steps'], moments at theta)."""
    th = cast(th0, dt)
    ll = []
    for i in range(1, steps + 1):
        mom = sform(th, S, N, p, q, dt)
        ll.append(mom["loglik"])
        if i >= 2 and ll[-1] - ll[-2] < atol:
            return th, ll, mom
        th = ecm_update(th, mom, p, dt, type)
    mom = sform(th, S, N, p, q, dt)
    ll.append(mom["loglik"])
    return th, ll, mom


def canonical(th):
    """The canonical form of estimates: the joint part by PPLS_simult's rule (EM_W_multi.R:794-799:
    decreasing |sigT b|, signs sign(sigT b)), the specific components by decreasing sigma, each
    column's sign so that its sum is >= 0."""
    th = {k: np.array(v) if np.ndim(v) else v for k, v in th.items()}
    sb = th["sigT"] * th["B"]
    sg = np.sign(sb)
    rot = np.argsort(-(th["sigT"] * (th["B"] * sg)), kind="stable")
    th["W"], th["C"] = th["W"][:, rot] * sg, th["C"][:, rot] * sg
    th["B"], th["sigT"] = (th["B"] * sg)[rot], th["sigT"][rot]
    for L, s in (("Wo", "sigTo"), ("Co", "sigUo")):
        if th[L].shape[1]:
            o = np.argsort(-th[s], kind="stable")
            A = th[L][:, o]
            th[L], th[s] = A * np.where(A.sum(axis=0) < 0, -1.0, 1.0), th[s][o]
    return th


def projector_distance(A, B):
    """||A A^+ - B B^+||_F for full-column-rank loadings (as projectors onto their column spaces)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.shape[1] == 0:
        return 0.0
    qa, qb = np.linalg.qr(A)[0], np.linalg.qr(B)[0]
    return float(np.linalg.norm(qa @ qa.T - qb @ qb.T))


# ------------------------------------------------------------------------------------------ bars
def _fro(A):
    return np.sqrt(np.sum(np.asarray(A, dtype=LD) ** 2))


def ratio(got, ref, bar):
    """max |got - ref| / bar; an entry whose bar is 0 must be exact; inf on a shape or NaN mismatch."""
    got = np.asarray(got)
    ref = np.asarray(ref, dtype=LD)
    bar = np.broadcast_to(np.asarray(bar, dtype=LD), ref.shape)
    if got.shape != ref.shape:
        return float("inf")
    err = np.abs(got.astype(LD) - ref)
    if not np.all(np.isfinite(err)):
        return float("inf")
    zero = bar == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float(np.max(err[~zero] / bar[~zero])) if np.any(~zero) else 0.0


class PassReference:
    """M, Q and G'G in long double for given loadings on a given S (real columns p, q; panel widths
    kx, ky free of the model), with their entrywise bars."""

    def __init__(self, S, p, q, Gx, Gy):
        S = np.asarray(S).astype(LD)
        Gx, Gy = np.asarray(Gx).astype(LD), np.asarray(Gy).astype(LD)
        kx, ky = Gx.shape[1], Gy.shape[1]
        gx, gy = gamma(padded_width(p) + 2), gamma(padded_width(q) + 2)
        self.M = np.hstack([S[:, :p] @ Gx, S[:, p:] @ Gy])
        self.bar_M = np.hstack([gx * (np.abs(S[:, :p]) @ np.abs(Gx)), gy * (np.abs(S[:, p:]) @ np.abs(Gy))]) * SLACK
        G = np.zeros((p + q, kx + ky), dtype=LD)
        G[:p, :kx], G[p:, kx:] = Gx, Gy
        gr = np.concatenate([np.full(kx, gx), np.full(ky, gy)])[:, None]     # the Gram sums over the rows column a lives on
        self.Q = G.T @ self.M
        self.bar_Q = (gr * (np.abs(G).T @ np.abs(self.M)) + (1 + gr) * (np.abs(G).T @ self.bar_M)) * SLACK
        self.bar_Q = np.maximum(self.bar_Q, self.bar_Q.T)                    # computed on one triangle, mirrored
        self.GGx, self.GGy = Gx.T @ Gx, Gy.T @ Gy
        self.bar_GGx, self.bar_GGy = gx * (np.abs(Gx).T @ np.abs(Gx)) * SLACK, gy * (np.abs(Gy).T @ np.abs(Gy)) * SLACK

    def ratios(self, M, Q, GGx, GGy):
        return dict(M=ratio(M, self.M, self.bar_M), Q=ratio(Q, self.Q, self.bar_Q),
                    GGx=ratio(GGx, self.GGx, self.bar_GGx), GGy=ratio(GGy, self.GGy, self.bar_GGy))


def small_bars(ref, th, N, p, q, ssqX, ssqY, e_Q=0.0, e_G=0.0):
    """The normwise bars of the module docstring for the small algebra, from the long-double reference
    `ref` (what `small` or `sform` returned) and the Frobenius norms of the bars carried in."""
    r, rx, ry, kx, ky, k = shape(th)
    N = LD(N)
    e_Q, e_G = LD(e_Q), LD(e_G)
    f64 = lambda A: np.asarray(A, dtype=np.float64)
    kL = LD(np.linalg.cond(f64(ref["Lam"])))
    kS = LD(np.linalg.cond(f64(sigma_z(cast(th, LD)))))
    d = LD(max(1 / float(th["sigE"]) ** 2, 1 / float(th["sigF"]) ** 2))
    nLam2 = LD(np.linalg.norm(f64(ref["Lam"]), 2))
    e_L = d * e_G + 8 * U * kS * _fro(ref["Lam"])
    rho = 8 * k * k * U * kL * kS + kL * e_L / nLam2
    e_I = rho * _fro(ref["Li"])
    nK, nQ, nT, nZ = _fro(ref["K"]), _fro(ref["Q"]), _fro(ref["T"]), _fro(ref["Czz"])
    e_K = d * e_I + U * nK
    e_T = e_Q * nK + nQ * e_K + gamma(k + 1) * nQ * nK
    e_Z = e_I + (e_K * nT + nK * e_T + gamma(k + 1) * nK * nT) / N + 2 * U * nZ
    T, Czz = np.asarray(ref["T"], dtype=LD), np.asarray(ref["Czz"], dtype=LD)

    def noise(ssq, sl, GGs, kk, pp):
        return (2 * np.sqrt(LD(kk)) * e_T / N + e_G * nZ + _fro(GGs) * e_Z
                + gamma(kk * kk + 6) * (LD(ssq) / N + 2 * abs(np.trace(T[sl, sl])) / N + np.sum(np.abs(GGs) * np.abs(Czz[sl, sl])))) / pp

    bm = 1 + LD(np.max(np.abs(th["B"])))
    logs = (abs(p * 2 * math.log(th["sigE"])) + abs(q * 2 * math.log(th["sigF"])) + 2 * r * abs(math.log(th["sigH"]))
            + 2 * sum(abs(math.log(v)) for key in ("sigT", "sigTo", "sigUo") for v in np.ravel(th[key])) + abs(ref["logdetL"]))
    e_ll = (N / 2 * (k * (rho + 4 * U) + gamma(3 * k + 8) * LD(logs))
            + (d * np.sqrt(LD(k)) * e_T + gamma(k + 8) * (LD(ssqX) / LD(th["sigE"]) ** 2 + LD(ssqY) / LD(th["sigF"]) ** 2
                                                         + d * np.sum(np.abs(np.diag(T))))) / 2
            + 4 * U * abs(ref["loglik"]))
    return dict(K=e_K * SLACK, Czz=e_Z * SLACK, Cee=noise(ssqX, slice(0, kx), ref["GGx"], kx, p) * SLACK,
                Cff=noise(ssqY, slice(kx, k), ref["GGy"], ky, q) * SLACK,
                Chh=(bm * bm * e_Z + 8 * U * bm * bm * np.max(np.abs(Czz))) * SLACK, loglik=e_ll * SLACK, rho=rho)


def small_ratios(got, ref, bars):
    """Worst err / bar per output of the small algebra (got: a dict with the same keys)."""
    out = {key: ratio(got[key], ref[key], bars[key]) for key in ("K", "Czz", "Chh")}
    for key in ("Cee", "Cff", "loglik"):
        out[key] = ratio(np.array([got[key]]), np.array([ref[key]]), np.array([bars[key]]))
    return out


def raw_update_bar(ref, th, bars, bar_M, N, p, side, stage, W_new=None):
    """Entrywise bar of a raw loading update (module docstring), from the long-double moments."""
    r, rx, ry, kx, ky, k = shape(th)
    N = LD(N)
    M = np.asarray(ref["M"], dtype=LD)
    rows = slice(0, p) if side == 0 else slice(p, M.shape[0])
    zoff = 0 if side == 0 else kx
    c0 = zoff + (r if stage else 0)
    nc = (ry if side else rx) if stage else r
    Kc = np.abs(np.asarray(ref["K"], dtype=LD)[:, c0:c0 + nc])
    Lo = np.abs(np.asarray(W_new if stage else (th["Co"] if side else th["Wo"]), dtype=LD))
    Cto = np.abs(np.asarray(ref["Cuuo" if side else "Ctto"], dtype=LD))
    coef = Cto if stage else Cto.T
    aM = np.abs(M[rows])
    bar = (np.asarray(bar_M, dtype=LD)[rows] @ Kc + aM.sum(axis=1, keepdims=True) * bars["K"] + gamma(k + 2) * (aM @ Kc)) / N
    bar = bar + Lo.sum(axis=1, keepdims=True) * bars["Czz"] + gamma(Lo.shape[1] + 2) * (Lo @ coef)
    return bar * SLACK


# --------------------------------------------------------------------------------- the test data
HOST_SEEDS = (11, 16, 17)          # chosen on the CPU: the fp64 loop alone meets both conditions of the host test
HOST_SHAPE = dict(N=400, p=13, q=9, r=2, rx=2, ry=1)


def host_truth(seed):
    """The true parameters of the recovery problem (a second joint component of b = 1.1 that a
    shared-only fit loses to the stronger X-specific directions)."""
    rng = np.random.default_rng(seed)
    s = HOST_SHAPE
    Gx = np.linalg.qr(rng.standard_normal((s["p"], s["r"] + s["rx"])))[0]
    Gy = np.linalg.qr(rng.standard_normal((s["q"], s["r"] + s["ry"])))[0]
    return dict(W=Gx[:, :s["r"]], Wo=Gx[:, s["r"]:], C=Gy[:, :s["r"]], Co=Gy[:, s["r"]:], B=np.array([1.3, 1.1]),
                sigT=np.array([1.6, 0.9]), sigTo=np.array([2.2, 1.8]), sigUo=np.array([1.5]), sigE=0.5, sigF=0.5, sigH=0.3)


def host_problem(seed):
    """(X, Y, truth) of the recovery problem for one seed, drawn by ppls_amd's simulate_PO2PLS."""
    from ppls_amd.po2 import simulate_PO2PLS
    tr, s = host_truth(seed), HOST_SHAPE
    X, Y = simulate_PO2PLS(s["N"], tr["W"], tr["C"], tr["Wo"], tr["Co"], tr["B"], tr["sigE"], tr["sigF"], tr["sigH"],
                           tr["sigT"], tr["sigTo"], tr["sigUo"], np.random.default_rng(seed + 100))
    return X, Y, tr


def without_specific(th):
    """The same start with rx = ry = 0 (the shared-only model)."""
    out = dict(th)
    out.update(Wo=th["Wo"][:, :0], Co=th["Co"][:, :0], sigTo=th["sigTo"][:0], sigUo=th["sigUo"][:0])
    return out


def start_theta(S, N, p, q, r, rx, ry, seed=0):
    """A deterministic start for the host loops: seeded orthonormal loadings, scalars scaled by the
    data's mean variances."""
    rng = np.random.default_rng(seed)
    Gx = np.linalg.qr(rng.standard_normal((p, r + rx)))[0]
    Gy = np.linalg.qr(rng.standard_normal((q, r + ry)))[0]
    vx, vy = np.trace(S[:p, :p]) / N / p, np.trace(S[p:, p:]) / N / q
    return dict(W=Gx[:, :r], Wo=Gx[:, r:], C=Gy[:, :r], Co=Gy[:, r:], B=np.ones(r), sigT=np.full(r, math.sqrt(vx)),
                sigTo=np.full(rx, math.sqrt(vx)), sigUo=np.full(ry, math.sqrt(vy)), sigE=math.sqrt(vx), sigF=math.sqrt(vy),
                sigH=math.sqrt(vy) / 2)
