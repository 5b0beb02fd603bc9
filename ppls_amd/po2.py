"""Host-side parts of PO2PLS (no GPU): the generator, the variation summary and the canonical form.

The model is the reference's wider one (simulC, Package/PPLS/src/loglC.cpp:268-315):
    x = W t + P_Yosc t_o + e,   y = C u + P_Xosc u_o + f,   u = B t + h,
which the fits of ``ppls_amd.api.PO2PLS`` estimate from the cross-products.
"""
from __future__ import annotations

import numpy as np


def _diagvec(v, n):
    v = np.asarray(v, dtype=np.float64)
    if n == 0:
        return np.zeros(0)
    return np.diag(v).copy() if v.ndim == 2 else np.broadcast_to(np.ravel(v), (n,)).astype(np.float64)


def simulate_PO2PLS(N, W, C, P_Yosc, P_Xosc, B_T, sigX, sigY, sigH, sigT, sigTo, sigUo, rng=None):
    """simulC's model (loglC.cpp:268-315) on the host in numpy: returns (X, Y), N x p and N x q.

    U keeps all r columns (``:309`` declares it a vector, which drops all but the first).  B_T, sigT,
    sigTo, sigUo: diagonal matrices or vectors.  The draws come from ``rng`` (numpy Generator) in the
    reference's order: e, f, t, t_o, u_o, h."""
    rng = rng if rng is not None else np.random.default_rng()
    W, C = np.atleast_2d(np.asarray(W, dtype=np.float64)), np.atleast_2d(np.asarray(C, dtype=np.float64))
    p, q, r = W.shape[0], C.shape[0], W.shape[1]
    Wo = np.asarray(P_Yosc, dtype=np.float64).reshape(p, -1) if P_Yosc is not None else np.zeros((p, 0))
    Co = np.asarray(P_Xosc, dtype=np.float64).reshape(q, -1) if P_Xosc is not None else np.zeros((q, 0))
    rx, ry = Wo.shape[1], Co.shape[1]
    E = sigX * rng.standard_normal((N, p))
    F = sigY * rng.standard_normal((N, q))
    T = rng.standard_normal((N, r)) * _diagvec(sigT, r)
    To = rng.standard_normal((N, rx)) * _diagvec(sigTo, rx)
    Uo = rng.standard_normal((N, ry)) * _diagvec(sigUo, ry)
    H = sigH * rng.standard_normal((N, r))
    U = T * _diagvec(B_T, r) + H
    return T @ W.T + To @ Wo.T + E, U @ C.T + Uo @ Co.T + F


def canonical_PO2PLS(est):
    """The canonical form a fit is returned in: the joint part by PPLS_simult's sign and order rule
    (EM_W_multi.R:794-799), the specific components by decreasing sigma, each specific column's sign
    so that its sum is >= 0.  ``est``: dict(W, Wo, C, Co, B, sigT, sigTo, sigUo, sigE, sigF, sigH) with
    diagonal matrices or vectors; returns the same keys with diagonal matrices."""
    W, C = np.array(est["W"], dtype=np.float64), np.array(est["C"], dtype=np.float64)
    r = W.shape[1]
    B, T = _diagvec(est["B"], r), _diagvec(est["sigT"], r)
    sg = np.sign(T * B)
    rot = np.argsort(-(T * (B * sg)), kind="stable")
    out = dict(est)
    out.update(W=W[:, rot] * sg, C=C[:, rot] * sg, B=np.diag((B * sg)[rot]), sigT=np.diag(T[rot]))
    for L, s in (("Wo", "sigTo"), ("Co", "sigUo")):
        A = np.array(est[L], dtype=np.float64).reshape(out["W" if L == "Wo" else "C"].shape[0], -1)
        sv = _diagvec(est[s], A.shape[1])
        o = np.argsort(-sv, kind="stable")
        A = A[:, o]
        out[L] = A * np.where(A.sum(axis=0) < 0, -1.0, 1.0) if A.shape[1] else A
        out[s] = np.diag(sv[o])
    return out


def summary_PO2PLS(fit):
    """Shares of joint, specific and noise variation in X and Y implied by the estimates:
        var X = tr(W sigT^2 W') + tr(Wo sigTo^2 Wo') + p sigE^2,
        var Y = tr(C (sigT^2 B^2 + sigH^2) C') + tr(Co sigUo^2 Co') + q sigF^2,
    and the share of Y's joint part that X predicts (sigT^2 B^2 against sigT^2 B^2 + sigH^2).
    Loadings need not be orthonormal.  Returns dict(X=dict(joint, specific, noise, total),
    Y=dict(...), predictable=...); the three shares of a block sum to 1."""
    e = fit["estimates"] if "estimates" in fit else fit
    W, C = np.asarray(e["W"], dtype=np.float64), np.asarray(e["C"], dtype=np.float64)
    p, q, r = W.shape[0], C.shape[0], W.shape[1]
    Wo, Co = np.asarray(e["Wo"], dtype=np.float64).reshape(p, -1), np.asarray(e["Co"], dtype=np.float64).reshape(q, -1)
    B, T = _diagvec(e["B"], r), _diagvec(e["sigT"], r)
    To, Uo = _diagvec(e["sigTo"], Wo.shape[1]), _diagvec(e["sigUo"], Co.shape[1])
    sE, sF, sH = (float(np.ravel(e[k])[0]) for k in ("sigE", "sigF", "sigH"))
    cn = lambda L: np.sum(L * L, axis=0)   # squared column norms: tr(L D L') = sum_j d_j ||L_j||^2
    jx, sx, nx = float(cn(W) @ T ** 2), float(cn(Wo) @ To ** 2), p * sE ** 2
    jy_pred, jy_h = float(cn(C) @ (T ** 2 * B ** 2)), float(cn(C).sum() * sH ** 2)
    sy, ny = float(cn(Co) @ Uo ** 2), q * sF ** 2
    tx, ty = jx + sx + nx, jy_pred + jy_h + sy + ny
    return dict(X=dict(joint=jx / tx, specific=sx / tx, noise=nx / tx, total=tx),
                Y=dict(joint=(jy_pred + jy_h) / ty, specific=sy / ty, noise=ny / ty, total=ty),
                predictable=jy_pred / (jy_pred + jy_h))
