"""Host-side parts of PO2PLS (no GPU): the generator, the variation summary, the canonical form, the prediction
map and the grid selection rule of the cross-validation.

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


def po2_predict_map(estimates, XorY="X"):
    """The linear map of a PO2PLS fit's prediction (``ppls_po2_predict_map``; host only).

    ``XorY="X"``: (L, Bp) with E[y | x] = C diag(Bp) L'x, L (p x r) the first r columns of
    Gx (diag(sigT, sigTo)^-2 + Gx'Gx / sigE^2)^-1 / sigE^2, Gx = [W Wo], and Bp = B.
    ``XorY="Y"``: (L, Bp) with E[x | y] = W diag(1 / Bp) L'y, L (q x r) from Gy = [C Co], sigF and the
    marginal variances sigT^2 b^2 + sigH^2, sigUo^2 of (u, uo); Bp = 1 / beta,
    beta_j = sigT_j^2 b_j / (sigT_j^2 b_j^2 + sigH^2).
    ``estimates``: a PO2PLS fit, its ``estimates`` dict or a ``Po2Theta``."""
    import ctypes as ct

    from . import _lib
    xy = XorY if isinstance(XorY, str) else XorY[0]
    if xy not in ("X", "Y"):
        raise ValueError("'arg' should be one of \"X\", \"Y\"")
    if isinstance(estimates, _lib.Po2Theta):
        th = estimates
    else:
        th = _lib.Po2Theta.from_dict(estimates["estimates"] if "estimates" in estimates else estimates)
    p, q, r = th.W.shape[0], th.C.shape[0], th.r
    L = np.zeros((q if xy == "Y" else p, r), order="F")
    Bp = np.zeros(r)
    ts = th.struct()
    rc = _lib.lib().ppls_po2_predict_map(ct.byref(ts), r, th.rx, th.ry, p, q, int(xy == "Y"), _lib.dptr(L), _lib.dptr(Bp))
    if rc != 0:
        raise _lib.PplsError(rc, "ppls_po2_predict_map: " + {-1: "sizes, a NULL loading, a non-finite value or a sigma not above 0",
                                                              -3: "Lambda is not positive definite, or an entry of B is 0"}.get(rc, ""))
    return L, Bp


# Cells of a cross-validation grid whose fold-mean errors differ by less than this relative amount count as
# equal (the mean of K roots of sums carries a few roundings; 64 u is far below any difference a model makes).
GRID_TIE = 64 * 2.0 ** -53


def select_grid_PO2PLS(per_fold, failed):
    """The selection rule of ``crossval_PO2PLS`` on its arrays: ``per_fold`` (K x nr x nrx x nry) the RMSEP
    of every fold and cell, ``failed`` (same shape, bool) where a start or fit failed.  Returns
    (errors, which_error): ``errors`` the fold mean, NaN for a cell with any failed (or NaN) fold;
    ``which_error`` the index triple of the first cell in grid order (C order: r slowest) whose error is
    within ``GRID_TIE`` (relative) of the minimum over the finite cells -- so ties go to the cell listed
    first -- or None when no cell is finite."""
    per_fold = np.asarray(per_fold, dtype=np.float64)
    failed = np.asarray(failed, dtype=bool)
    if per_fold.ndim != 4 or failed.shape != per_fold.shape:
        raise ValueError("per_fold and failed must be K x nr x nrx x nry")
    bad = np.any(failed | ~np.isfinite(per_fold), axis=0)
    errors = np.where(bad, np.nan, np.mean(np.where(bad[None], 0.0, per_fold), axis=0))
    if np.all(bad):
        return errors, None
    lo = np.nanmin(errors)
    hit = np.flatnonzero(np.ravel(~bad) & (np.ravel(np.nan_to_num(errors, nan=np.inf)) <= lo * (1.0 + GRID_TIE)))
    return errors, tuple(int(v) for v in np.unravel_index(hit[0], errors.shape))


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
