"""Reference, a-priori error bars and a host model of the PO2PLS row diagnostics kernel, shared by
tests/test_po2_rowdiag_host.py and tests/test_gpu_po2_rowdiag.py.

The model is po2_bar's: x = W t + Wo to + e, y = C u + Co uo + f, u = B t + h; Gx = [W Wo] (kx columns),
Gy = [C Co] (ky), z = (t, to | u, uo), k = kx + ky.  The loadings need not be orthonormal.

References, both in long double from the fp64 values passed (for fp32 storage over the rows rounded to fp32):

* ``dense_reference``: d2 = d' Sigma^-1 d and loglik through the dense (p+q) x (p+q) covariance of
  po2_bar.dense_cov and its Gauss-Jordan inverse, mu = d' Sigma^-1 G Sigma_z (small shapes only).
* ``reference``: the closed form.  Gx = Qx Rx, Gy = Qy Ry (Householder, R's diagonal positive), a = Qx'x,
  b = Qy'y, R = blockdiag(Rx, Ry), Sigma_c = R Sigma_z R' + diag(sE2 I_kx, sF2 I_ky):
      odx2 = ||x - Qx a||^2, ody2 = ||y - Qy b||^2, sd2 = c' Sigma_c^-1 c with c = (a; b),
      d2 = odx2 / sE2 + ody2 / sF2 + sd2, mu = c' Sigma_c^-1 R Sigma_z,
      loglik = -((p+q) log 2 pi + (p-kx) log sE2 + (q-ky) log sF2 + log|Sigma_c|) / 2 - d2 / 2.

The kernel's order and the bars (``bars``), with u = 2^-53 and gamma(n) = n u / (1 - n u); the constants K_* not
listed here are rowdiag_bar's, with the same meaning.  Nothing is measured.

* host QR.  Householder QR in fp64 gives Qh = Q + dQ with ||dQ||_2 <= eps and ||Rh - R||_2 <= eps ||R||_2,
      eps(n, c) = sqrt(c) gamma(K_QR n c),  K_QR = 6
  (Higham, Accuracy and Stability, Thm 19.4 and (19.13): columnwise gamma~_{nc}; its constant is a small
  integer -- applying a reflector costs about 4 n operations per column -- and sqrt(c) turns the columnwise
  bound into a 2-norm).  So Qh'Qh - I is at most 2 eps + eps^2 in norm.
* scores.  As rowdiag_bar (lane partial of L1 terms, the six-level tree) plus what dQ moves them:
      Ea_m = gamma(L1 + K_TREE) sum_j |x_j| |q_jm| + eps ||x||.
* residual.  rowdiag_bar's de (k_b + 1 roundings behind a term of x - sum_m a_m q_m, and the error of the
  scores carried through) and the change of the projector, ||(Qh Qh' - Q Q') x|| <= (2 eps + eps^2) ||x||:
      nde = ||de|| + (2 eps + eps^2) ||x||,
      bar(odx2) = gamma(L1 + sweeps + K_TREE + 1) (||e|| + nde)^2 + 2 ||e|| nde + nde^2.
* Uc.  The library forms Sigma_c from Rh (relative change at most 2 eps_max + eps_max^2 in norm, eps_max the
  larger of the two blocks'), factors it by Cholesky and inverts the triangle.  As po2_bar's rho (Higham Thm
  10.3 / 10.4: a Cholesky solve errs by (3k + 1) k u kappa relatively, the explicit inverse is two solves per
  column), with kC = kappa_2(Sigma_c):
      rho = (c(k) u + 4 eps_max) kC,  c(k) = 8 k^2        (relative error of Uc'Uc against Sigma_c^-1)
* sd2 = ||Uc c||^2.  Lane i adds the k products of row i in order (k roundings, a product each), squares, and
  the squares meet in a five-level tree: with Ec = (Ea; Eb) and S2 = ||Sigma_c^-1||_2
      bar(sd2) = rho S2 ||c||^2 + S2 (2 ||c|| ||Ec|| + ||Ec||^2) + gamma(2 (k + 1) + 1 + 5) sum_i (|Uc| |c|)_i^2.
* mu = c' Kmu, Kmu = Uc' (Uc (R Sigma_z)): three k-term products behind an entry of Kmu and the errors of
  Uc'Uc and Rh; lane 32 + i adds k products in order:
      e_K = (rho + 2 eps_max + gamma(3 k + 2)) S2 ||R||_2 ||Sigma_z||_2            (2-norm of a column's error)
      bar(mu_i) = sum_j Ec_j |Kmu_ji| + e_K (||c|| + ||Ec||) + gamma(k + 1) sum_j |c_j| |Kmu_ji|.
* d2.  rowdiag_bar's: bar(odx2) / sE2 + bar(ody2) / sF2 + bar(sd2) + gamma(K_D2) (odx2 / sE2 + ody2 / sF2 + sd2).
* loglik = cst - d2 / 2.  log|Sigma_c| from the Cholesky diagonal moves by at most k times the relative
  perturbation of the eigenvalues (po2_bar's e_ll):
      bar(loglik) = bar(d2) / 2 + k (rho + 4 u) / 2 + gamma(K_CST + k) |cst|_abs + gamma(K_FORM) (p + q) / 2
                    + 2 u |loglik|.
"""
import math

import numpy as np

import po2_bar
import rowdiag_bar
import sweep_bar
from finalize_bar import householder_qr, inverse
from rowdiag_bar import K_CST, K_D2, K_FORM, K_TREE, gamma, lane_terms, stored

L = sweep_bar.LD
U = rowdiag_bar.U
K_QR = 6

SIZES = [(1, 0, 0), (1, 1, 0), (1, 0, 1), (2, 2, 1), (5, 3, 0), (4, 4, 5), (3, 5, 13), (8, 8, 8)]
OUTPUTS = ("odx2", "ody2", "sd2", "d2", "loglik", "mu")
WIDE_X = [(37, 41, 37, 8, 1, 0, False), (37, 41, 37, 5, 4, 0, True), (33, 261, 130, 8, 1, 0, True), (33, 261, 130, 5, 4, 0, False)]
DENSE_MAX = 200      # p + q up to which the dense reference is formed (Gauss-Jordan in long double)


def tile_of(kb):
    return 8 if kb <= 8 else 16


def rows_per_wave(kx, ky, p, q, f32):
    """ppls_po2_rowdiag_rows_per_wave: rowdiag_bar's rule at the wider block."""
    return rowdiag_bar.rows_per_wave(max(kx, ky), p, q, f32)


def qr_pos(G):
    """Householder QR in long double with R's diagonal positive."""
    Q, R = householder_qr(np.asarray(G).astype(L))
    s = np.where(np.diag(R) < 0, L(-1), L(1))
    return Q * s, R * s[:, None]


def sigma_c(th, Rx, Ry):
    """(Sigma_c, R, Sigma_z) in the dtype of Rx."""
    r, rx, ry, kx, ky, k = po2_bar.shape(th)
    dt = Rx.dtype.type
    R = np.zeros((k, k), dtype=Rx.dtype)
    R[:kx, :kx], R[kx:, kx:] = Rx, Ry
    Sz = po2_bar.sigma_z(po2_bar.cast(th, dt))
    Sc = R @ Sz @ R.T
    Sc = (Sc + Sc.T) / 2
    Sc[np.arange(kx), np.arange(kx)] += dt(th["sigE"]) ** 2
    Sc[kx + np.arange(ky), kx + np.arange(ky)] += dt(th["sigF"]) ** 2
    return Sc, R, Sz


def _cst(th, p, q, logdet_c, dt):
    r, rx, ry, kx, ky, k = po2_bar.shape(th)
    terms = [dt(p + q) * po2_bar._log2pi(dt), dt(p - kx) * 2 * np.log(dt(th["sigE"])), dt(q - ky) * 2 * np.log(dt(th["sigF"])),
             logdet_c]
    return -(terms[0] + terms[1] + terms[2] + terms[3]) / dt(2), float(sum(abs(t) for t in terms)) / 2


def reference(X, Y, th, f32=False):
    """Every output by the closed form in long double (module docstring), with the pieces the bars need."""
    th = po2_bar.cast(th, L)
    Gx, Gy = po2_bar.loadings(th)
    p, q = Gx.shape[0], Gy.shape[0]
    Xl, Yl = stored(X, f32).astype(L), stored(Y, f32).astype(L)
    Qx, Rx = qr_pos(Gx)
    Qy, Ry = qr_pos(Gy)
    a, b = Xl @ Qx, Yl @ Qy
    ex, ey = Xl - a @ Qx.T, Yl - b @ Qy.T
    odx2, ody2 = (ex * ex).sum(axis=1), (ey * ey).sum(axis=1)
    Sc, R, Sz = sigma_c(th, Rx, Ry)
    Sci = inverse(Sc)
    Sci = (Sci + Sci.T) / 2
    c = np.hstack([a, b])
    sd2 = ((c @ Sci) * c).sum(axis=1)
    Kmu = Sci @ R @ Sz
    sE2, sF2 = th["sigE"] ** 2, th["sigF"] ** 2
    d2 = odx2 / sE2 + ody2 / sF2 + sd2
    cst, cabs = _cst(th, p, q, po2_bar._logdet_spd(Sc), L)
    return dict(odx2=odx2, ody2=ody2, sd2=sd2, d2=d2, loglik=cst - d2 / 2, mu=c @ Kmu, a=a, b=b, c=c, Qx=Qx, Qy=Qy, R=R,
                Sz=Sz, Sc=Sc, Sci=Sci, Kmu=Kmu, cst=cst, cabs=cabs, ex=ex, ey=ey)


def dense_reference(X, Y, th, f32=False):
    """d2, loglik and mu through the dense covariance and its inverse (no QR, no Sigma_c)."""
    th = po2_bar.cast(th, L)
    Sig, G = po2_bar.dense_cov(th)
    D = np.hstack([stored(X, f32).astype(L), stored(Y, f32).astype(L)])
    Si = inverse(Sig)
    Si = (Si + Si.T) / 2
    d2 = ((D @ Si) * D).sum(axis=1)
    P = Sig.shape[0]
    ll = -L(0.5) * P * po2_bar._log2pi(L) - L(0.5) * po2_bar._logdet_spd(Sig) - d2 / 2
    return dict(d2=d2, loglik=ll, mu=D @ Si @ G @ po2_bar.sigma_z(th))


def qr_eps(n, c):
    return math.sqrt(c) * float(gamma(K_QR * n * c))


def _block_bar(Xs, Q, f32, eps, dX=None):
    """(Ea n x kb, bar of the squared residual norm n) of one block: rowdiag_bar._block_bar's terms (its input
    perturbation ``dX`` included) and the host QR's (module docstring)."""
    kb = Q.shape[1]
    L1, sweeps, _ = lane_terms(Xs.shape[1], f32)
    Xl = Xs.astype(L)
    aX, aQ = np.abs(Xl), np.abs(Q)
    nx = np.sqrt((Xl * Xl).sum(axis=1))
    a = Xl @ Q
    Ea = gamma(L1 + K_TREE) * (aX @ aQ) + eps * nx[:, None]
    de = gamma(kb + 1) * (aX + (np.abs(a) + Ea) @ aQ.T) + Ea @ aQ.T
    if dX is not None:
        dXl = np.asarray(dX, dtype=np.float64).astype(L)
        Ea = Ea + dXl @ aQ
        de = de + dXl + (dXl @ aQ) @ aQ.T
    e = Xl - a @ Q.T
    ne = np.sqrt((e * e).sum(axis=1))
    nde = np.sqrt((de * de).sum(axis=1)) + (2 * eps + eps * eps) * nx
    return Ea, gamma(L1 + sweeps + K_TREE + 1) * (ne + nde) ** 2 + 2 * ne * nde + nde ** 2


def bars(X, Y, th, f32=False, ref=None, dX=None, dY=None):
    """The a-priori bar of every output as float64 arrays (module docstring).  ``dX``, ``dY``: elementwise bounds
    on an input perturbation, as rowdiag_bar.bars takes them."""
    ref = reference(X, Y, th, f32) if ref is None else ref
    r, rx, ry, kx, ky, k = po2_bar.shape(th)
    p, q = X.shape[1], Y.shape[1]
    ex_, ey_ = qr_eps(p, kx), qr_eps(q, ky)
    em = max(ex_, ey_)
    Ea, bx = _block_bar(stored(X, f32), ref["Qx"], f32, ex_, dX)
    Eb, by = _block_bar(stored(Y, f32), ref["Qy"], f32, ey_, dY)
    f64 = lambda A: np.asarray(A, dtype=np.float64)   # noqa: E731
    kC = L(np.linalg.cond(f64(ref["Sc"])))
    S2 = L(np.linalg.norm(f64(ref["Sci"]), 2))
    rho = (8 * k * k * U + 4 * em) * kC
    c, Ec = ref["c"], np.hstack([Ea, Eb])
    nc, nEc = np.sqrt((c * c).sum(axis=1)), np.sqrt((Ec * Ec).sum(axis=1))
    Uc = np.abs(np.linalg.cholesky(f64(ref["Sci"])).T).astype(L)   # Sigma_c^-1 = Uc'Uc, Uc upper
    bsd = rho * S2 * nc ** 2 + S2 * (2 * nc * nEc + nEc ** 2) + gamma(2 * (k + 1) + 6) * ((np.abs(c) @ Uc.T) ** 2).sum(axis=1)
    aK = np.abs(ref["Kmu"])
    e_K = (rho + 2 * em + gamma(3 * k + 2)) * S2 * L(np.linalg.norm(f64(ref["R"]), 2)) * L(np.linalg.norm(f64(ref["Sz"]), 2))
    bmu = Ec @ aK + (e_K * (nc + nEc))[:, None] + gamma(k + 1) * (np.abs(c) @ aK)
    sE2, sF2 = L(th["sigE"]) ** 2, L(th["sigF"]) ** 2
    bd2 = bx / sE2 + by / sF2 + bsd + gamma(K_D2) * (ref["odx2"] / sE2 + ref["ody2"] / sF2 + np.abs(ref["sd2"]))
    bll = bd2 / 2 + k * (rho + 4 * U) / 2 + gamma(K_CST + k) * ref["cabs"] + gamma(K_FORM) * (p + q) / 2 + 2 * U * np.abs(ref["loglik"])
    return dict(odx2=f64(bx), ody2=f64(by), sd2=f64(bsd), d2=f64(bd2), loglik=f64(bll), mu=f64(bmu))


def loglik_sum_bar(X, Y, th, f32=False, ref=None, br=None):
    """Bar of sum_i loglik_i against ppls_po2_loglik on S = Z'Z of the same n rows: the rows' own bars, the n
    additions of the sum, and the entry's own error -- S is a sum of n products per entry and the entry
    contracts it with Sigma^-1 in pieces: K_ENTRY stages of gamma(n + p + q) of the absolute sum
    (||X||_F^2 / sE2 + ||Y||_F^2 / sF2 + S2 sum_i ||c_i||^2) / 2 + n |cst|_abs, as rowdiag_bar.loglik_sum_bar
    counts an existing entry, plus §26's a-priori bar e_ll on l (po2_bar.small_bars with the pass's bars carried in)."""
    ref = reference(X, Y, th, f32) if ref is None else ref
    br = bars(X, Y, th, f32, ref) if br is None else br
    n, p, q = X.shape[0], X.shape[1], Y.shape[1]
    Xs, Ys = stored(X, f32).astype(L), stored(Y, f32).astype(L)
    sE2, sF2 = L(th["sigE"]) ** 2, L(th["sigF"]) ** 2
    S2 = L(np.linalg.norm(np.asarray(ref["Sci"], dtype=np.float64), 2))
    mag = ((Xs * Xs).sum() / sE2 + (Ys * Ys).sum() / sF2 + S2 * (ref["c"] ** 2).sum()) / 2 + n * ref["cabs"]
    Z = np.hstack([Xs, Ys])
    S = Z.T @ Z
    sref = po2_bar.sform(th, S, n, p, q)
    pr = po2_bar.PassReference(S, p, q, *po2_bar.loadings(th))
    e_G = np.sqrt(po2_bar._fro(pr.bar_GGx) ** 2 + po2_bar._fro(pr.bar_GGy) ** 2)
    e_ll = po2_bar.small_bars(sref, th, n, p, q, np.trace(S[:p, :p]), np.trace(S[p:, p:]), po2_bar._fro(pr.bar_Q), e_G)["loglik"]
    return float(br["loglik"].sum() + gamma(n) * np.abs(ref["loglik"]).sum() + rowdiag_bar.K_ENTRY * gamma(n + p + q) * mag + e_ll)


inside = rowdiag_bar.inside


def robust_reference(ref, th, nus, keep, p, q, N):
    """w (for nus[keep]) and l_t (per nu) in long double from the reference's d2, as robust_bar.reference forms
    them; logdet = -2 cst - (p + q) log 2 pi."""
    import robust_bar
    P = p + q
    nus = [float(v) for v in np.atleast_1d(nus)]
    d2 = ref["d2"]
    logdet = -2 * ref["cst"] - L(P) * po2_bar._log2pi(L)
    w = (L(nus[keep]) + L(P)) / (L(nus[keep]) + d2)
    ll = np.array([L(N) * L(robust_bar.t_constant(v, P)[0]) - L(N) / 2 * logdet - (L(v) + L(P)) / 2 * np.log1p(d2 / L(v)).sum()
                   for v in nus], dtype=L)
    return dict(w=w, loglik_t=ll)


def robust_bars(ref, br, th, nus, keep, p, q, N):
    """robust_bar.bars with this module's bar on d2 and on logdet (k (rho + 4 u) + gamma(K_CST + k) |logdet|_abs +
    gamma(K_FORM) (p + q): bar(loglik)'s constant terms, doubled)."""
    import robust_bar as rob
    P, n = p + q, ref["d2"].shape[0]
    nus = [float(v) for v in np.atleast_1d(nus)]
    bd2 = br["d2"]
    d2 = np.asarray(ref["d2"], dtype=np.float64)
    assert np.all(bd2 < min(nus) + d2)
    nk = nus[keep]
    w = (nk + P) / (nk + d2)
    bw = w * (bd2 / (nk + d2 - bd2) + gamma(rob.K_WT))
    ll_const = np.asarray(br["loglik"] - br["d2"] / 2 - 2 * U * np.abs(np.asarray(ref["loglik"], dtype=np.float64)))
    bld = 2 * float(ll_const.max())                    # the bar of logdet: the same for every row
    ldabs = 2 * ref["cabs"]
    bl = []
    for v in nus:
        t = np.log1p(d2 / v)
        b = float((bd2 / (v + d2 - bd2) + gamma(rob.K_LOG) * t).sum() + gamma(rob.depth(n)) * t.sum())
        cabs = rob.t_constant(v, P)[1]
        bl.append(0.5 * (v + P) * b + N * gamma(rob.K_LG) * cabs + 0.5 * N * bld +
                  gamma(rob.K_LL) * (N * cabs + 0.5 * N * ldabs + 0.5 * (v + P) * float(t.sum())))
    return dict(w=bw, loglik_t=np.array(bl))


# ------------------------------------------------------------------------------------ host model
def host_model(X, Y, th, f32=False, want_mu=True, defect=None):
    """The kernel's outputs and the library's d2, loglik from a plain fp64 evaluation in the kernel's and the
    host algebra's order.  ``defect``: None or one of "gram_forgotten", "coupling_sign", "y_offset",
    "drop_unit", "expand_x" (tests/test_po2_rowdiag_host.py)."""
    th = po2_bar.cast(th, np.float64)
    r, rx, ry, kx, ky, k = po2_bar.shape(th)
    Gx, Gy = po2_bar.loadings(th)
    p, q = Gx.shape[0], Gy.shape[0]

    def qr64(G):
        Q, R = np.linalg.qr(G)
        s = np.where(np.diag(R) < 0, -1.0, 1.0)
        return Q * s, R * s[:, None]

    Qx, Rx = qr64(Gx)
    Qy, Ry = qr64(Gy)
    rw = rows_per_wave(kx, ky, p, q, f32)
    Xs, Ys = stored(X, f32), stored(Y, f32)
    a, ox = rowdiag_bar._model_block(Xs, Qx, f32, rw * tile_of(kx), defect == "drop_unit", defect == "expand_x")
    b, oy = rowdiag_bar._model_block(Ys, Qy, f32, rw * tile_of(ky), defect == "drop_unit")
    if defect == "gram_forgotten":                    # x - Gx (Gx'x): (G'G)^-1 forgotten
        ex = Xs - (Xs @ Gx) @ Gx.T
        ox = (ex * ex).sum(axis=1)
    th_z = dict(th)
    if defect == "coupling_sign":
        th_z["B"] = -th["B"]
    Sc, R, Sz = sigma_c(th_z, Rx, Ry)
    Lr = np.linalg.cholesky(Sc[::-1, ::-1])
    Uc = np.linalg.inv(Lr)[::-1, ::-1]                # upper: Sigma_c^-1 = Uc'Uc
    Uc = np.triu(Uc)
    Kmu = Uc.T @ (Uc @ (R @ Sz))
    n = Xs.shape[0]
    c = np.zeros((n, k))
    c[:, :kx] = a
    if defect == "y_offset":                          # the Y block at offset ky instead of kx
        m = min(ky, k - ky)
        c[:, ky:ky + m] = b[:, :m]
    else:
        c[:, kx:] = b
    v = np.zeros((n, 32))
    mu = np.zeros((n, k))
    for j in range(k):                                # one accumulator per lane, j ascending
        v[:, :k] = v[:, :k] + Uc[:, j][None, :] * c[:, j][:, None]
        mu = mu + Kmu[j][None, :] * c[:, j][:, None]
    sd2 = rowdiag_bar._tree(v * v, 32)
    sE2, sF2 = th["sigE"] * th["sigE"], th["sigF"] * th["sigF"]
    logdet_c = 2.0 * np.log(np.diag(Lr)).sum()
    cst = -0.5 * ((p + q) * math.log(6.283185307179586) + (((p - kx) * math.log(sE2) + (q - ky) * math.log(sF2)) + logdet_c))
    out = dict(odx2=ox, ody2=oy, sd2=sd2, mu=mu)
    out["d2"] = (ox / sE2 + oy / sF2) + sd2
    out["loglik"] = cst - 0.5 * out["d2"]
    if not want_mu:
        out.pop("mu")
    return out


# ------------------------------------------------------------------------------------ test data
def fits(p, q, r, rx, ry):
    return r + rx <= min(16, p) and r + ry <= min(16, q)


def cases():
    """Every (n, p, q, r, rx, ry, orthonormal) of rowdiag_bar.SHAPES x SIZES that fits, with orthonormal and with
    plain normal loadings (make_theta(..., orthonormal=False, scale=2.0)), and WIDE_X: SIZES has no kx > 8 with
    ky <= 8, so these are the only cases on the (16, 8) tile pair."""
    return [(n, p, q, r, rx, ry, orth) for (n, p, q) in rowdiag_bar.SHAPES for (r, rx, ry) in SIZES if fits(p, q, r, rx, ry)
            for orth in (True, False)] + WIDE_X


def case_id(c):
    return "n{}-p{}-q{}-r{}-{}-{}-{}".format(*c[:6], "orth" if c[6] else "plain")


def draw_rows(rng, th, n):
    """n rows from the model at theta (a dict of po2_bar's shapes)."""
    r, rx, ry, kx, ky, k = po2_bar.shape(th)
    p, q = th["W"].shape[0], th["C"].shape[0]
    T = rng.standard_normal((n, r)) * th["sigT"]
    To = rng.standard_normal((n, rx)) * th["sigTo"]
    Uu = T * th["B"] + th["sigH"] * rng.standard_normal((n, r))
    Uo = rng.standard_normal((n, ry)) * th["sigUo"]
    X = T @ th["W"].T + To @ th["Wo"].T + th["sigE"] * rng.standard_normal((n, p))
    Y = Uu @ th["C"].T + Uo @ th["Co"].T + th["sigF"] * rng.standard_normal((n, q))
    return X, Y


def make_case(n, p, q, r, rx, ry, orthonormal=True, seed=0, sigE=None):
    """(X, Y, theta dict): po2_bar.make_theta's theta (every second b negative, the specific sigmas decaying
    geometrically) and rows drawn from it."""
    rng = np.random.default_rng([seed, n, p, q, r, rx, ry, int(orthonormal)])
    th = po2_bar.make_theta(rng, p, q, r, rx, ry, orthonormal=orthonormal, scale=2.0)
    th["B"] = th["B"] * np.where(np.arange(r) % 2 == 0, 1.0, -1.0)
    th["sigTo"], th["sigUo"] = 1.1 * np.exp(-0.1 * np.arange(rx)), 0.9 * np.exp(-0.1 * np.arange(ry))   # above 0 for 13 columns
    if sigE is not None:
        th["sigE"] = sigE
    X, Y = draw_rows(rng, th, n)
    return X, Y, th


def theta_of(th):
    from ppls_amd import Po2Theta
    return Po2Theta.from_dict(th)


def planted(seed=20261021):
    """The planted-outlier data of the GPU test: n = 203, p = 37, q = 21, (r, rx, ry) = (2, 2, 1) drawn from the
    model at orthonormal loadings, then row 5 moved 12 sigE off the X plane, row 77 12 sigF off the Y plane and
    row 150 8 sqrt(sigTo_1^2 + sigE^2) along wo_1.  Returns X, Y, theta (dict) and the planted rows by statistic."""
    n, p, q, r, rx, ry = 203, 37, 21, 2, 2, 1
    rng = np.random.default_rng(seed)
    th = po2_bar.make_theta(rng, p, q, r, rx, ry)
    th.update(sigE=0.3, sigF=0.4, sigH=0.2)
    X, Y = draw_rows(rng, th, n)
    Gx, Gy = po2_bar.loadings(th)
    u, v = rng.standard_normal(p), rng.standard_normal(q)
    for _ in range(2):
        u -= Gx @ (Gx.T @ u)
        v -= Gy @ (Gy.T @ v)
    X[5] += 12 * th["sigE"] * u / np.linalg.norm(u)
    Y[77] += 12 * th["sigF"] * v / np.linalg.norm(v)
    X[150] += 8 * math.sqrt(th["sigTo"][0] ** 2 + th["sigE"] ** 2) * th["Wo"][:, 0]
    return X, Y, th, dict(odx2=5, ody2=77, sd2=150)


# ------------------------------------------------------------------------------------ the robust loop
def contaminated(seed):
    """po2_bar.host_problem(seed) with 16 of its 400 rows replaced by 4 N(0, 1): (X, Y, truth, bad rows)."""
    X, Y, tr = po2_bar.host_problem(seed)
    X, Y = X.copy(), Y.copy()
    g = np.random.default_rng(seed + 7)
    bad = g.choice(400, 16, replace=False)
    X[bad] = 4 * g.standard_normal((16, 13))
    Y[bad] = 4 * g.standard_normal((16, 9))
    return X, Y, tr, bad


def row_d2(X, Y, th, dt=np.float64):
    """d2 per row by the closed form in ``dt`` (numpy's QR in fp64, Householder in long double)."""
    thc = po2_bar.cast(th, dt)
    Gx, Gy = po2_bar.loadings(thc)
    if dt == L:
        (Qx, Rx), (Qy, Ry) = qr_pos(Gx), qr_pos(Gy)
    else:
        (Qx, Rx), (Qy, Ry) = np.linalg.qr(Gx), np.linalg.qr(Gy)
    Xd, Yd = np.asarray(X).astype(dt), np.asarray(Y).astype(dt)
    a, b = Xd @ Qx, Yd @ Qy
    ex, ey = Xd - a @ Qx.T, Yd - b @ Qy.T
    Sc = sigma_c(thc, Rx, Ry)[0]
    Sci = inverse(Sc) if dt == L else np.linalg.inv(Sc)
    c = np.hstack([a, b])
    return (ex * ex).sum(axis=1) / thc["sigE"] ** 2 + (ey * ey).sum(axis=1) / thc["sigF"] ** 2 + ((c @ Sci) * c).sum(axis=1)


def robust_loop(X, Y, th0, nu, outer, inner, dt=np.float64, type="SVD"):
    """The t-model loop written out: per outer iteration d2 at theta, u_i = (nu + p + q) / (nu + d2_i),
    S_u = sum u_i d_i d_i' and ``inner`` forced ECM steps on S_u with N = n; returns (theta, weights at theta)."""
    n, p, q = X.shape[0], X.shape[1], Y.shape[1]
    Z = np.hstack([X, Y]).astype(dt)
    th = po2_bar.cast(th0, dt)
    for _ in range(outer):
        w = dt(nu + p + q) / (dt(nu) + row_d2(X, Y, th, dt))
        S = (Z * w[:, None]).T @ Z
        for _ in range(inner):
            th = po2_bar.ecm_update(th, po2_bar.sform(th, S, n, p, q, dt), p, dt, type)
    return th, dt(nu + p + q) / (dt(nu) + row_d2(X, Y, th, dt))
