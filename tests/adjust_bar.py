"""References, a-priori error bars and host models of the covariate adjustment, shared by
tests/test_adjust_host.py and tests/test_gpu_adjust.py.  u = 2^-53, gamma(m) = m u / (1 - m u).

Coefficient pass.  G = Q'D: a thread adds the rows of its row block in row order, one fma per row and
(a, j); the row blocks' partials are added in block order; ranks add once more.  Behind any term stand at
most c(n) = ceil(n / nblocks) + nblocks + ranks + 2 roundings (the product's -- absent under fma -- and two
spare), so
    |delta G_aj| <= gamma(c(n)) sum_i |q_ia d_ij|.
fp32 storage holds floats that convert to fp64 exactly: the same bar on what the device holds.

Residual.  x_ij - sum_a q_ia g_aj as one chain of k1 fmas from x_ij: k1 roundings, one spare,
    |delta r_ij| <= gamma(k1 + 1) (|x_ij| + sum_a |q_ia g_aj|) + sum_a |q_ia| bar(G_aj)   (+ 2^-24 |r_ij|: fp32 store).

Against the exact least-squares residual the host's Q adds two terms.  Cholesky-QR2 of an n x k matrix
(Yamamoto, Nakatsukasa, Yanagisawa, Fukaya 2015, Thm 3.3 and 3.4) leaves ||Q'Q - I|| <= EQ(n, k) = 6 (n k + k (k
+ 1)) u and ||Q R - A||_F <= 5 k^2 u ||A||_2; the first enters as Q E G, the second moves the projector by at
most 2 kappa(A) times the relative residual:
    + EQ sum_a |q_ia| sum_b |g_bj| + 10 k1^2 u kappa ||d_j||_2,
kappa the condition number of the unit-norm design (the tests compute it: numpy's svd).

Coefficients.  Gamma solves the least-squares problem with the unit-norm design A (kappa as above); with
a backward error of eta = EQ(n, k1) Wedin's bound gives, on the unit-norm columns,
    ||delta Gamma~_j||_2 <= eta kappa (||Gamma~_j||_2 + kappa ||r_j||_2) =: bar, |delta Gamma_aj| <= bar / nrm_a.

Schur entry.  dst_ij = S_ij - sum_a F_ia F_ja as a chain of k fmas from S_ij,
    gamma(k + 1) (|S_ij| + sum_a |F_ia F_ja|) + KF(k) u kappa(C) ||f_i||_2 ||f_j||_2,   KF(k) = 3 k (k + 1) + 4:
F = S_dz D^-1 Lc^-T comes from the Cholesky factor of the unit-diagonal C = D^-1 S_zz D^-1 (L L' = C + dC, |dC| <=
gamma(k + 1) |L||L'|, norm <= k gamma(k + 1)) and two substitutions (k gamma(k) each), the division by D and a
spare; f_i'(C + dC)^-1 f_j moves by at most kappa(C) times that.
scale = 1 divides by d_i d_j, d = sqrt(diag): the bar over d_i d_j, plus |R_ij| (bar_ii / (2 S_ii) + bar_jj / (2
S_jj) + 4 u) for the two roots, their product and the division.
"""
import numpy as np

L = np.longdouble
U = 2.0 ** -53
TOL = 1e-7           # lm.fit's tol: PPLS_ADJ_TOL
KMAX = 16


def gamma(m):
    return m * U / (1.0 - m * U)


def kt_of(k1):
    return 4 if k1 <= 4 else 8 if k1 <= 8 else 16


def scale_plan(n, cols, f32, num_cus=256):
    """ppls_scale_plan restated: dict(units, ldc, tx, ty, grid_x, grid_y, nblocks)."""
    ve = 4 if f32 else 2
    units = max((cols + ve - 1) // ve, 1)
    tx = 1
    while tx < units and tx < 256:
        tx *= 2
    ty = 256 // tx
    grid_x = (units + tx - 1) // tx
    wgs = (num_cus if num_cus > 0 else 256) * 8
    gy = max(wgs // grid_x, 1)
    nb = min((n + 15) // 16, gy * ty, 2048)
    nb = max(nb, 1)
    return dict(units=units, ldc=units * ve, tx=tx, ty=ty, grid_x=grid_x, grid_y=(nb + ty - 1) // ty, nblocks=nb)


def blocks(n, nblocks):
    """The even split: block b owns rows [b n // nblocks, (b + 1) n // nblocks)."""
    return [(b * n // nblocks, (b + 1) * n // nblocks) for b in range(nblocks)]


def c_of(n, nblocks, ranks=1):
    return -(-n // nblocks) + nblocks + ranks + 2


# ------------------------------------------------------------------------------------ host models
def coef_model(Q, D, nblocks, skip_block=None):
    """Q'D in the kernel's order with plain fp64 (a product, then an add): rows in order inside a row
    block, the blocks' partials in block order."""
    G = np.zeros((Q.shape[1], D.shape[1]))
    for b, (r0, r1) in enumerate(blocks(D.shape[0], nblocks)):
        if b == skip_block:
            continue
        part = np.zeros_like(G)
        for i in range(r0, r1):
            part += Q[i][:, None] * D[i][None, :]
        G += part
    return G


def apply_model(Q, G, D, f32=False, acc32=False):
    """x - sum_a q_a g_a, a ascending from x, plain fp64 (acc32: the defect of an fp32 accumulator)."""
    t = np.float32 if acc32 else np.float64
    R = D.astype(t)
    for a in range(Q.shape[1]):
        R = (R - Q[:, a].astype(t)[:, None] * G[a].astype(t)[None, :]).astype(t)
    R = R.astype(np.float64)
    return R.astype(np.float32).astype(np.float64) if f32 else R


def gram_rows(A):
    G = np.zeros((A.shape[1], A.shape[1]))
    for i in range(A.shape[0]):
        G += A[i][:, None] * A[i][None, :]
    return G


def chol_pivot(G, tol):
    """ppls_adj_chol: (L, 0) or (None, 1-based refused column): a pivot L_jj that is not > tol."""
    k = G.shape[0]
    Lo = np.zeros((k, k))
    for j in range(k):
        d = G[j, j] - np.dot(Lo[j, :j], Lo[j, :j])
        if not (d > tol * tol) or not np.isfinite(d):
            return None, j + 1
        Lo[j, j] = np.sqrt(d)
        for i in range(j + 1, k):
            Lo[i, j] = (G[i, j] - np.dot(Lo[i, :j], Lo[j, :j])) / Lo[j, j]
    return Lo, 0


def solve_rows(A, Lo):
    """A L^-T row by row (forward substitution)."""
    A = A.copy()
    for j in range(Lo.shape[0]):
        A[:, j] = (A[:, j] - A[:, :j] @ Lo[j, :j]) / Lo[j, j]
    return A


def design_q(Z, intercept=True, shards=None):
    """The host side of ppls_adjust_data in numpy: centre, unit-scale, Cholesky-QR2 with the pivot rule.
    Returns dict(Q (n x k1), zc, nrm, L1, L2) or dict(refused=column).  shards: row ranges whose sums
    are formed apart and added (the ranks)."""
    Z = np.asarray(Z, dtype=np.float64)
    n, k = Z.shape
    parts = shards or [(0, n)]

    def rsum(f):
        tot = None
        for r0, r1 in parts:
            v = f(r0, r1)
            tot = v if tot is None else tot + v
        return tot
    zc = rsum(lambda a, b: Z[a:b].sum(axis=0) if b > a else np.zeros(k)) / n if intercept else np.zeros(k)
    # T = [1 / sqrt(n) | Z - zc]: the constant column goes through both rounds with the others
    T = np.hstack([np.full((n, 1), 1.0 / np.sqrt(n)), Z - zc]) if intercept else Z - zc
    i0 = int(intercept)
    C = rsum(lambda a, b: gram_rows(T[a:b]))
    nrm = np.sqrt(np.diag(C))
    nrm[:i0] = 1.0
    raw = np.sqrt(np.diag(C)[i0:] + n * zc * zc)
    bad = np.nonzero(~(nrm[i0:] > TOL * raw))[0]
    if bad.size:
        return dict(refused=int(bad[0]) + 1)
    C = C / np.outer(nrm, nrm)
    np.fill_diagonal(C, 1.0)
    L1, piv = chol_pivot(C, TOL)
    if piv:
        return dict(refused=piv - i0)
    T = solve_rows(T / nrm, L1)
    L2, piv = chol_pivot(rsum(lambda a, b: gram_rows(T[a:b])), 0.0)
    if piv:
        return dict(refused=piv - i0)
    return dict(Q=solve_rows(T, L2), zc=zc, nrm=nrm, L1=L1, L2=L2)


def gamma_from(G, q, intercept=True):
    """The record from the coefficients G: H = L1^-T L2^-T G, Gamma = diag(1 / nrm) H's covariate rows and
    the centre H_0 / sqrt(n)."""
    i0 = int(intercept)
    H = np.linalg.solve(q["L1"].T, np.linalg.solve(q["L2"].T, G))
    n = q["Q"].shape[0]
    return H[i0:] / q["nrm"][i0:, None], (H[0] / np.sqrt(n) if intercept else np.zeros(G.shape[1]))


def schur_f(S, z0, k, live):
    """schur_plan in numpy: F' (k x P over the live columns of S[:P, :P]), kappa(C), D, Lc; or None, column."""
    P = live.shape[0]
    Szz = np.tril(S[z0:z0 + k, z0:z0 + k])
    Szz = Szz + np.tril(Szz, -1).T
    d = np.sqrt(np.diag(Szz))
    if not np.all(d > 0):
        return None, int(np.nonzero(~(d > 0))[0][0]) + 1
    C = Szz / np.outer(d, d)
    np.fill_diagonal(C, 1.0)
    Lc, piv = chol_pivot(C, TOL)
    if piv:
        return None, piv
    Ft = np.where(live[None, :], S[z0:z0 + k, :P] / d[:, None], 0.0)
    Ft = np.linalg.solve(Lc, Ft) if k > 1 else Ft / Lc[0, 0]
    return dict(Ft=Ft, kappa=float(np.linalg.cond(C)), d=d, Lc=Lc), 0


def schur_model(S, Ft, live, mirror_upper=False):
    """dst = S[:P, :P] - F F' by the kernel's chain (plain fp64), the lower triangle mirrored (mirror_upper:
    the defect of mirroring the upper one), padding 0."""
    P = live.shape[0]
    R = S[:P, :P].copy()
    for a in range(Ft.shape[0]):
        R = R - np.outer(Ft[a], Ft[a])
    R = np.where(np.outer(live, live), R, 0.0)
    T = np.triu(R) if mirror_upper else np.tril(R)
    return T + (np.triu(R, 1).T if mirror_upper else np.tril(R, -1).T)


def joint_live(p, ldx, q, ldy):
    c = np.arange(ldx + ldy)
    return (c < p) | ((c >= ldx) & (c < ldx + q))


# ------------------------------------------------------------------------------------ long-double references
def ld_qr(A):
    """Q (long double, n x k) of A by Gram-Schmidt with two passes per column."""
    A = np.asarray(A, dtype=L)
    Q = np.zeros_like(A)
    for j in range(A.shape[1]):
        v = A[:, j].copy()
        for _ in range(2):
            for m in range(j):
                v = v - Q[:, m] * np.sum(Q[:, m] * v, dtype=L)
        Q[:, j] = v / np.sqrt(np.sum(v * v, dtype=L))
    return Q


def ld_design(Z, intercept=True):
    Z = np.asarray(Z, dtype=L)
    return np.hstack([np.ones((Z.shape[0], 1), dtype=L), Z]) if intercept else Z


def ld_coef(Q, D):
    """Q'D in long double (Q, D as held: fp64)."""
    Q, D = np.asarray(Q, dtype=L), np.asarray(D, dtype=L)
    return np.array([[np.sum(Q[:, a] * D[:, j], dtype=L) for j in range(D.shape[1])] for a in range(Q.shape[1])], dtype=L)


def ld_resid(Z, D, intercept=True):
    """The least-squares residuals of D on [1 Z], and the orthonormal basis used, in long double."""
    Q = ld_qr(ld_design(Z, intercept))
    D = np.asarray(D, dtype=L)
    return D - Q @ ld_coef(Q, D), Q


def ld_gamma(Z, D, intercept=True):
    """lm's coefficients (without the intercept's row), long double: R^-1 Q'D of the centred design."""
    Z = np.asarray(Z, dtype=L)
    Zc = Z - Z.mean(axis=0, dtype=L) if intercept else Z
    Q = ld_qr(Zc)
    R = np.array([[np.sum(Q[:, a] * Zc[:, b], dtype=L) for b in range(Z.shape[1])] for a in range(Z.shape[1])], dtype=L)
    B = ld_coef(Q, D)
    for a in range(Z.shape[1] - 1, -1, -1):      # back substitution
        B[a] = (B[a] - R[a, a + 1:] @ B[a + 1:]) / R[a, a]
    return B


def ld_schur(S, z0, k, live):
    """S_dd - S_dz S_zz^-1 S_zd over the live columns, long double (Cholesky and substitutions)."""
    P = live.shape[0]
    S = np.asarray(S, dtype=L)
    Szz = np.tril(S[z0:z0 + k, z0:z0 + k])
    Szz = Szz + np.tril(Szz, -1).T
    Lo = np.zeros((k, k), dtype=L)
    for j in range(k):
        Lo[j, j] = np.sqrt(Szz[j, j] - np.sum(Lo[j, :j] ** 2, dtype=L))
        for i in range(j + 1, k):
            Lo[i, j] = (Szz[i, j] - np.sum(Lo[i, :j] * Lo[j, :j], dtype=L)) / Lo[j, j]
    F = np.where(live[None, :], S[z0:z0 + k, :P], L(0))
    for j in range(k):
        F[j] = (F[j] - Lo[j, :j] @ F[:j]) / Lo[j, j]
    T = np.tril(S[:P, :P])
    R = T + np.tril(T, -1).T - F.T @ F
    return np.where(np.outer(live, live), R, L(0))


# ------------------------------------------------------------------------------------ bars
def eq_of(n, k):
    return 6.0 * (n * k + k * (k + 1)) * U


def coef_bar(Q, D, nblocks, ranks=1):
    return gamma(c_of(D.shape[0], nblocks, ranks)) * (np.abs(Q).T @ np.abs(D))


def resid_bar(Q, G, D, gbar, f32=False, resid=None):
    """The bar of the apply pass given Q and the coefficients it used (gbar: their own bar)."""
    k1 = Q.shape[1]
    aQ = np.abs(Q)
    b = gamma(k1 + 1) * (np.abs(D) + aQ @ np.abs(G)) + aQ @ gbar
    if f32:
        b = b + 2.0 ** -24 * np.abs(resid)
    return b


def design_terms(Q, G, D, kappa):
    """What the host's Q adds against the exact least-squares residual."""
    n, k1 = Q.shape
    return (eq_of(n, k1) * np.outer(np.abs(Q).sum(axis=1), np.abs(G).sum(axis=0))
            + 10.0 * k1 * k1 * U * kappa * np.sqrt((D * D).sum(axis=0))[None, :])


def design_kappa(Z, intercept=True):
    """kappa of the unit-norm design [1/sqrt(n) | centred unit columns] (or the unit columns of Z)."""
    Z = np.asarray(Z, dtype=np.float64)
    A = Z - Z.mean(axis=0) if intercept else Z
    A = A / np.sqrt((A * A).sum(axis=0))
    return float(np.linalg.cond(A))


def gamma_bar(Z, D, intercept=True):
    """|delta Gamma_aj| <= eta kappa (||Gamma~_j|| + kappa ||r_j||) / nrm_a."""
    Z = np.asarray(Z, dtype=np.float64)
    n, k = Z.shape
    A = Z - Z.mean(axis=0) if intercept else Z
    nrm = np.sqrt((A * A).sum(axis=0))
    kap = design_kappa(Z, intercept)
    Dc = D - D.mean(axis=0) if intercept else D
    gt, *_ = np.linalg.lstsq(A / nrm, Dc, rcond=None)
    r = Dc - (A / nrm) @ gt
    bar = eq_of(n, k + int(intercept)) * kap * (np.sqrt((gt * gt).sum(axis=0)) + kap * np.sqrt((r * r).sum(axis=0)))
    return bar[None, :] / nrm[:, None]


def kf_of(k):
    return 3.0 * k * (k + 1) + 4.0


def schur_bar(S, f, live):
    P = live.shape[0]
    Ft, k = f["Ft"], f["Ft"].shape[0]
    nf = np.sqrt((Ft * Ft).sum(axis=0))
    b = gamma(k + 1) * (np.abs(S[:P, :P]) + np.abs(Ft).T @ np.abs(Ft)) + kf_of(k) * U * f["kappa"] * np.outer(nf, nf)
    return np.where(np.outer(live, live), b, 0.0)


def schur_scaled(R, bar, live):
    """(R_ij / (d_i d_j), its bar) with d = sqrt(diag R) over the live columns."""
    dg = np.where(live, np.diag(R).astype(np.float64), 1.0)
    d = np.sqrt(dg)
    Rs = np.asarray(R / np.outer(d, d).astype(R.dtype))
    rel = np.where(live, np.diag(bar) / (2.0 * dg), 0.0)
    return Rs, bar / np.outer(d, d) + np.abs(Rs.astype(np.float64)) * (rel[:, None] + rel[None, :] + 4.0 * U)


def inside(got, ref, bar):
    """max over the entries of |got - ref| / bar (0 / 0 = 0): inside the bar when <= 1."""
    err = np.abs(np.asarray(got, dtype=L) - np.asarray(ref, dtype=L)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bar)
    return float(np.max(ratio)) if ratio.size else 0.0
