"""Long-double reference and a-priori error bar for the statistics pass of one meta_PPLSi EM step
from per-population cross-products (ppls_xprod_meta.hip), and the same step in plain numpy.

Shared by tests/test_gpu_meta_xprod.py (the HIP kernels against the bar, the fits against the
oracle) and tests/test_meta_xprod_host.py (the bar itself and the algebra, no GPU).

With S_j = [X_j Y_j]'[X_j Y_j] in blocks S_xx, S_xy, S_yx, S_yy, the shared loadings w, c and the
population's mu coefficients alpha_j .. delta_j:
    M_j = S_j blockdiag(w, c):   m0x = S_xx w, m1x = S_xy c, m0y = S_yx w, m1y = S_yy c
    SX_j = alpha_j m0x + beta_j m1x            (= X_j' mu_T)
    SY_j = gamma_j m0y + delta_j m1y           (= Y_j' mu_U)
    G_j  = [[w'm0x, w'm1x], [w'm1x, c'm1y]]    (= Gram([X_j w, Y_j c]))
The reference evaluates them in np.longdouble from the fp64 S_j, w, c and coefficients, which are
exact inputs here: the S_j are the matrices the device holds (downloaded), the coefficients the
ones the library staged (ppls_rank1_mu_coefficients), so neither the Gram's rounding nor the
evaluation of the coefficient formulas is charged to the kernel.

The bar is entrywise and holds for any summation order and for FMA (Higham, Accuracy and Stability
of Numerical Algorithms, 3.1 and 3.5).  u = 2^-53, gamma_k = k u / (1 - k u), m = max(ldx, ldy) + 4
(a dot product over a padded row of S_j, the two coefficient products, their sum, one to spare):
    |SX_j - ref| <= gamma_m (|alpha_j| |S_xx||w| + |beta_j| |S_xy||c|)
    |SY_j - ref| <= gamma_m (|gamma_j| |S_yx||w| + |delta_j| |S_yy||c|)
    e0x = gamma_m |S_xx||w|, e1x = gamma_m |S_xy||c|, e1y = gamma_m |S_yy||c|   (the entries of M_j)
    |G_00 - ref| <= gamma_ldx |w|'|m0x| + (1 + gamma_ldx) |w|'e0x
    |G_01 - ref| <= gamma_ldx |w|'|m1x| + (1 + gamma_ldx) |w|'e1x
    |G_11 - ref| <= gamma_ldy |c|'|m1y| + (1 + gamma_ldy) |c|'e1y
each times 1 + 2^-10 for the reference's own rounding.  Nothing in it is measured.
"""
import math

import numpy as np

from sweep_bar import LD, SLACK, gamma, padded_width


def pop_params(K):
    """K x 5 (B_T, sigX, sigY, sigH, sigT), distinct per population and well conditioned as
    sweep_bar.sweep_problem's theta is (sigX, sigY > sigT)."""
    j = np.arange(K, dtype=np.float64)
    return np.column_stack([1.2 - 0.1 * j, 2.0 + 0.1 * j, 1.7 + 0.05 * j, 0.9 - 0.05 * j, 1.1 - 0.1 * j])


def blocks(S, p):
    return S[:p, :p], S[:p, p:], S[p:, :p], S[p:, p:]


def stats_fp64(S_list, p, w, c, coef, drop=None, swap=False, pop0=False):
    """The statistics in plain fp64 numpy: (SX K x p, SY K x q, G K x 2 x 2).  Seeded defects for
    the bar's own test: drop = a joint column every S_j loses, swap = alpha_j and beta_j exchanged,
    pop0 = every population uses population 0's coefficients."""
    w, c = np.ravel(w).astype(np.float64), np.ravel(c).astype(np.float64)
    SX, SY, G = [], [], []
    for j, S in enumerate(S_list):
        S = np.array(S, dtype=np.float64)
        if drop is not None:
            S[:, drop] = 0.0
        al, be, ga, de = coef[0 if pop0 else j]
        if swap:
            al, be = be, al
        xx, xy, yx, yy = blocks(S, p)
        m0x, m1x, m0y, m1y = xx @ w, xy @ c, yx @ w, yy @ c
        SX.append(al * m0x + be * m1x)
        SY.append(ga * m0y + de * m1y)
        g01 = w @ m1x
        G.append(np.array([[w @ m0x, g01], [g01, c @ m1y]]))
    return np.array(SX), np.array(SY), np.array(G)


class MetaReference:
    """The K statistics blocks in long double and their entrywise bars."""

    def __init__(self, S_list, p, q, w, c, coef):
        ldx, ldy = padded_width(p), padded_width(q)
        gm, gx, gy = gamma(max(ldx, ldy) + 4), gamma(ldx), gamma(ldy)
        wl, cl = np.ravel(w).astype(LD), np.ravel(c).astype(LD)
        aw, ac = np.abs(wl), np.abs(cl)
        self.SX, self.SY, self.G, self.bar_SX, self.bar_SY, self.bar_G = [], [], [], [], [], []
        for j, S in enumerate(S_list):
            Sl = np.asarray(S).astype(LD)
            xx, xy, yx, yy = blocks(Sl, p)
            al, be, ga, de = (LD(v) for v in coef[j])
            m0x, m1x, m0y, m1y = xx @ wl, xy @ cl, yx @ wl, yy @ cl
            a0x, a1x, a0y, a1y = np.abs(xx) @ aw, np.abs(xy) @ ac, np.abs(yx) @ aw, np.abs(yy) @ ac
            self.SX.append(al * m0x + be * m1x)
            self.SY.append(ga * m0y + de * m1y)
            self.bar_SX.append(gm * (abs(al) * a0x + abs(be) * a1x) * SLACK)
            self.bar_SY.append(gm * (abs(ga) * a0y + abs(de) * a1y) * SLACK)
            g00, g01, g11 = wl @ m0x, wl @ m1x, cl @ m1y
            b00 = gx * (aw @ np.abs(m0x)) + (1 + gx) * (aw @ (gm * a0x))
            b01 = gx * (aw @ np.abs(m1x)) + (1 + gx) * (aw @ (gm * a1x))
            b11 = gy * (ac @ np.abs(m1y)) + (1 + gy) * (ac @ (gm * a1y))
            self.G.append(np.array([[g00, g01], [g01, g11]], dtype=LD))
            self.bar_G.append(np.array([[b00, b01], [b01, b11]], dtype=LD) * SLACK)
        for k in ("SX", "SY", "G", "bar_SX", "bar_SY", "bar_G"):
            setattr(self, k, np.array(getattr(self, k), dtype=LD))

    @staticmethod
    def _ratio(got, ref, bar):
        """max err / bar; an entry whose bar is 0 must be exact."""
        err = np.abs(np.asarray(got).astype(LD) - ref)
        if err.shape != ref.shape or not np.all(np.isfinite(err)):
            return float("inf")
        zero = bar == 0
        if np.any(err[zero] != 0):
            return float("inf")
        return float(np.max(err[~zero] / bar[~zero])) if np.any(~zero) else 0.0

    def ratios(self, SX, SY, G):
        """Worst err / bar per quantity over all populations; <= 1 is inside the bar."""
        return dict(SX=self._ratio(SX, self.SX, self.bar_SX), SY=self._ratio(SY, self.SY, self.bar_SY),
                    G=self._ratio(G, self.G, self.bar_G))


def mu_coefficients_fp64(params):
    """K x 4 (alpha, beta, gamma, delta) from params (K x 5) by EMstepC_fast's formulas
    (src/loglC.cpp:354-361; oracle.ppls_oracle.emstepc_fast / emstep_w), in fp64."""
    out = []
    for B, sX, sY, sH, sT in np.asarray(params, dtype=np.float64):
        c1, c2, c3 = _c123(B, sX, sY, sH, sT)
        s2X, s2Y, s2T, v = sX * sX, sY * sY, sT * sT, sT * sT * B * B + sH * sH
        out.append([s2T * (-c1 + -c2 * B + 1 / s2X), s2T * (-c2 + -c3 * B + 1 / s2Y * B),
                    -s2T * B * c1 + -c2 * v + 1 / s2X * B * s2T, -c2 * B * s2T + -c3 * v + 1 / s2Y * v])
    return np.array(out)


def _c123(B, sX, sY, sH, sT):
    """meta_EMstep's c1, Kwc, c3 (EM_W_multi.R:466-474)."""
    g = sT ** 2 * B ** 2 + sH ** 2
    Kw = sT ** 2 - sT ** 4 * B ** 2 / sY ** 2 + sT ** 4 * B ** 2 * g / (sY ** 2 * (g + sY ** 2))
    Kc = g - sT ** 4 * B ** 2 / sX ** 2 + sT ** 6 * B ** 2 / (sX ** 2 * (sT ** 2 + sX ** 2))
    Kwc = (sT ** 2 * B / (sX ** 2 * sY ** 2) - Kc * sT ** 2 * B / (sX ** 2 * sY ** 2 * (Kc + sY ** 2))
           - sT ** 4 * B / (sX ** 2 * sY ** 2 * (sT ** 2 + sX ** 2))
           + Kc * sT ** 4 * B / (sX ** 2 * sY ** 2 * (Kc + sY ** 2) * (sT ** 2 + sX ** 2)))
    return Kw / (sX ** 2 * (Kw + sX ** 2)), Kwc, Kc / (sY ** 2 * (Kc + sY ** 2))


def emstep_from_xprod(S_list, N_list, p, q, W, C, params):
    """meta_EMstep (EM_W_multi.R:446-485) from the populations' cross-products alone: the statistics
    above, ssq(X_j), ssq(Y_j) = the traces of S_j's diagonal blocks, N_j the row counts; then
    EMstepC_fast's moments (src/loglC.cpp:353-375) with every mu'mu written as a quadratic form in
    G_j.  Returns what oracle.ppls_oracle.meta_emstep returns."""
    W, C = np.ravel(W), np.ravel(C)
    P = np.array([[float(np.ravel(pp[k])[0]) for k in ("B_T", "sigX", "sigY", "sigH", "sigT")] for pp in params])
    SX, SY, G = stats_fp64(S_list, p, W, C, mu_coefficients_fp64(P))
    ret = []
    for j, S in enumerate(S_list):
        B, sX, sY, sH, sT = P[j]
        N = float(N_list[j])
        c1, c2, c3 = _c123(B, sX, sY, sH, sT)
        s2X, s2Y, s2H, s2T = sX * sX, sY * sY, sH * sH, sT * sT
        v = s2T * B * B + s2H
        al, be, ga, de = mu_coefficients_fp64(P[j:j + 1])[0]
        xw2, xy, yc2 = G[j][0, 0], G[j][0, 1], G[j][1, 1]
        ssqX, ssqY = float(np.trace(S[:p, :p])), float(np.trace(S[p:, p:]))
        tt = al * al * xw2 + 2 * al * be * xy + be * be * yc2                      # mu_T'mu_T
        ut = ga * al * xw2 + (ga * be + de * al) * xy + de * be * yc2              # mu_U'mu_T
        Ctt = s2T - s2T * s2T * (-c1 - 2 * B * c2 - B * B * (c3 - 1 / s2Y) + 1 / s2X) + tt / N
        Cut = s2T * B - (-s2T * s2T * B * (c1 - 1 / s2X) - s2T * s2T * B * B * c2 - s2T * v * c2
                         - v * s2T * B * (c3 - 1 / s2Y)) + ut / N
        Cee = s2X - (-s2X * s2X * c1 + p * s2X) / p + (
            c1 * c1 * s2X * s2X * xw2 + ssqX + c2 * c2 * s2X * s2X * yc2 - 2 * c1 * s2X * xw2
            + 2 * c1 * c2 * s2X * s2X * xy - 2 * c2 * s2X * xy) / N / p
        Cff = s2Y - (-s2Y * s2Y * c3 + q * s2Y) / q + (
            c3 * c3 * s2Y * s2Y * yc2 + ssqY + c2 * c2 * s2Y * s2Y * xw2 - 2 * c3 * s2Y * yc2
            + 2 * c3 * c2 * s2Y * s2Y * xy - 2 * c2 * s2Y * xy) / N / q
        h1, h2 = -c2 * s2H, -(c3 - 1 / s2Y) * s2H                                  # mh = h1 Xw + h2 Yc
        Chh = s2H - (-s2H * s2H * (c3 - 1 / s2Y)) + (h1 * h1 * xw2 + 2 * h1 * h2 * xy + h2 * h2 * yc2) / N
        ret.append(dict(B=Cut / Ctt, sighat=np.array([math.sqrt(Cee), math.sqrt(Cff)]),
                        siglathat=np.array([math.sqrt(Chh), math.sqrt(Ctt)]), Cxt=SX[j] / N, Cyu=SY[j] / N))
    sg = [float(np.sign(ret[0]["Cxt"] @ e["Cxt"])) for e in ret]
    Wn = sum(s * e["Cxt"] for s, e in zip(sg, ret))
    Cn = sum(s * e["Cyu"] for s, e in zip(sg, ret))
    return dict(pops=ret, W=Wn / np.linalg.norm(Wn), C=Cn / np.linalg.norm(Cn))
