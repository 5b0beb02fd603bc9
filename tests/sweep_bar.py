"""Long-double reference and a-priori error bar for one statistics step of a sweep kernel.

Shared by tests/test_gpu_sweep_matrix.py (the HIP kernels against the bar) and
tests/test_sweep_bar_host.py (the bar itself: plain fp64 lies inside it, seeded defects outside).

Statistics of one sweep at theta = (W, C, B, sigE, sigF, sigH, sigT):
    a = X W, b = Y C, mu_T = alpha a + beta b, mu_U = gamma a + delta b   (EM_W_multi.R:691-694)
    SX = X' mu_T, SY = Y' mu_U, G = [a b]' [a b]
with alpha..delta from oracle.ppls_oracle.mu_coefficients.  The reference evaluates them in
np.longdouble from the fp64 inputs.

The bar is entrywise and holds for any summation order and for FMA (Higham, Accuracy and Stability
of Numerical Algorithms, 3.1 and 3.5): with u = 2^-53, gamma_k = k u / (1 - k u), n rows and
m = max(ldx, ldy) + 4 (a dot product over a padded row, the two coefficient products, their sum,
one to spare):
    E_T = gamma_m (|alpha| |X||W| + |beta| |Y||C|)                       |mu_T - ref| <= E_T
    |SX - ref| <= gamma_n |X|'|mu_T| + (1 + gamma_n) |X|' E_T            (SY, E_U alike)
    e = gamma_m [|X||W|  |Y||C|], z = [a b]
    |G - ref| <= gamma_n |z|'|z| + |z|'e + e'|z| + e'e
each times 1 + 2^-10 for the reference's own rounding.  Nothing in it is measured.
"""
import numpy as np

from oracle import ppls_oracle as o

LD = np.longdouble
U = LD(2.0) ** -53
SLACK = LD(1.0) + LD(2.0) ** -10

# p, q of the smallest shapes that select each body of the split sweep (fp64 storage)
SHAPES = {
    "A": (9, 12),        # NSH 1, guarded
    "B": (500, 390),     # NSH 1, full
    "C": (600, 7),       # NSH 2, guarded
    "D": (1000, 900),    # NSH 2, full, nch = 16 (the CPW 2 limit)
    "E": (1100, 40),     # NSH 4, CPW 2, guarded, five DMA waves
    "E'": (40, 1100),    # the same with Y the wide side
    "F": (2000, 300),    # NSH 4, CPW 4, guarded, nch = 19 (odd: clamped duplicate chunk)
    "G": (2000, 2000),   # NSH 4, CPW 4, full (the C3 width)
}
RMAX_OF = {"A": 8, "B": 8, "C": 8, "D": 8, "E": 5, "E'": 5, "F": 5, "G": 5}
# (rows, grid): the per-workgroup row counts at which the ring's prologue and tail branches change
# (SLOTS = 4, RP <= 2), 5 and 6 rows per workgroup, and empty workgroups
ROWS = [(n, 1) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13)] + [(37, 7), (3, 7)]


# the panel sweep (fp64 and fp32 storage): p, q and the component counts run at each
PANEL_SHAPES = {"narrow": (70, 37), "wide": (2100, 9)}
PANEL_R = {"narrow": tuple(range(1, 17)), "wide": (1, 10, 16)}
PANEL_ROWS = (1, 31, 32, 33, 63, 65, 129)   # around the 32- and 64-row dots tiles and the 128-row acc batch


def panel_pq(shape, r):
    """p, q of a panel shape at r components: q = r where ncol(Y) >= r asks for it (wide, r = 10, 16)."""
    p, q = PANEL_SHAPES[shape]
    return p, max(q, r)


def shape_pq(shape, r):
    """p, q of a shape at r components.  A fit needs ncol(Y) >= r (EM_W_multi.R:245, which the
    library's theta check enforces), so shape C takes q = 8 at r = 8: the same padded width
    ldy = 8, hence the same kernel body and LDS layout, with the padding column holding data."""
    p, q = SHAPES[shape]
    return p, max(q, r)


def padded_width(p, f32=False):
    """The leading dimension the library gives a p-column matrix (ld_of in ppls_capi.cpp)."""
    es = 4 if f32 else 8
    nbytes = p * es
    if nbytes < 1024 or (not f32 and p <= 2048):
        return (p + 3) & ~3 if f32 else (p + 1) & ~1
    al = 4096 if nbytes >= 16384 else 128
    return (nbytes + al - 1) // al * al // es


def gamma(k):
    k = LD(k)
    return k * U / (LD(1.0) - k * U)


def _polar(M):
    Uu, _, Vt = np.linalg.svd(M, full_matrices=False)
    return Uu @ Vt


def sweep_problem(n, p, q, r, seed):
    """make_problem-style Gaussian data with column scales spread over 10^+-2 (one wrong column pair
    shows entrywise) and a theta with unequal B and sigT (alpha..delta differ per component).

    The bar takes alpha..delta as exact inputs, but the library and the oracle each evaluate them in
    fp64 from theta, in their own operation order: alpha = t^2 / sigE^2 - c1 t^2 - c2 t^2 b (and its
    kin) cancels, so the two evaluations differ by a few u times the cancellation.  That difference
    is no property of a sweep kernel, yet it is charged to the bar, and at the narrowest shape
    (m = 16) the bar has no room for it.  So the theta here has noise variances above the latent
    ones (sigE, sigF > sigT), where the subtracted terms are small against t^2 / sigE^2 and the
    formulas are well conditioned: the two evaluations then agree to about 4 u (against 14 to 28 u
    at sigE = 0.9, sigF = 0.8, sigH = 0.3), which the bar absorbs."""
    rng = np.random.default_rng(seed)
    W0 = _polar(rng.standard_normal((p, r)))
    C0 = _polar(rng.standard_normal((q, r)))
    t = np.exp(-0.1 * np.arange(r))
    b = np.exp(np.log(1.5) - 0.3 * np.arange(r))
    T = rng.standard_normal((n, r)) * t
    Uu = T * b + 0.1 * rng.standard_normal((n, r))
    X = (T @ W0.T + 0.5 * rng.standard_normal((n, p))) * 10.0 ** rng.uniform(-2, 2, p)
    Y = (Uu @ C0.T + 0.6 * rng.standard_normal((n, q))) * 10.0 ** rng.uniform(-2, 2, q)
    th = dict(W=_polar(W0 + 0.5 * rng.standard_normal((p, r))), C=_polar(C0 + 0.5 * rng.standard_normal((q, r))),
              B=np.diag(np.linspace(1.2, 0.7, r)), sigE=2.0, sigF=1.7, sigH=0.9,
              sigT=np.diag(np.linspace(1.1, 0.6, r)))
    return X, Y, th


def coefficients(th):
    cf = o.mu_coefficients(th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])
    return tuple(np.asarray(cf[k], dtype=np.float64) for k in ("alpha", "beta", "gamma", "delta"))


class Reference:
    """The statistics of one sweep in long double and their entrywise bars."""

    def __init__(self, X, Y, th, ldx, ldy):
        n = X.shape[0]
        Xl, Yl = X.astype(LD), Y.astype(LD)
        Wl, Cl = np.asarray(th["W"]).astype(LD), np.asarray(th["C"]).astype(LD)
        al, be, ga, de = (c.astype(LD) for c in coefficients(th))
        a, b = Xl @ Wl, Yl @ Cl
        self.mu_T, self.mu_U = a * al + b * be, a * ga + b * de
        self.SX, self.SY = Xl.T @ self.mu_T, Yl.T @ self.mu_U
        z = np.hstack([a, b])
        self.G = z.T @ z
        aX, aY = np.abs(Xl), np.abs(Yl)
        gm, gn = gamma(max(ldx, ldy) + 4), gamma(n)
        aa, ab = aX @ np.abs(Wl), aY @ np.abs(Cl)
        E_T = gm * (np.abs(al) * aa + np.abs(be) * ab)
        E_U = gm * (np.abs(ga) * aa + np.abs(de) * ab)
        self.bar_T, self.bar_U = E_T * SLACK, E_U * SLACK
        self.bar_SX = (gn * (aX.T @ np.abs(self.mu_T)) + (1 + gn) * (aX.T @ E_T)) * SLACK
        self.bar_SY = (gn * (aY.T @ np.abs(self.mu_U)) + (1 + gn) * (aY.T @ E_U)) * SLACK
        az, e = np.abs(z), gm * np.hstack([aa, ab])
        self.bar_G = (gn * (az.T @ az) + az.T @ e + e.T @ az + e.T @ e) * SLACK

    @staticmethod
    def _ratio(got, ref, bar):
        """max err / bar; an entry whose bar is 0 (an all-zero column) must be exact."""
        err = np.abs(np.asarray(got).astype(LD) - ref)
        if not np.all(np.isfinite(err)):
            return float("inf")
        if err.size == 0:
            return 0.0
        zero = bar == 0
        if np.any(err[zero] != 0):
            return float("inf")
        return float(np.max(err[~zero] / bar[~zero])) if np.any(~zero) else 0.0

    def ratios(self, SX, SY, G, mu=None):
        """Worst err / bar per quantity, {"SX", "SY", "G"[, "mu_T", "mu_U"]}; <= 1 is inside the bar."""
        out = dict(SX=self._ratio(SX, self.SX, self.bar_SX), SY=self._ratio(SY, self.SY, self.bar_SY),
                   G=self._ratio(G, self.G, self.bar_G))
        if mu is not None:
            r = self.mu_T.shape[1]
            out["mu_T"] = self._ratio(mu[:, :r], self.mu_T, self.bar_T)
            out["mu_U"] = self._ratio(mu[:, r:], self.mu_U, self.bar_U)
        return out
