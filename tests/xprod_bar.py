"""Long-double reference and a-priori error bars for the cross-product statistics pass alone
(ppls_xprod_tile_kernel and ppls_xprod_gram_kernel, ppls_xprod.hip; ``Context.xprod_pass``).

Shared by tests/test_xprod_bar_host.py (the bars themselves: plain fp64 numpy inside, seeded defects
outside; no GPU) and tests/test_gpu_xprod_matrix.py (every (R, RW) instantiation against them).

The pass, for S (P x P, P = ldx + ldy, the X block ldx wide), B = blockdiag(W, C) with R columns a side
and the coefficient vectors alpha, beta, gamma, delta:
    M  = S B                       P x 2R:  Mw = M[:, :R] = S[:, X] W,  Mc = M[:, R:] = S[:, Y] C
    SX[i, t] = alpha_t Mw[i, t] + beta_t  Mc[i, t]      rows i <  ldx  (X'mu_T)
    SY[i, t] = gamma_t Mw[i, t] + delta_t Mc[i, t]      rows i >= ldx  (Y'mu_U)
    G  = B'M                       2R x 2R, one triangle computed, mirrored
The reference evaluates all of it in np.longdouble from the fp64 S, W, C and coefficients the kernel was
given: nothing upstream of the pass (the MFMA Gram that formed S, the library's own alpha..delta) is in it.

Bars.  u = 2^-53, gamma_n = n u / (1 - n u).  M and G are po2_bar.PassReference's M and Q: a dot product
of n terms errs by at most gamma_n |a|'|b| in any order, with or without FMA (Higham 3.1, 3.5), n = the
padded width + 2.  SX is two products and one sum (or one product and one FMA) of the computed M:
    bar_SX = (|alpha| bar_Mw + |beta| bar_Mc) (1 + gamma_2) + gamma_2 (|alpha| |Mw| + |beta| |Mc|)
and SY alike with gamma, delta; each times 1 + 2^-10 for the reference's own rounding.  Nothing is measured.

Prefix property.  Column t of M, SX, SY and row / column t of G depend on column t of W and C (and entry t
of the coefficients) only, so one 16-column problem per shape serves every R: the R-form gets the first R
columns and is held to the first R columns of the one reference (``XprodReference.ratios``).

An exact case (``exact_problem``): S symmetric with integers in [-8, 8], W and C integers in [-4, 4], the
coefficients signed powers of two in [2^-3, 2^3].  Every product and partial sum is an integer (or an
integer / 8) far below 2^53 -- sum |S||B| <= 32 ld, |G| <= 4 P 32 ld -- so fp64 is exact in any order, the
bars are 0 and every output must equal the int64 result.
"""
import numpy as np

from po2_bar import PassReference, ratio
from sweep_bar import LD, SLACK, gamma, padded_width

RMAX = 16
QUANTITIES = ("M", "SX", "SY", "G")


def legal_rw(r):
    """The rows-per-wave forms the launcher has at r components."""
    return (1, 2, 4, 8) if r <= 8 else (1, 2, 4)


FORMS = tuple((r, rw) for r in range(1, RMAX + 1) for rw in legal_rw(r))      # 16 x 3 + 8 = 56
DEFECTS = ("drop_pair", "y_offset", "row_past_P", "swap_ab", "gram_wrong_side", "scatter_off_by_one")


def tile_rows(P, r, rw_opt, num_cus):
    """ppls_xprod_tile_rows restated."""
    if rw_opt in (1, 2, 4) or (rw_opt == 8 and r <= 8):
        return rw_opt
    return 2 if P // 8 >= 2 * num_cus else 1


def tile_nt(P):
    """ppls_xprod_tile_nt restated: 8 P^2 bytes against 200 MiB."""
    return int(8 * P * P > 200 * (1 << 20))


# ------------------------------------------------------------------------------------------- data
def coefficients(rng, r=RMAX):
    """alpha..delta (4 x r) with per-column distinct magnitudes (10^+-1) and signs."""
    return rng.choice([-1.0, 1.0], (4, r)) * 10.0 ** rng.uniform(-1, 1, (4, r))


def data(p, q, rows, seed):
    """(D, W, C, coef): `rows` Gaussian rows of p + q columns with column scales spread over 10^+-2 (as
    sweep_bar.sweep_problem: one wrong column pair shows entrywise); W (p x 16), C (q x 16) Gaussian;
    coefficients as above."""
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((rows, p + q)) * 10.0 ** rng.uniform(-2, 2, p + q)
    return D, rng.standard_normal((p, RMAX)), rng.standard_normal((q, RMAX)), coefficients(rng)


def problem(p, q, rows, seed):
    """(S, W, C, coef) without padding: S = D'D of ``data``, mirrored to be bitwise symmetric."""
    D, W, C, coef = data(p, q, rows, seed)
    S = D.T @ D
    return np.triu(S) + np.triu(S, 1).T, W, C, coef


def exact_problem(p, q, seed):
    """The exact case of the module docstring."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-8, 9, (p + q, p + q))
    S = (np.triu(A) + np.triu(A, 1).T).astype(np.float64)
    W = rng.integers(-4, 5, (p, RMAX)).astype(np.float64)
    C = rng.integers(-4, 5, (q, RMAX)).astype(np.float64)
    coef = rng.choice([-1.0, 1.0], (4, RMAX)) * 2.0 ** rng.integers(-3, 4, (4, RMAX))
    return S, W, C, coef


def layout(p, q, ldx=None, ldy=None):
    """(ldx, ldy, live): the padded widths (the library's for p and q columns unless given: the pass takes
    any even widths >= 2) and the indices of the real columns in the padded layout."""
    ldx, ldy = ldx or padded_width(p), ldy or padded_width(q)
    assert ldx >= p and ldy >= q and ldx % 2 == 0 and ldy % 2 == 0
    return ldx, ldy, np.r_[np.arange(p), ldx + np.arange(q)]


def padded(S, W, C, p, q, fill=0.0, ldx=None, ldy=None):
    """S, W, C in the padded layout (zeros in S's padding rows and columns; `fill` in the padding rows of
    W and C, which meet only zeros of S and of M)."""
    ldx, ldy, live = layout(p, q, ldx, ldy)
    Sp = np.zeros((ldx + ldy, ldx + ldy))
    Sp[np.ix_(live, live)] = S
    Wp, Cp = np.full((ldx, W.shape[1]), fill), np.full((ldy, C.shape[1]), fill)
    Wp[:p], Cp[:q] = W, C
    return Sp, Wp, Cp


# -------------------------------------------------------------------------------------- reference
class XprodReference:
    """M, SX, SY, G of the 16-column problem in long double with their entrywise bars; ``ratios`` holds an
    R-form's padded outputs to the first R columns."""

    def __init__(self, S, p, q, W, C, coef, ldx=None, ldy=None):
        self.p, self.q = p, q
        self.ldx, self.ldy, self.live = layout(p, q, ldx, ldy)
        assert self.ldx <= padded_width(p) and self.ldy <= padded_width(q)     # PassReference's term count covers the sums
        R = self.R = W.shape[1]
        pr = PassReference(S, p, q, W, C)
        self.M, self.bar_M, self.G, self.bar_G = pr.M, pr.bar_M, pr.Q, pr.bar_Q
        al, be, ga, de = (np.asarray(v, dtype=np.float64).astype(LD) for v in coef)
        Mw, Mc, bw, bc = pr.M[:, :R], pr.M[:, R:], pr.bar_M[:, :R], pr.bar_M[:, R:]
        g2 = gamma(2)

        def side(rows, a, b):
            val = a * Mw[rows] + b * Mc[rows]
            bar = ((np.abs(a) * bw[rows] + np.abs(b) * bc[rows]) * (1 + g2)
                   + g2 * (np.abs(a) * np.abs(Mw[rows]) + np.abs(b) * np.abs(Mc[rows]))) * SLACK
            return val, bar

        self.SX, self.bar_SX = side(slice(0, p), al, be)
        self.SY, self.bar_SY = side(slice(p, p + q), ga, de)

    def _cols(self, r):
        return np.r_[np.arange(r), self.R + np.arange(r)]

    @staticmethod
    def _padded(got, live_rows, ref, bar):
        """err / bar over the live rows; every other row must be exactly 0 (inf when not)."""
        got = np.asarray(got)
        pad = np.setdiff1d(np.arange(got.shape[0]), live_rows)
        if not np.all(got[pad] == 0.0):
            return float("inf")
        return ratio(got[live_rows], ref, bar)

    def ratios(self, M, SX, SY, G):
        """Worst err / bar per quantity for an r-form's outputs in the padded layout (M: P x 2r, SX:
        ldx x r, SY: ldy x r, G: 2r x 2r); <= 1 is inside; a non-zero padding row is inf."""
        r = np.asarray(G).shape[0] // 2
        c = self._cols(r)
        return dict(M=self._padded(M, self.live, self.M[:, c], self.bar_M[:, c]),
                    SX=self._padded(SX, np.arange(self.p), self.SX[:, :r], self.bar_SX[:, :r]),
                    SY=self._padded(SY, np.arange(self.q), self.SY[:, :r], self.bar_SY[:, :r]),
                    G=ratio(G, self.G[np.ix_(c, c)], self.bar_G[np.ix_(c, c)]))


def exact_reference(S, W, C, coef, p, q, ldx=None, ldy=None):
    """The int64 result of the exact case in the padded layout, as fp64 (M, SX, SY, G)."""
    Si, Wi, Ci = (np.asarray(A).astype(np.int64) for A in (S, W, C))
    assert np.array_equal(Si, S) and np.array_equal(Wi, W) and np.array_equal(Ci, C)
    ldx, ldy, live = layout(p, q, ldx, ldy)
    R = W.shape[1]
    Ml = np.hstack([Si[:, :p] @ Wi, Si[:, p:] @ Ci])
    Bl = np.zeros((p + q, 2 * R), dtype=np.int64)
    Bl[:p, :R], Bl[p:, R:] = Wi, Ci
    G = Bl.T @ Ml
    assert np.abs(G).max() < 2 ** 50
    M = np.zeros((ldx + ldy, 2 * R))
    M[live] = Ml
    c8 = np.asarray(coef) * 8
    assert np.array_equal(c8, np.rint(c8))
    c8 = c8.astype(np.int64)
    SX, SY = np.zeros((ldx, R)), np.zeros((ldy, R))
    SX[:p] = (c8[0] * Ml[:p, :R] + c8[1] * Ml[:p, R:]) / 8.0          # integers below 2^53 over a power of two
    SY[:q] = (c8[2] * Ml[p:, :R] + c8[3] * Ml[p:, R:]) / 8.0
    return M, SX, SY, G.astype(np.float64)


def first(r, W, C, coef):
    """The R-form's share of a 16-column problem."""
    return W[:, :r], C[:, :r], np.asarray(coef)[:, :r]


# ------------------------------------------------------------------ plain fp64 numpy, with defects
def model(Sp, Wp, Cp, coef, ldx, defect=None):
    """The pass in plain fp64 numpy on padded inputs (M, SX, SY, G as ``Context.xprod_pass`` returns them),
    with one of the seeded DEFECTS."""
    P = Sp.shape[0]
    ldy = P - ldx
    r = Wp.shape[1]
    al, be, ga, de = (np.asarray(v, dtype=np.float64) for v in coef)
    Mw, Mc = Sp[:, :ldx] @ Wp, Sp[:, ldx:] @ Cp
    if defect == "drop_pair":             # one 16-byte column pair of one row lost at a 128-column tile edge
        c = 128 if ldx > 130 else 0
        i = int(np.argmax(np.abs(Sp[:ldx, c])))                      # an X row: M and SX move
        Mw[i] = np.delete(Sp[i, :ldx], [c, c + 1]) @ np.delete(Wp, [c, c + 1], axis=0)
    if defect == "y_offset":              # the Y phase starts 2 columns early
        Mc = Sp[:, ldx - 2:P - 2] @ Cp
    M = np.hstack([Mw, Mc])
    if defect == "row_past_P":            # a row past P (no data: modelled as a row of ones) lands on row P - 1
        M[P - 1] = np.hstack([Wp.sum(axis=0), Cp.sum(axis=0)])
    if defect == "scatter_off_by_one":    # component 0 of row 1 written to row 0 (one wave at every RW >= 2)
        M[0, 0] = Sp[1, :ldx] @ Wp[:, 0]
    Mw, Mc = M[:, :r], M[:, r:]
    if defect == "swap_ab":
        al, be = be, al
    SX = al * Mw[:ldx] + be * Mc[:ldx]
    SY = ga * Mw[ldx:] + de * Mc[ldx:]
    B = np.zeros((P, 2 * r))
    B[:ldx, :r], B[ldx:, r:] = Wp, Cp
    G = np.triu(B.T @ M)
    if defect == "gram_wrong_side":       # entry (0, r): W's column against the Y rows of M
        n = min(ldx, ldy)
        G[0, r] = Wp[:n, 0] @ M[ldx:ldx + n, r]
    G = G + np.triu(G, 1).T
    return M, SX, SY, G
