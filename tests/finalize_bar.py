"""Long-double reference and error bars for one finalize (the other half of an EM iteration).

Shared by tests/test_gpu_finalize_matrix.py (the HIP finalize against the bars) and
tests/test_finalize_bar_host.py (the bars themselves: plain fp64 lies inside, seeded defects
outside).  numpy longdouble only; u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1), every quantity below is evaluated in long double.

Polar factor.  Reference: Householder QR S = Q_h R in long double (r reflections, LAPACK's sign
convention R_kk = -sign(a_kk) ||a||, and no reflection of a last row when m = r), then the polar factor of the r x r triangle by the Newton
iteration X <- (X + X^-T) / 2 with a hand-written Gauss-Jordan inverse, iterated to a fixed point;
Q_ref = Q_h polar(R).  Type "QR": sign(R_11) Q_h (functions.R:257-259).  Its own error is 2^-11 of
an fp64 result's.  With m rows, r columns, sigma_1 >= .. >= sigma_r the singular values of S:

  c_b = 6 (m r + r (r + 1)) + 32 r^2.
      The device's factorisations are backward stable with ||dS||_F <= c_b u ||S||_F: Cholesky-QR2
      leaves ||Q'Q - I||_F <= 6 (m r u + r (r + 1) u) and a residual of 5 r^2 u ||S|| (Yamamoto,
      Nakatsukasa, Yanagisawa, Fukaya, ETNA 44 (2015), Theorems 3.1 and 3.2); Householder QR has
      sqrt(r) gamma_{c m r} (Higham, Theorem 19.4), no larger for the shapes here; the r x r work
      (two triangular products, a Jacobi SVD, U V', one r-long row product per entry of the result)
      is charged 32 r^2 u: about three dozen rounded r-long dot products per entry.
  (a) ||Q'Q - I||_F <= A = c_b u.  On the Cholesky-QR1 fast path Q = S R1^-1 polar(R1) keeps the
      orthogonality of Cholesky-QR1, (5 / 64) (8 kappa sqrt(m r u + r (r + 1) u))^2 (ibid., eq.
      (3.1)) with kappa <= kappa_F = ||R1||_F ||R1^-1||_F, the quantity the kernel tests against
      polar1_kappa: A_fast = A + 5 kappa_F^2 (m r + r (r + 1)) u.  That factor appears on this
      path only.
  (b) ||Q - Q_ref||_F <= A + c_b u ||S||_F / sigma_r: the polar factor of a full-rank rectangular
      matrix moves by at most ||dS||_F / sigma_r (Li, SIMAX 16 (1995)), and the nearest matrix
      with orthonormal columns is within A.  QR type: the Q factor moves by sqrt(2) ||dS||_F /
      sigma_r to first order (Sun, BIT 31 (1991)); the bar takes 2.
  (c) polar property, no reference: Q'S is symmetric to ||Q'S - S'Q||_F <= 2 (c_b u + A) ||S||_F
      (the skew part of Q'(S + dS) vanishes) and positive definite; QR type: the strict lower
      triangle of Q'S is within (c_b u + A) ||S||_F and (Q'S)_11 > 0.
  Floors: what tests/test_gpu_numerics.py asserts holds beside the Frobenius bars, as it states
      it, on the largest entry: (a) max|Q'Q - I| < 1e-13, (b) max|Q - Q_ref| < 1e-13 + 64 eps
      sigma_1 / sigma_r, (c) max|Q'S - S'Q| (QR: the strict lower triangle) < 1e-12 max|S|
      ("orth_max", "dist_max", "sym_max").  At all but the smallest shapes these are the tighter.
  (d) padding rows are exactly 0.
  (e) gram_nxt with exact_gram: |G - Q'Q| <= gamma_{m + 2} |Q|'|Q| entrywise, Q the returned
      loadings; without: exactly I.
  (f) the carried Jacobi V: ||V'V - I||_F <= 128 r u.  A rotation (c, s) formed from t by two
      roundings each is orthogonal to 6 u; a column takes part in r - 1 rotations a sweep, and ten
      sweeps are more than the Jacobi needs from a cold start: 12 (r - 1) u x 10 < 128 r u.  The
      re-orthonormalisation (modified Gram-Schmidt of a matrix with kappa = 1 + 1e-6) leaves less.
Nothing above is measured; the issue's fallback (8 x the error of numpy's SVD polar factor) is not
used.

Scalar block.  Expect_M's moments (EM_W_multi.R:696-716), logl_W (loglC.cpp:318-338) and
Maximiz_M's scalars with the next mu coefficients (EM_W_multi.R:734-738, :691-694) are restated
over a number type that carries, beside the long-double value, the same expression with every term
replaced by its absolute value (a / b: |a| / |b| times the condition |b|~ / |b| of the divisor;
log: |x|~ / |x| + |log x|).  The bar is k u times that second evaluation, k the rounded operations
on the longest path, counted from ppls_math.h (fma counted as two):
  coefficients c1, c2, c3: 13 (Kwc's fourth term: Kc 6, two products, a four-factor divisor, the
      quotient, three additions);
  Ctt, Cuu, Cut: c2 + 3 products + 6 additions + the Gram term = 23;  Chh: 20;
  Cee, Cff: (Z'Z)_kl W'W_lk 19, summed over r^2 pairs, ssq 4, :706 5 = 28 + r^2;
  moments: k = 32 + r^2;  log-likelihood: trace term 19, summed over r, :331-336 7, log() counted
      as 2: k = 32 + r;
  next theta: B 25, sigT 24, sigE, sigF 29 + r^2, sigH 22 + r, alpha..delta 17 more: k = 48 + r^2.
Cee and Cff cancel (||X||^2 - 2 s tr + s^2 tr): the absolute evaluation charges that to the bar.

Fused Gram: |G - B'M| <= gamma_{max(ldx, ldy) + 2} |B|'|M| entrywise, B = blockdiag(W, C) padded,
the entries the kernel forms (X rows: a < r, b >= a; Y rows: r <= a <= b) mirrored.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
EPS = 2.0 ** -52


def gamma(k):
    k = LD(k)
    return k * U / (LD(1.0) - k * U)


def fro(A):
    A = np.asarray(A, dtype=LD)
    return np.sqrt(np.sum(A * A))


# ---------------------------------------------------------------------------- long-double linear algebra
def householder_qr(S):
    """Q (m x r, orthonormal columns), R (r x r upper) of S in long double, LAPACK's signs."""
    A = np.array(S, dtype=LD)
    m, r = A.shape
    vs = []
    for k in range(r):
        x = A[k:, k]
        sig = np.sqrt(np.sum(x * x))
        alpha = -sig if x[0] >= 0 else sig
        if len(x) == 1:   # a last row has nothing to reflect (LINPACK dqrdc2 and LAPACK dlarfg: H = I)
            alpha = x[0]
        v = x.copy()
        v[0] -= alpha
        vtv = np.sum(v * v)
        vs.append((v, vtv))
        if vtv > 0:
            A[k:, k:] -= np.outer(v, (LD(2.0) / vtv) * (v @ A[k:, k:]))
    R = np.triu(A[:r, :r])
    Q = np.zeros((m, r), dtype=LD)
    Q[np.arange(r), np.arange(r)] = 1
    for k in range(r - 1, -1, -1):
        v, vtv = vs[k]
        if vtv > 0:
            Q[k:, :] -= np.outer(v, (LD(2.0) / vtv) * (v @ Q[k:, :]))
    return Q, R


def inverse(A):
    """Gauss-Jordan with partial pivoting in long double (r <= 16)."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    M = np.hstack([A, np.eye(n, dtype=LD)])
    for k in range(n):
        piv = k + int(np.argmax(np.abs(M[k:, k])))
        if M[piv, k] == 0:
            raise np.linalg.LinAlgError("singular")
        M[[k, piv]] = M[[piv, k]]
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    return M[:, n:]


def polar_small(R):
    """The orthogonal polar factor of a nonsingular r x r matrix: X <- (X + X^-T) / 2 to a fixed point."""
    X = np.array(R, dtype=LD)
    X = X / fro(X)
    best = None
    for _ in range(200):
        Xn = (X + inverse(X).T) / 2
        d = fro(Xn - X)
        X = Xn
        if best is not None and d >= best:
            break
        best = d
    return X


def singular_values(S):
    """sigma_1 >= .. >= sigma_r (fp64 of the long-double triangle is accurate enough for a bar)."""
    return np.linalg.svd(np.asarray(householder_qr(S)[1], dtype=np.float64), compute_uv=False)


def kappa_F(S):
    """||R1||_F ||R1^-1||_F of the Cholesky factor of S'S: what the kernel tests against polar1_kappa."""
    R = householder_qr(S)[1]
    return float(fro(R) * fro(inverse(R)))


class PolarRef:
    """Reference factor and bars (a) to (c) for S (m x r) and one type ("SVD" or "QR")."""

    def __init__(self, S, typ="SVD"):
        self.S = np.asarray(S, dtype=LD)
        self.typ = typ
        m, r = self.S.shape
        self.m, self.r = m, r
        Qh, R = householder_qr(self.S)
        if typ == "SVD":
            self.Q = Qh @ polar_small(R)
        else:
            self.Q = Qh * (LD(-1.0) if R[0, 0] < 0 else LD(1.0))
        sv = np.linalg.svd(np.asarray(R, dtype=np.float64), compute_uv=False)
        self.sigma1, self.sigmar = float(sv[0]), float(sv[-1])
        self.kappa2 = self.sigma1 / self.sigmar
        self.kF = float(fro(R) * fro(inverse(R)))
        self.normS = fro(self.S)
        self.cb = LD(6 * (m * r + r * (r + 1)) + 32 * r * r)

    def bars(self, fast=False):
        """{"orth", "dist", "sym"}: the Frobenius bars (a), (b), (c), fast: the Cholesky-QR1 path's; and
        {"orth_max", "dist_max", "sym_max"}: the entrywise floors."""
        m, r = self.m, self.r
        A = self.cb * U
        if fast:
            A = A + 5 * LD(self.kF) ** 2 * (m * r + r * (r + 1)) * U
        back = self.cb * U
        cond = self.normS / LD(self.sigmar)
        dist = A + (2 if self.typ == "QR" else 1) * back * cond
        sym = (2 if self.typ == "SVD" else 1) * (back + A) * self.normS
        return dict(orth=A, dist=dist, sym=sym, orth_max=LD(1e-13),
                    dist_max=LD(1e-13) + LD(64 * EPS) * LD(self.kappa2), sym_max=LD(1e-12) * np.max(np.abs(self.S)))

    def measure(self, Q):
        """{"orth", "dist", "sym"} of a computed factor (its m rows), and whether Q'S is positive
        (SVD: definite; QR: the (1, 1) entry)."""
        Q = np.asarray(Q, dtype=LD)
        if not np.all(np.isfinite(np.asarray(Q, dtype=np.float64))):
            inf = LD(np.inf)
            return dict(orth=inf, dist=inf, sym=inf, orth_max=inf, dist_max=inf, sym_max=inf), False
        r = self.r
        H = Q.T @ self.S
        E = dict(orth=Q.T @ Q - np.eye(r, dtype=LD), dist=Q - self.Q)
        if self.typ == "SVD":
            E["sym"] = H - H.T
            pos = bool(np.linalg.eigvalsh(np.asarray((H + H.T) / 2, dtype=np.float64)).min() > 0)
        else:
            E["sym"] = np.tril(H, -1)
            pos = bool(H[0, 0] > 0)
        out = {k: fro(v) for k, v in E.items()}
        out.update({k + "_max": np.max(np.abs(v)) for k, v in E.items()})
        return out, pos

    def ratios(self, Q, fast=False):
        """err / bar per quantity (<= 1 is inside) and the positivity flag."""
        got, pos = self.measure(Q)
        bars = self.bars(fast)
        return {k: float(got[k] / bars[k]) for k in got}, pos


def gram_ratio(G, Q):
    """(e): worst |G - Q'Q| / (gamma_{m + 2} |Q|'|Q|) over the entries, Q the returned loadings."""
    Q = np.asarray(Q, dtype=LD)
    ref = Q.T @ Q
    bar = gamma(Q.shape[0] + 2) * (np.abs(Q).T @ np.abs(Q))
    return _ratio(G, ref, bar)


def v_ratio(V):
    """(f): ||V'V - I||_F / (128 r u)."""
    V = np.asarray(V, dtype=LD)
    r = V.shape[0]
    if not np.all(np.isfinite(np.asarray(V, dtype=np.float64))):
        return float("inf")
    return float(fro(V.T @ V - np.eye(r, dtype=LD)) / (128 * r * U))


def _ratio(got, ref, bar):
    """max err / bar; an entry whose bar is 0 must be exact."""
    err = np.abs(np.asarray(got).astype(LD) - ref)
    if not np.all(np.isfinite(np.asarray(err, dtype=np.float64))):
        return float("inf")
    zero = bar == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float(np.max(err[~zero] / bar[~zero])) if np.any(~zero) else 0.0


# ---------------------------------------------------------------------------- inputs with a chosen path
def with_condition(rng, m, r, kappa, scale=3.7):
    """An m x r matrix with singular values geometric from scale down to scale / kappa."""
    Uu = np.linalg.qr(rng.standard_normal((m, r)))[0]
    V = np.linalg.qr(rng.standard_normal((r, r)))[0]
    s = np.geomspace(1.0, 1.0 / kappa, r) * scale if r > 1 else np.array([scale])
    return (Uu * s) @ V.T


def path_input(rng, m, r, path, bound):
    """S whose polar factor the kernel computes on `path` when polar1_kappa's bound is `bound`:
    "fast" kappa_F <= bound / 2; "qr2" kappa_F >= 2 bound, kappa_2 <= 1e5; "fb10", "fb13" kappa_2 =
    1e10, 1e13 (Cholesky-QR2 refuses).  r = 1 has kappa = 1: every path but "fast" needs r >= 2."""
    if path == "fast":
        # singular values 1 .. 1/k: kappa_F^2 = sum s^2 sum s^-2 <= r^2 k^2; k = bound / (2 r) >= 1
        k = max(1.0, min(3.0, bound / (2.0 * r)))
        return with_condition(rng, m, r, k)
    if r < 2:
        raise ValueError("one column has kappa = 1")
    return with_condition(rng, m, r, {"qr2": 1e4 if bound < 2000 else 1e5, "fb10": 1e10, "fb13": 1e13}[path])


def polar1_bound(r, polar1_kappa=0):
    """The kernel's bound on kappa_F (polar1_bound in ppls_capi.cpp): the option, or min(8 r, 40)."""
    return polar1_kappa if polar1_kappa > 0 else min(8 * r, 40)


# ---------------------------------------------------------------------------- the scalar block
class AV:
    """A long-double value and the same expression with every term replaced by its absolute value."""
    __slots__ = ("v", "a")

    def __init__(self, v, a=None):
        self.v = LD(v)
        self.a = abs(self.v) if a is None else LD(a)

    @staticmethod
    def of(x):
        return x if isinstance(x, AV) else AV(x)

    def __add__(self, o):
        o = AV.of(o)
        return AV(self.v + o.v, self.a + o.a)

    __radd__ = __add__

    def __sub__(self, o):
        o = AV.of(o)
        return AV(self.v - o.v, self.a + o.a)

    def __rsub__(self, o):
        return AV.of(o) - self

    def __neg__(self):
        return AV(-self.v, self.a)

    def __mul__(self, o):
        o = AV.of(o)
        return AV(self.v * o.v, self.a * o.a)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = AV.of(o)
        return AV(self.v / o.v, self.a / abs(o.v) * (o.a / abs(o.v)))

    def __rtruediv__(self, o):
        return AV.of(o) / self

    def sqrt(self):
        return AV(np.sqrt(self.v), np.sqrt(abs(self.v)) * (self.a / abs(self.v)) if self.v != 0 else 0)

    def log(self):
        return AV(np.log(self.v), self.a / abs(self.v) + abs(np.log(self.v)))

    def fabs(self):
        return AV(abs(self.v), self.a)


def _coef(t, b, sE, sF, sH, logl=False):
    """c1, c2, c3, Kc of ppls_coef_estep (EM_W_multi.R:670-686) / ppls_coef_logl (:312-320)."""
    t2 = t * t
    t4 = t2 * t2
    t6 = t4 * t2
    b2 = b * b
    sE2, sF2 = sE * sE, sF * sF
    g = t2 * b2 + sH * sH
    if logl:
        gs = g.sqrt()
        g = gs * gs
    Kw = t2 - t4 * b2 / sF2 + t4 * b2 * g / (sF2 * (g + sF2))
    Kc = g - t4 * b2 / sE2 + t6 * b2 / (sE2 * (t2 + sE2))
    Kwc = (t2 * b / (sE2 * sF2) - Kc * t2 * b / (sE2 * sF2 * (Kc + sF2)) - t4 * b / (sE2 * sF2 * (t2 + sE2)) +
           Kc * t4 * b / (sE2 * sF2 * (Kc + sF2) * (t2 + sE2)))
    return Kw / (sE2 * (Kw + sE2)), Kwc, Kc / (sF2 * (Kc + sF2)), Kc


def _mu_coef(t, b, sE, sF, sH):
    c1, c2, c3, _ = _coef(t, b, sE, sF, sH)
    t2 = t * t
    v = t2 * b * b + sH * sH
    iE, iF = 1 / (sE * sE), 1 / (sF * sF)
    return (iE * t2 - c1 * t2 - c2 * t2 * b, iF * t2 * b - c2 * t2 - c3 * b * t2,
            iE * t2 * b - c1 * t2 * b - c2 * v, iF * v - c2 * t2 * b - c3 * v)


class ScalarRef:
    """The scalar block's outputs in long double with their bars, from what the kernel takes: the Gram
    G (2r x 2r), W'W, C'C, ssq, N, p, q and theta's scalars (B, sigT, sigE, sigF, sigH and the
    alpha..delta the library staged: ``coef`` = (alpha, beta, gamma, delta))."""

    def __init__(self, G, WtW, CtC, ssqX, ssqY, N, p, q, B, sigT, sigE, sigF, sigH, coef):
        r = len(B)
        self.r = r
        Gm = [[AV(G[i, j]) for j in range(2 * r)] for i in range(2 * r)]
        A = lambda k, l: Gm[k][l]           # noqa: E731
        D = lambda k, l: Gm[k][r + l]       # noqa: E731
        Bm = lambda k, l: Gm[r + k][r + l]  # noqa: E731
        t = [AV(x) for x in sigT]
        b = [AV(x) for x in B]
        sE, sF, sH = AV(sigE), AV(sigF), AV(sigH)
        N = AV(N)
        al, be, ga, de = ([AV(x) for x in c] for c in coef)
        sE2, sF2, sH2 = sE * sE, sF * sF, sH * sH
        iE, iF = 1 / sE2, 1 / sF2
        cs = [_coef(t[k], b[k], sE, sF, sH) for k in range(r)]
        Ctt, Cuu, Cut = [], [], []
        xz = yz = sc1 = sc3 = AV(0)
        for k in range(r):
            c1, c2, c3, _ = cs[k]
            t2 = t[k] * t[k]
            t4 = t2 * t2
            b2 = b[k] * b[k]
            v = t2 * b2 + sH2
            tt = al[k] * al[k] * A(k, k) + 2 * al[k] * be[k] * D(k, k) + be[k] * be[k] * Bm(k, k)
            uu = ga[k] * ga[k] * A(k, k) + 2 * ga[k] * de[k] * D(k, k) + de[k] * de[k] * Bm(k, k)
            ut = ga[k] * al[k] * A(k, k) + (ga[k] * be[k] + de[k] * al[k]) * D(k, k) + de[k] * be[k] * Bm(k, k)
            Ctt.append((t2 - iE * t4 - iF * (t4 * b2) + t4 * c1 + 2 * (t4 * b[k] * c2) + t4 * b2 * c3 + tt / N).fabs())
            Cuu.append((v - iE * (t4 * b2) - iF * (v * v) + t4 * b2 * c1 + 2 * (t2 * b[k] * v * c2) + v * v * c3 +
                        uu / N).fabs())
            Cut.append(t2 * b[k] - iE * (t4 * b[k]) - iF * (t2 * b[k] * v) + t4 * b[k] * c1 + t2 * v * c2 +
                       t4 * b2 * c2 + t2 * b[k] * v * c3 + ut / N)
            xz = xz + (c1 * A(k, k) + c2 * D(k, k))
            yz = yz + (c3 * Bm(k, k) + c2 * D(k, k))
            sc1 = sc1 + c1
            sc3 = sc3 + c3
        zz = ww = AV(0)
        Chh = [[None] * r for _ in range(r)]
        for l in range(r):
            for k in range(r):
                c1k, c2k, c3k, _ = cs[k]
                c1l, c2l, c3l, _ = cs[l]
                zkl = c1k * c1l * A(k, l) + c1k * c2l * D(k, l) + c2k * c1l * D(l, k) + c2k * c2l * Bm(k, l)
                fkl = c3k * c3l * Bm(k, l) + c3k * c2l * D(l, k) + c2k * c3l * D(k, l) + c2k * c2l * A(k, l)
                zz = zz + zkl * AV(WtW[l, k])
                ww = ww + fkl * AV(CtC[l, k])
                h1k, h2k = iF * sH2 - sH2 * c3k, -(sH2 * c2k)
                h1l, h2l = iF * sH2 - sH2 * c3l, -(sH2 * c2l)
                hh = h1k * h1l * Bm(k, l) + h1k * h2l * D(l, k) + h2k * h1l * D(k, l) + h2k * h2l * A(k, l)
                vv = hh / N
                if k == l:
                    vv = (sH2 - sH2 * sH2 / sF2) + sH2 * sH2 * c3k + vv
                Chh[k][l] = vv.fabs()
        ssqE = AV(ssqX) - 2 * sE2 * xz + sE2 * sE2 * zz
        ssqF = AV(ssqY) - 2 * sF2 * yz + sF2 * sF2 * ww
        pd, qd = AV(p), AV(q)
        Cee = (pd * sE2 - pd * sE2 + sE2 * sE2 * sc1 + ssqE / N) / pd
        Cff = (qd * sF2 - qd * sF2 + sF2 * sF2 * sc3 + ssqF / N) / qd
        # log-likelihood (loglC.cpp:318-338)
        logs = trk = AV(0)
        for k in range(r):
            c1, c2, c3, Kc = _coef(t[k], b[k], sE, sF, sH, logl=True)
            logs = logs + ((sE2 + t[k] * t[k]).log() + (sF2 + Kc).log())
            trk = trk + (-(c1 * A(k, k)) - 2 * c2 * D(k, k) - c3 * Bm(k, k))
        logdet = logs + AV(p - r) * sE2.log() + AV(q - r) * sF2.log()
        traceL = 1 / sE2 * AV(ssqX) + 1 / sF2 * AV(ssqY) + trk
        twopi = AV(2 * np.arccos(LD(-1.0))).log()
        logl = -(AV(0.5) * N * AV(p + q) * twopi) - AV(0.5) * N * logdet - AV(0.5) * traceL
        # Maximiz_M (EM_W_multi.R:734-738) and the next mu coefficients
        nb = [Cut[k] * (1 / Ctt[k]) for k in range(r)]
        nt = [Ctt[k].sqrt() for k in range(r)]
        trChh = AV(0)
        for k in range(r):
            trChh = trChh + Chh[k][k]
        nE, nF, nH = Cee.sqrt(), Cff.sqrt(), (trChh / AV(r)).sqrt()
        mu = [_mu_coef(nt[k], nb[k], nE, nF, nH) for k in range(r)]
        km, kl, kn = 32 + r * r, 32 + r, 48 + r * r
        vec = lambda xs: (np.array([x.v for x in xs], dtype=LD), np.array([x.a for x in xs], dtype=LD))  # noqa: E731
        self.out = {}

        def put(name, xs, k):
            v, a = vec(xs)
            self.out[name] = (v, k * U * a)

        put("Ctt", Ctt, km)
        put("Cuu", Cuu, km)
        put("Cut", Cut, km)
        put("Cee", [Cee], km)
        put("Cff", [Cff], km)
        put("Chh", [Chh[k][l] for l in range(r) for k in range(r)], km)   # column-major
        put("loglik", [logl], kl)
        put("B", nb, kn)
        put("sigT", nt, kn)
        put("sigE", [nE], kn)
        put("sigF", [nF], kn)
        put("sigH", [nH], kn)
        for i, name in enumerate(("alpha", "beta", "gamma", "delta")):
            put(name, [m[i] for m in mu], kn)

    def ratios(self, got):
        """got: {name: array}; worst err / bar per name present in got."""
        out = {}
        for name, val in got.items():
            ref, bar = self.out[name]
            out[name] = _ratio(np.ravel(np.asarray(val, dtype=np.float64)), ref, bar)
        return out


# ---------------------------------------------------------------------------- the fused Gram
def fused_gram_ref(W, C, M, ldx, ldy):
    """B'M as the scalar block forms it from M ((ldx + ldy) x 2r) and the loadings W (p x r), C
    (q x r), in long double with its entrywise bar: X rows give (a, b), a < r, b in [a, 2r); Y rows
    (r + a, r + b), a <= b < r; both mirrored."""
    r = W.shape[1]
    p, q = W.shape[0], C.shape[0]
    Ml = np.asarray(M, dtype=LD)
    Wl = np.zeros((ldx, r), dtype=LD)
    Wl[:p] = W
    Cl = np.zeros((ldy, r), dtype=LD)
    Cl[:q] = C
    G = np.zeros((2 * r, 2 * r), dtype=LD)
    bar = np.zeros((2 * r, 2 * r), dtype=LD)
    gx = Wl.T @ Ml[:ldx, :]                      # r x 2r
    bx = np.abs(Wl).T @ np.abs(Ml[:ldx, :])
    gy = Cl.T @ Ml[ldx:, r:]                     # r x r
    by = np.abs(Cl).T @ np.abs(Ml[ldx:, r:])
    for a in range(r):
        for b in range(a, 2 * r):
            G[a, b] = G[b, a] = gx[a, b]
            bar[a, b] = bar[b, a] = bx[a, b]
        for b in range(a, r):
            G[r + a, r + b] = G[r + b, r + a] = gy[a, b]
            bar[r + a, r + b] = bar[r + b, r + a] = by[a, b]
    return G, gamma(max(ldx, ldy) + 2) * bar


def fused_gram_ratio(got, W, C, M, ldx, ldy):
    ref, bar = fused_gram_ref(W, C, M, ldx, ldy)
    return _ratio(got, ref, bar)


# ---------------------------------------------------------------------------- the matrix's shapes
TEAM_T = 64   # option team_rows of the team cases.  The option accepts any positive count, but a member
              # needs rows to split: 64 (one wave) is the smallest at which 4 T - 3 >= r for every r and
              # both team shapes below stay a few thousand rows
STAGE_MAX = 136 * 1024   # PPLS_FIN_STAGE_MAX: the largest staging budget an instantiation can report
# name -> (p, q, team_rows, KX, KY); q = max(q, r) at r components (shape_pq)
GEOMETRY = {
    "small": (9, 12, 0, 1, 1),
    "mid": (500, 390, 0, 1, 1),
    "team4": (4 * TEAM_T - 3, 12, TEAM_T, 4, 1),                     # 253 = 63 + 63 + 63 + 64 rows, odd
    "team2": (4 * TEAM_T - 3, 12, 2 * TEAM_T, 2, 1),                 # the same rows over 2 and over 16 members:
    "team16": (4 * TEAM_T - 3, 12, TEAM_T // 4, 16, 1),              # where r = 10 loses orthogonality (see the GPU test)
    "team4x2": (4 * TEAM_T - 3, 2 * TEAM_T - 1, TEAM_T, 4, 2),
    "team32": (32 * TEAM_T + 5, 12, TEAM_T, 32, 1),                  # 33 members asked, 32 given; 2053
    "team32x2": (32 * TEAM_T + 5, 2 * TEAM_T - 1, TEAM_T, 32, 2),    # columns pad to 2560: 507 padding rows
}
TEAM_UNSTAGED = (2 * 2048 - 3, 12, 0, 2, 1)   # r = 10, default team_rows: members of 2046 and 2047 rows


def shape_pq(p, q, r):
    return p, max(q, r)


def unstaged_p(r, budget=STAGE_MAX):
    """The smallest p one block cannot stage at r components: r p 8 > budget."""
    return budget // (8 * r) + 1


def padded_width(p):
    """ld_of in ppls_capi.cpp for fp64 storage."""
    if p * 8 < 1024 or p <= 2048:
        return (p + 1) & ~1
    al = 4096 if p * 8 >= 16384 else 128
    return (p * 8 + al - 1) // al * al // 8


def scalar_problem(p, q, r, seed, n=24):
    """What the scalar block takes, from a small data set: theta with sigE, sigF above sigT (the
    coefficient formulas are then well conditioned, as sweep_bar.sweep_problem argues) and loadings on
    a 2^-10 grid, not orthonormal -- W'W and C'C are then exact in fp64 in any summation order and
    their off-diagonal entries matter; the Gram of [XW YC] plus a relative 1e-3 of asymmetric noise,
    so that an index pair taken the wrong way round shows."""
    rng = np.random.default_rng(seed)
    W = np.round((np.linalg.qr(rng.standard_normal((p, r)))[0] + 0.1 * rng.standard_normal((p, r))) * 1024) / 1024
    C = np.round((np.linalg.qr(rng.standard_normal((q, r)))[0] + 0.1 * rng.standard_normal((q, r))) * 1024) / 1024
    X = rng.standard_normal((n, p))
    Y = rng.standard_normal((n, q)) + X[:, :1]
    Z = np.hstack([X @ W, Y @ C])
    G = Z.T @ Z
    G = G * (1 + 1e-3 * rng.standard_normal(G.shape))
    th = dict(W=W, C=C, B=np.diag(np.linspace(1.2, 0.7, r)), sigE=2.0, sigF=1.7, sigH=0.9,
              sigT=np.diag(np.linspace(1.1, 0.6, r)))
    return dict(X=X, Y=Y, th=th, G=G, WtW=W.T @ W, CtC=C.T @ C, ssqX=float(np.sum(X * X)), ssqY=float(np.sum(Y * Y)),
                N=float(n), p=p, q=q)
