"""Reference, a-priori error bars and a host model of the row diagnostics kernel, shared by
tests/test_rowdiag_host.py and tests/test_gpu_diagnostics.py.

Per row (x, y) and theta with a = W'x, b = C'y the kernel returns odx2 = ||x - W a||^2, ody2 = ||y - C b||^2,
sd2 = sum_m (s22 a^2 - 2 s12 a b + s11 b^2) / det and mu_T = alpha a + beta b, mu_U = gamma a + delta b; the
library then forms d2 = (odx2 / sigE^2 + ody2 / sigF^2) + sd2 and loglik = cst - d2 / 2 on the host.

Reference (``reference``): the same quantities in long double from the W, C and scalars actually passed (fp64
values, not re-orthonormalised), for fp32 storage over the rows rounded to fp32.  The mu coefficients are the
library's own (ppls_mu_coefficients, a host function): the kernel applies them, it does not derive them.

The kernel's order and the bar (``bars``), with u = 2^-53 and gamma(n) = n u / (1 - n u):

* scores.  Lane l holds the 16-byte units l, l + 64, .. of the row (VE = 2 doubles or 4 floats each) and adds
  their products to one accumulator: at most L1 = VE ceil(units / 64) roundings behind a term (fused or not),
  then the six-level tree: Ea_m = gamma(L1 + K_TREE) sum_j |x_j| |w_jm|.
* residual.  e_j = x_j - sum_m a_m w_jm, component after component: at most k + 1 roundings behind a term,
  plus what the error of the scores moves it:
      de_j = gamma(k + 1) (|x_j| + sum_m (|a_m| + Ea_m) |w_jm|) + sum_m Ea_m |w_jm|.
* norm.  The squares of a lane's units, one addition per lane sweep, the tree: L1 + sweeps + K_TREE + 1
  roundings behind a square.  With ||.|| the 2-norm over j
      bar(odx2) = gamma(L1 + sweeps + K_TREE + 1) (||e|| + ||de||)^2 + 2 ||e|| ||de|| + ||de||^2.
  The reference forms the same residual from the same W, so this needs no orthonormality of W.
* 2 x 2 forms.  The library's s11, s12, s22 and det (formed as t^2 (sH^2 + sF^2) + sE^2 s22, every term
  non-negative) carry at most K_FORM roundings each; a term's products, sums and division K_TERM more and the
  tree over the tile log2(KT) <= 4: with T_m = (s22 a^2 + 2 |s12| |a| |b| + s11 b^2) / det
      bar(sd2) = gamma(2 K_FORM + K_TERM + 4) sum_m T_m
                 + sum_m [s22 (2|a| Ea + Ea^2) + 2 |s12| (|a| Eb + |b| Ea + Ea Eb) + s11 (2|b| Eb + Eb^2)] / det.
* mu.  bar(mu_T) = |alpha| Ea + |beta| Eb + gamma(K_MU) (|alpha| |a| + |beta| |b|), K_MU = 3 (two products, a sum).
* d2.  sigE^2, two divisions, two additions: bar(d2) = bar(odx2) / sE2 + bar(ody2) / sF2 + bar(sd2)
  + gamma(K_D2) (odx2 / sE2 + ody2 / sF2 + |sd2|).
* loglik = cst - d2 / 2 with cst = -((p+q) log 2pi + (p-r) log sE2 + (q-r) log sF2 + sum log det) / 2: the
  logarithms' arguments carry K_FORM roundings (a relative error of an argument is an absolute one of its
  logarithm), the logarithms and their sum K_CST roundings of the absolute sum:
      bar(loglik) = bar(d2) / 2 + gamma(K_CST) |cst|_abs + gamma(K_FORM) (p + q) / 2 + 2 u |loglik|.

An input perturbation (``dX``, ``dY``: elementwise bounds, for rows that reach the kernel through another
chain of roundings) moves a_m by sum_j dx_j |w_jm| and e_j by dx_j on top: both are added to Ea and de.

Orthonormality.  The existing entries (ppls_loglik, loglC_fast) use ||x||^2 - ||a||^2 for the residual norm,
which equals ||x - W a||^2 only for W'W = I: ||x - W a||^2 = ||x||^2 - ||a||^2 + a'(W'W - I) a.  A comparison
with them therefore carries ``orth_term`` = ||W'W - I||_2 ||a||^2 / sE2 + ||C'C - I||_2 ||b||^2 / sF2 of the W and C
actually passed (not exactly orthonormal in fp64); the comparison with the long-double reference does not.
"""
import ctypes as ct
import math

import numpy as np

U = 2.0 ** -53
L = np.longdouble

K_TREE = 6     # levels of the wave tree
K_FORM = 6     # roundings behind any of s11, s12, s22, det, sE2, sF2 as the library forms them
K_TERM = 6     # a component's term of sd2: squares / product, three scalings, two sums, the division
K_MU = 3
K_D2 = 5
K_CST = 8      # four logarithm groups, their weights, the sum, the halving
K_ENTRY = 4    # stages of an existing entry's own sum over all rows (sums of squares, Gram, algebra, combination)
K_SCALE = 16   # roundings of gamma(n) size between two device scalings of one data set (see rescale_perturbation)


def gamma(n):
    return n * U / (1.0 - n * U)


def tile_of(r):
    return 8 if r <= 8 else 16


SHORT_ROW_BYTES = 16384


def rows_per_wave(r, p, q, f32):
    """Rows a wave owns at a time (ppls_rowdiag_rows_per_wave): four for k <= 16; for k <= 8 two while the
    longer row of a block is at most 16 KB, four beyond."""
    if r > 8:
        return 4
    return 2 if max(p, q) * (4 if f32 else 8) <= SHORT_ROW_BYTES else 4


def lane_terms(cols, f32):
    """(L1, sweeps, units): terms a lane adds per row, its sweeps over the row, the row's 16-byte units."""
    ve = 4 if f32 else 2
    units = -(-cols // ve)
    sweeps = -(-units // 64)
    return ve * sweeps, sweeps, units


def stored(A, f32):
    A = np.asarray(A, dtype=np.float64)
    return A.astype(np.float32).astype(np.float64) if f32 else A


def theta_parts(th):
    """W, C, b, t (vectors) and sigE, sigF, sigH as fp64 from a Theta or a dict of the reference's shapes."""
    g = (lambda k: th[k]) if isinstance(th, dict) else (lambda k: getattr(th, k))
    W = np.array(g("W"), dtype=np.float64, ndmin=2)
    C = np.array(g("C"), dtype=np.float64, ndmin=2)
    b = np.asarray(g("B"), dtype=np.float64)
    t = np.asarray(g("sigT"), dtype=np.float64)
    b = np.diag(b).copy() if b.ndim == 2 else np.ravel(b).copy()
    t = np.diag(t).copy() if t.ndim == 2 else np.ravel(t).copy()
    return W, C, b, t, float(np.ravel(g("sigE"))[0]), float(np.ravel(g("sigF"))[0]), float(np.ravel(g("sigH"))[0])


def forms(th, dtype=L):
    """s11, s12, s22, det per component and sE2, sF2 in ``dtype`` (det in its cancellation-free form)."""
    _, _, b, t, sE, sF, sH = theta_parts(th)
    b, t = b.astype(dtype), t.astype(dtype)
    sE2, sF2, sH2 = dtype(sE) * dtype(sE), dtype(sF) * dtype(sF), dtype(sH) * dtype(sH)
    t2 = t * t
    s11 = t2 + sE2
    s12 = b * t2
    s22 = b * b * t2 + sH2 + sF2
    det = t2 * (sH2 + sF2) + sE2 * s22
    return s11, s12, s22, det, sE2, sF2


def mu_coef(th):
    """alpha, beta, gamma, delta (r each) from the library's host function ppls_mu_coefficients."""
    from ppls_amd import _lib
    _, _, b, t, sE, sF, sH = theta_parts(th)
    r = b.shape[0]
    bb, tt = np.ascontiguousarray(b), np.ascontiguousarray(t)
    s = _lib.PplsTheta(None, None, _lib.dptr(bb), _lib.dptr(tt), sE, sF, sH)
    out = np.zeros(4 * r)
    rc = _lib.lib().ppls_mu_coefficients(ct.byref(s), r, _lib.dptr(out))
    assert rc == 0
    return out[:r], out[r:2 * r], out[2 * r:3 * r], out[3 * r:]


def log_constant(th, p, q, dtype=L):
    """(cst, |cst|_abs): loglik_i = cst - d2_i / 2, and the absolute sum of cst's terms."""
    s11, s12, s22, det, sE2, sF2 = forms(th, dtype)
    r = det.shape[0]
    ld = np.log(det)
    terms = [dtype(p + q) * np.log(dtype(2) * dtype(np.pi)), dtype(p - r) * np.log(sE2), dtype(q - r) * np.log(sF2), ld.sum()]
    cabs = float(abs(terms[0]) + abs(terms[1]) + abs(terms[2]) + np.abs(ld).sum()) / 2
    return -(terms[0] + terms[1] + terms[2] + terms[3]) / dtype(2), cabs


def reference(X, Y, th, f32=False):
    """Every output in long double (module docstring)."""
    W, C, b, t, sE, sF, sH = theta_parts(th)
    Xl, Yl, Wl, Cl = stored(X, f32).astype(L), stored(Y, f32).astype(L), W.astype(L), C.astype(L)
    a, bb = Xl @ Wl, Yl @ Cl
    ex, ey = Xl - a @ Wl.T, Yl - bb @ Cl.T
    odx2, ody2 = (ex * ex).sum(axis=1), (ey * ey).sum(axis=1)
    s11, s12, s22, det, sE2, sF2 = forms(th, L)
    sd2 = ((s22 * a * a - 2 * s12 * a * bb + s11 * bb * bb) / det).sum(axis=1)
    d2 = odx2 / sE2 + ody2 / sF2 + sd2
    cst, _ = log_constant(th, X.shape[1], Y.shape[1], L)
    al, be, ga, de = (v.astype(L) for v in mu_coef(th))
    return dict(a=a, b=bb, odx2=odx2, ody2=ody2, sd2=sd2, d2=d2, loglik=cst - d2 / 2, mu_T=a * al + bb * be,
                mu_U=a * ga + bb * de)


def _block_bar(Xs, W, f32, dX):
    """(Ea n x k, bar of the squared residual norm n) of one block, in float64 arithmetic on long-double inputs."""
    k = W.shape[1]
    L1, sweeps, _ = lane_terms(Xs.shape[1], f32)
    aX, aW = np.abs(Xs).astype(L), np.abs(W).astype(L)
    a = Xs.astype(L) @ W.astype(L)
    Ea = gamma(L1 + K_TREE) * (aX @ aW)
    de = gamma(k + 1) * (aX + (np.abs(a) + Ea) @ aW.T) + Ea @ aW.T
    if dX is not None:
        dXl = np.asarray(dX, dtype=np.float64).astype(L)
        Ea = Ea + dXl @ aW
        de = de + dXl + (dXl @ aW) @ aW.T
    e = Xs.astype(L) - a @ W.astype(L).T
    ne, nde = np.sqrt((e * e).sum(axis=1)), np.sqrt((de * de).sum(axis=1))
    bar = gamma(L1 + sweeps + K_TREE + 1) * (ne + nde) ** 2 + 2 * ne * nde + nde ** 2
    return a, Ea, bar


def bars(X, Y, th, f32=False, dX=None, dY=None):
    """The a-priori bar of every output as float64 arrays (module docstring)."""
    W, C, b, t, sE, sF, sH = theta_parts(th)
    p, q, k = W.shape[0], C.shape[0], W.shape[1]
    a, Ea, bx = _block_bar(stored(X, f32), W, f32, dX)
    bb, Eb, by = _block_bar(stored(Y, f32), C, f32, dY)
    s11, s12, s22, det, sE2, sF2 = forms(th, L)
    A, B = np.abs(a), np.abs(bb)
    T = (s22 * A * A + 2 * np.abs(s12) * A * B + s11 * B * B) / det
    move = (s22 * (2 * A * Ea + Ea * Ea) + 2 * np.abs(s12) * (A * Eb + B * Ea + Ea * Eb) + s11 * (2 * B * Eb + Eb * Eb)) / det
    bsd = gamma(2 * K_FORM + K_TERM + 4) * T.sum(axis=1) + move.sum(axis=1)
    ref = reference(X, Y, th, f32)
    bd2 = bx / sE2 + by / sF2 + bsd + gamma(K_D2) * (ref["odx2"] / sE2 + ref["ody2"] / sF2 + np.abs(ref["sd2"]))
    _, cabs = log_constant(th, p, q, L)
    bll = bd2 / 2 + gamma(K_CST) * cabs + gamma(K_FORM) * (p + q) / 2 + 2 * U * np.abs(ref["loglik"])
    al, be, ga, de = (np.abs(v).astype(L) for v in mu_coef(th))
    bT = al * Ea + be * Eb + gamma(K_MU) * (al * A + be * B)
    bU = ga * Ea + de * Eb + gamma(K_MU) * (ga * A + de * B)
    f = lambda v: np.asarray(v, dtype=np.float64)   # noqa: E731
    return dict(odx2=f(bx), ody2=f(by), sd2=f(bsd), d2=f(bd2), loglik=f(bll), mu_T=f(bT), mu_U=f(bU))


def orth_term(X, Y, th, f32=False):
    """Per row: ||W'W - I||_2 ||a||^2 / sE2 + ||C'C - I||_2 ||b||^2 / sF2 of the W, C passed (module docstring)."""
    W, C, *_ = theta_parts(th)
    ref = reference(X, Y, th, f32)
    *_, sE2, sF2 = forms(th, L)
    k = W.shape[1]
    ow = np.linalg.norm(np.asarray(W.astype(L).T @ W.astype(L) - np.eye(k), dtype=np.float64), 2)
    oc = np.linalg.norm(np.asarray(C.astype(L).T @ C.astype(L) - np.eye(k), dtype=np.float64), 2)
    return np.asarray(ow * (ref["a"] ** 2).sum(axis=1) / sE2 + oc * (ref["b"] ** 2).sum(axis=1) / sF2, dtype=np.float64)


def loglik_sum_bar(X, Y, th, f32=False):
    """Bar of sum_i loglik_i against an existing entry's logl_W over the same n rows: the rows' own bars, the
    n additions of the sum, the entry's own sums (K_ENTRY stages of gamma(n + p + q) of the absolute sum
    (||X||_F^2 / sE2 + ||Y||_F^2 / sF2 + sum_i sum_m T_im) / 2 + n |cst|_abs, which its expanded form adds and
    subtracts) and half the orthonormality term."""
    W, C, *_ = theta_parts(th)
    n, p, q = X.shape[0], W.shape[0], C.shape[0]
    ref, br = reference(X, Y, th, f32), bars(X, Y, th, f32)
    s11, s12, s22, det, sE2, sF2 = forms(th, L)
    A, B = np.abs(ref["a"]), np.abs(ref["b"])
    T = ((s22 * A * A + 2 * np.abs(s12) * A * B + s11 * B * B) / det).sum()
    Xs, Ys = stored(X, f32).astype(L), stored(Y, f32).astype(L)
    _, cabs = log_constant(th, p, q, L)
    mag = ((Xs * Xs).sum() / sE2 + (Ys * Ys).sum() / sF2 + T) / 2 + n * cabs
    return float(br["loglik"].sum() + gamma(n) * np.abs(ref["loglik"]).sum() + K_ENTRY * gamma(n + p + q) * mag +
                 orth_term(X, Y, th, f32).sum() / 2)


def estep_mu_bar(X, Y, th, f32=False):
    """Bars of mu_T, mu_U against Expect_M's (ppls_estep): this kernel's bars plus the entry's own scores,
    p (or q) products added in whatever order: gamma(p + K_TREE) of the absolute sums, through the same
    coefficients."""
    W, C, *_ = theta_parts(th)
    br = bars(X, Y, th, f32)
    aX, aY = np.abs(stored(X, f32)).astype(L), np.abs(stored(Y, f32)).astype(L)
    Ea = gamma(W.shape[0] + K_TREE) * (aX @ np.abs(W).astype(L))
    Eb = gamma(C.shape[0] + K_TREE) * (aY @ np.abs(C).astype(L))
    al, be, ga, de = (np.abs(v).astype(L) for v in mu_coef(th))
    ref = reference(X, Y, th, f32)
    A, B = np.abs(ref["a"]), np.abs(ref["b"])
    bT = br["mu_T"] + np.asarray(al * Ea + be * Eb + gamma(K_MU) * (al * A + be * B), dtype=np.float64)
    bU = br["mu_U"] + np.asarray(ga * Ea + de * Eb + gamma(K_MU) * (ga * A + de * B), dtype=np.float64)
    return bT, bU


def rescale_perturbation(Xraw, center, scale, n_total):
    """Elementwise bound on the difference between rows scaled on the host, (x - c) / s with the centre and
    scale of one context, and the same rows as another context of the same data holds them after its own
    device scaling.  Both centres are sums of n_total values and both scales roots of sums of n_total
    squares, each within K_SCALE / 2 stages of gamma(n_total) of the exact one (the streamed S counts 7,
    tests/test_stream_host.py; the resident passes fewer), and the element itself sees a subtraction and a
    division (or a product with a rounded reciprocal) on either side, 6 roundings in all:
        dx' = gamma(6) |x'| + K_SCALE gamma(n_total) (mean_i |x_i| / s + |x'|)."""
    Xraw = np.asarray(Xraw, dtype=np.float64)
    xs = np.abs((Xraw - center) / scale)
    return gamma(6) * xs + K_SCALE * gamma(max(int(n_total), 1)) * (np.abs(Xraw).mean(axis=0) / scale + xs)


def inside(val, ref, bar):
    """Whether val lies within the bar of the long-double ref, and the largest error in units of the bar."""
    err = np.asarray(np.abs(np.asarray(val, dtype=np.float64).astype(L) - ref), dtype=np.float64)
    bar = np.asarray(bar, dtype=np.float64)
    if err.size == 0:
        return True, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return bool(np.all(err <= bar)) and bool(np.all(np.isfinite(np.asarray(val, dtype=np.float64)))), float(ratio.max())


def pvalue_bar(stat, df, bar_stat):
    """Bar of an upper chi-square tail whose statistic is known within bar_stat: the density's maximum over
    [stat - bar, stat + bar] (at an end or, inside, at the mode df - 2) times bar_stat, plus 64 u p for the
    incomplete gamma function's own evaluation."""
    import scipy.special
    stat = np.asarray(stat, dtype=np.float64)
    bar_stat = np.asarray(bar_stat, dtype=np.float64)
    if df <= 0:
        return np.zeros_like(stat)

    def pdf(x):
        x = np.maximum(x, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            lp = (0.5 * df - 1.0) * np.log(0.5 * x) - 0.5 * x - scipy.special.gammaln(0.5 * df)
        return np.where(x > 0, 0.5 * np.exp(lp), 0.5 if df == 2 else (np.inf if df < 2 else 0.0))

    lo, hi = stat - bar_stat, stat + bar_stat
    mode = max(df - 2.0, 0.0)
    dens = np.maximum(pdf(lo), pdf(hi))
    dens = np.where((lo <= mode) & (mode <= hi), np.maximum(dens, pdf(np.full_like(stat, mode))), dens)
    return dens * bar_stat + 64 * U * scipy.special.gammaincc(0.5 * df, 0.5 * np.maximum(stat, 0.0))


# ------------------------------------------------------------------------------------ host model
def _tree(v, width, nv=None):
    """The xor tree over the last axis (length ``width``, a power of two): partners differing in the top bit
    first; with ``nv`` (the scores of a wave's row group) the bits nv / 2 .. 1 first, then 32 .. nv, as the
    reduce-scatter takes them.  Every slot ends with the same bits (a + b == b + a)."""
    idx = np.arange(width)
    bits = [h for h in (32, 16, 8, 4, 2, 1) if h < width]
    if nv is not None:
        bits = [h for h in bits if h < nv] + [h for h in bits if h >= nv]
    for h in bits:
        v = v + v[..., idx ^ h]
    return v[..., 0]


def _model_block(Xs, W, f32, nv, drop_last_unit=False, expand=False):
    """(a, r2) of one block in the kernel's order, plain fp64 (products and sums rounded separately)."""
    ve = 4 if f32 else 2
    n, cols = Xs.shape
    k = W.shape[1]
    L1, sweeps, units = lane_terms(cols, f32)
    if drop_last_unit and cols % ve:
        units -= 1                                   # defect 1: the row's last, partial unit is not read
    width = sweeps * 64 * ve
    Xp, Wp = np.zeros((n, width)), np.zeros((width, k))
    keep = min(cols, units * ve)
    Xp[:, :keep], Wp[:keep] = Xs[:, :keep], W[:keep]
    Xu, Wu = Xp.reshape(n, sweeps, 64, ve), Wp.reshape(sweeps, 64, ve, k)
    acc = np.zeros((n, 64, k))
    for s in range(sweeps):
        for e in range(ve):
            acc = acc + Xu[:, s, :, e, None] * Wu[None, s, :, e, :]
    a = _tree(np.moveaxis(acc, 1, -1), 64, nv)         # n x k
    if expand:                                           # defect 4: ||x||^2 - ||a||^2
        return a, (Xs * Xs).sum(axis=1) - (a * a).sum(axis=1)
    E = Xu.copy()
    for m in range(k):
        E = E - a[:, None, None, None, m] * Wu[None, :, :, :, m]
    r2 = np.zeros((n, 64))
    for s in range(sweeps):
        sq = np.zeros((n, 64))
        for e in range(ve):
            sq = sq + E[:, s, :, e] * E[:, s, :, e]
        r2 = r2 + sq
    return a, _tree(r2, 64)


def host_model(X, Y, th, f32=False, want_mu=True, defect=None):
    """The kernel's outputs and the library's d2, loglik from a plain fp64 evaluation in the kernel's order.
    ``defect``: None, or one of the seeded defects "drop_unit", "group_first", "s12_sign", "expand_x"."""
    W, C, b, t, sE, sF, sH = theta_parts(th)
    k = W.shape[1]
    rw = rows_per_wave(k, W.shape[0], C.shape[0], f32)
    nv = rw * tile_of(k)
    a, rx = _model_block(stored(X, f32), W, f32, nv, defect == "drop_unit", defect == "expand_x")
    bb, ry = _model_block(stored(Y, f32), C, f32, nv, defect == "drop_unit")
    s11, s12, s22, det, sE2, sF2 = forms(th, np.float64)
    if defect == "s12_sign":
        s12 = -s12
    kt = tile_of(k)
    term = np.zeros((a.shape[0], kt))
    term[:, :k] = ((s22 * (a * a) - 2.0 * s12 * (a * bb)) + s11 * (bb * bb)) / det
    sd2 = _tree(term, kt)
    al, be, ga, de = mu_coef(th)
    out = dict(odx2=rx, ody2=ry, sd2=sd2, mu_T=al * a + be * bb, mu_U=ga * a + de * bb)
    if defect == "group_first":                          # rows of a partial last group take the group's first row
        n = a.shape[0]
        g0 = (n // rw) * rw
        if g0 < n:
            for key in out:
                out[key] = out[key].copy()
                out[key][g0:] = out[key][g0]
    cst, _ = log_constant(th, W.shape[0], C.shape[0], np.float64)
    out["d2"] = (out["odx2"] / sE2 + out["ody2"] / sF2) + out["sd2"]
    out["loglik"] = cst - 0.5 * out["d2"]
    if not want_mu:
        out.pop("mu_T"), out.pop("mu_U")
    return out


# ------------------------------------------------------------------------------------ test data
# (1, 5, 3): fewer rows than the smallest group (two); (3, 5, 3), (37, 41, 37): a partial last group; (67, 131, 9):
# p beyond one lane sweep of 64 units in fp64, q narrower than a wave (and, at r = 9, q = r: no residual in Y);
# (33, 261, 130): p beyond one lane sweep in fp32, a second in fp64; (6, 2051, 3) and (6, 4101, 3): rows beyond
# 16 KB in fp64 and in fp32, where a wave owns four rows for k <= 8, with a partial group
SHAPES = [(1, 5, 3), (3, 5, 3), (37, 41, 37), (67, 131, 9), (33, 261, 130), (6, 2051, 3), (6, 4101, 3)]
RANKS = [1, 5, 8, 9, 16]
OUTPUTS = ("odx2", "ody2", "sd2", "d2", "loglik", "mu_T", "mu_U")


def cases():
    """Every (n, p, q, r) of SHAPES x RANKS with r <= min(p, q)."""
    return [(n, p, q, r) for (n, p, q) in SHAPES for r in RANKS if r <= min(p, q)]


def make_case(n, p, q, r, seed=0, sigE=0.3, sigF=0.4, sigH=0.2):
    """Rows drawn from the model at a theta with orthonormal W, C (a QR's Q, orthonormal to rounding only)."""
    rng = np.random.default_rng([seed, n, p, q, r])
    W = np.linalg.qr(rng.standard_normal((p, r)))[0]
    C = np.linalg.qr(rng.standard_normal((q, r)))[0]
    t = np.exp(-0.15 * np.arange(r)) * 1.4
    b = np.where(np.arange(r) % 2 == 0, 1.0, -1.0) * np.exp(np.log(1.3) - 0.2 * np.arange(r))
    T = rng.standard_normal((n, r)) * t
    Uu = T * b + sigH * rng.standard_normal((n, r))
    X = T @ W.T + sigE * rng.standard_normal((n, p))
    Y = Uu @ C.T + sigF * rng.standard_normal((n, q))
    th = dict(W=W, C=C, B=np.diag(b), sigE=sigE, sigF=sigF, sigH=sigH, sigT=np.diag(t))
    return X, Y, th


def theta_of(th):
    from ppls_amd import Theta
    return Theta(th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])


def planted(seed=20261020):
    """The planted-outlier data of the GPU test: n = 203, p = 37, q = 21, r = 3 drawn from the model at the
    true theta, then row 5 moved 12 sigE off the X plane, row 77 12 sigF off the Y plane and row 150
    8 sqrt(s11_1) along w_1.  Returns X, Y, theta (dict) and the planted rows by statistic."""
    n, p, q, r = 203, 37, 21, 3
    rng = np.random.default_rng(seed)
    b, t = np.array([1.3, 0.8, -0.5]), np.array([1.5, 1.0, 0.7])
    sE, sF, sH = 0.3, 0.4, 0.2
    W = np.linalg.qr(rng.standard_normal((p, r)))[0]
    C = np.linalg.qr(rng.standard_normal((q, r)))[0]
    T = rng.standard_normal((n, r)) * t
    Uu = T * b + sH * rng.standard_normal((n, r))
    X = T @ W.T + sE * rng.standard_normal((n, p))
    Y = Uu @ C.T + sF * rng.standard_normal((n, q))
    u = rng.standard_normal(p)
    u -= W @ (W.T @ u)
    u -= W @ (W.T @ u)
    v = rng.standard_normal(q)
    v -= C @ (C.T @ v)
    v -= C @ (C.T @ v)
    X[5] += 12 * sE * u / np.linalg.norm(u)
    Y[77] += 12 * sF * v / np.linalg.norm(v)
    X[150] += 8 * math.sqrt(t[0] ** 2 + sE ** 2) * W[:, 0]
    th = dict(W=W, C=C, B=np.diag(b), sigE=sE, sigF=sF, sigH=sH, sigT=np.diag(t))
    return X, Y, th, dict(odx2=5, ody2=77, sd2=150)
