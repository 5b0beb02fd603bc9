"""References, a-priori error bars and host models of the robust fit's device pieces, shared by
tests/test_robust_host.py and tests/test_gpu_robust.py.

Real-weighted Gram.  S_u = sum_i w_i d_i d_i' with real w_i >= 0: the count-weighted kernel's order
(tests/resample_bar.py: k-steps of 4 rows, the A operand of row i multiplied by w_i first, the split partials
added last) with a weight that is no integer.  Reference: long double from the weights as the device holds
them (fp64).  Bar: K_W gamma(n) outer(d, d), K_W = 2 -- one rounding for w x_a (exact for a count, a relative
u <= gamma(n) here), then the accumulation; ``resample_bar.inside`` serves as it stands.

Weights and sum log1p.  The kernel reads a row's odx2, ody2, sd2 and forms, per row,
    d2 = (odx2 / sE2 + ody2 / sF2) + sd2,   w = (nu + P) / (nu + d2),   t_j = log1p(d2 / nu_j).
``rowdiag_bar.bars`` bounds |delta d2| =: bd2.  Both w and t are smooth in d2 with slope 1 / (nu + d2) (times w
for the weight), and nu + d2 - bd2 bounds the denominator anywhere between the two values:
    bar(w)   = w [bd2 / (nu + d2 - bd2) + gamma(K_WT)]            K_WT = 4: nu + P, nu + d2, the division, a spare
    bar(t_j) = bd2 / (nu_j + d2 - bd2) + gamma(K_LOG) t_j          K_LOG = 6: the division (u x / (1 + x) <= u t),
                                                                  log1p itself within a few ulps, a spare
The sum adds a thread's PPLS_ROBUST_BLOCK / 256 rows, the 6 + 2 levels of the workgroup tree, then the block
partials ceil(blocks / 256) to a thread and the same tree: DEPTH(n) additions behind any term,
    bar(sum_j) = sum_i bar(t_ij) + gamma(DEPTH(n)) sum_i t_ij     (+ gamma(ranks) of the sum when sharded).

l_t = N c(nu) - (N / 2) logdet - ((nu + P) / 2) sum_j with c = lgamma((nu + P) / 2) - lgamma(nu / 2) -
(P / 2) log(nu pi), the constants formed on the host in fp64 (the reference takes the same lgamma: K_LG = 8
ulps of each cover both evaluations), logdet as rowdiag_bar's log constant (K_CST, K_FORM):
    bar(l_t) = ((nu + P) / 2) bar(sum_j) + N gamma(K_LG) |c|_abs + (N / 2) (gamma(K_CST) |logdet|_abs + gamma(K_FORM) (p + q))
               + gamma(K_LL) (N |c|_abs + (N / 2) |logdet|_abs + ((nu + P) / 2) sum_j).
"""
import math

import numpy as np

import rowdiag_bar as rb
from resample_bar import K_W, inside as gram_inside, kernel_order, weighted_ref  # noqa: F401  (re-exported)
from rowdiag_bar import L, U, gamma

BLOCK = 1024       # PPLS_ROBUST_BLOCK
K_WT = 4
K_LOG = 6
K_LG = 8
K_LL = 6           # the three products and two differences of l_t, a spare


def depth(n, ranks=1):
    blocks = max(-(-n // BLOCK), 1)
    return BLOCK // 256 + 8 + -(-blocks // 256) + 8 + (ranks if ranks > 1 else 0)


def draw_weights(n, P, nu, seed):
    """n weights (nu + P) / (nu + chi2_P), the E-step weights of rows that follow the model."""
    rng = np.random.default_rng([seed, n, P])
    return (nu + P) / (nu + rng.chisquare(P, n))


# ------------------------------------------------------------------------------------ references
def logdet_parts(th, p, q, dtype=L):
    """(logdet, |logdet|_abs) with logdet = (p - r) log sE2 + (q - r) log sF2 + sum_k log det_k."""
    _, _, _, det, sE2, sF2 = rb.forms(th, dtype)
    r = det.shape[0]
    ld = np.log(det)
    terms = [dtype(p - r) * np.log(sE2), dtype(q - r) * np.log(sF2)]
    return terms[0] + terms[1] + ld.sum(), float(abs(terms[0]) + abs(terms[1]) + np.abs(ld).sum())


def t_constant(nu, P):
    """(c, |c|_abs) of one row's normalising constant, fp64 as the library forms it."""
    a, b, c = math.lgamma(0.5 * (nu + P)), math.lgamma(0.5 * nu), 0.5 * P * math.log(nu * math.pi)
    return a - b - c, abs(a) + abs(b) + abs(c)


def reference(X, Y, th, nus, keep=0, f32=False, N=None):
    """d2, w (for nus[keep]), sums (per nu) and loglik_t (per nu) in long double; N: the rows of all ranks."""
    p, q = X.shape[1], Y.shape[1]
    P = p + q
    d2 = rb.reference(X, Y, th, f32)["d2"]
    nus = [float(v) for v in np.atleast_1d(nus)]
    w = (L(nus[keep]) + L(P)) / (L(nus[keep]) + d2)
    sums = np.array([np.log1p(d2 / L(v)).sum() for v in nus], dtype=L)
    N = X.shape[0] if N is None else N
    logdet, _ = logdet_parts(th, p, q, L)
    ll = np.array([L(N) * L(t_constant(v, P)[0]) - L(N) / 2 * logdet - (L(v) + L(P)) / 2 * s for v, s in zip(nus, sums)], dtype=L)
    return dict(d2=d2, w=w, sums=sums, loglik_t=ll)


def bars(X, Y, th, nus, keep=0, f32=False, N=None, ranks=1):
    """The a-priori bars of w, sums and loglik_t as float64 (module docstring)."""
    p, q = X.shape[1], Y.shape[1]
    P, n = p + q, X.shape[0]
    N = n if N is None else N
    nus = [float(v) for v in np.atleast_1d(nus)]
    bd2 = rb.bars(X, Y, th, f32)["d2"]
    d2 = np.asarray(rb.reference(X, Y, th, f32)["d2"], dtype=np.float64)
    assert np.all(bd2 < min(nus) + d2)
    nk = nus[keep]
    w = (nk + P) / (nk + d2)
    bw = w * (bd2 / (nk + d2 - bd2) + gamma(K_WT))
    _, ldabs = logdet_parts(th, p, q, L)
    bs, bl = [], []
    for v in nus:
        t = np.log1p(d2 / v)
        b = float((bd2 / (v + d2 - bd2) + gamma(K_LOG) * t).sum() + gamma(depth(n, ranks)) * t.sum())
        bs.append(b)
        cabs = t_constant(v, P)[1]
        bl.append(0.5 * (v + P) * b + N * gamma(K_LG) * cabs + 0.5 * N * (gamma(rb.K_CST) * ldabs + gamma(rb.K_FORM) * P) +
                  gamma(K_LL) * (N * cabs + 0.5 * N * ldabs + 0.5 * (v + P) * float(t.sum())))
    return dict(w=bw, sums=np.array(bs), loglik_t=np.array(bl))


def inside(val, ref, bar):
    return rb.inside(val, ref, bar)


# ------------------------------------------------------------------------------------ host model
def _group_sum(v):
    """The 256 thread values along the last axis: lanes by the xor tree, then the waves as (0 + 1) + (2 + 3)."""
    w = rb._tree(v.reshape(v.shape[:-1] + (4, 64)), 64)
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def model_sum(t):
    """sum of the n row terms t in the kernel's order, plain fp64."""
    n = t.shape[0]
    blocks = max(-(-n // BLOCK), 1)
    tp = np.zeros(blocks * BLOCK)
    tp[:n] = t
    tb = tp.reshape(blocks, BLOCK // 256, 256)
    acc = np.zeros((blocks, 256))
    for k in range(BLOCK // 256):
        acc = acc + tb[:, k, :]
    part = _group_sum(acc)                        # one partial per block
    per = -(-blocks // 256)
    pp = np.zeros(per * 256)
    pp[:blocks] = part
    acc = np.zeros(256)
    for k in range(per):
        acc = acc + pp[k * 256:(k + 1) * 256]
    return float(_group_sum(acc))


def host_model(odx2, ody2, sd2, th, nus, keep, P, defect=None):
    """d2, w, sums from a plain fp64 evaluation in the kernel's order; defect: None or "log" (log of d2 / nu
    in place of log1p)."""
    *_, sE2, sF2 = rb.forms(th, np.float64)
    d2 = (odx2 / sE2 + ody2 / sF2) + sd2
    nus = [float(v) for v in np.atleast_1d(nus)]
    w = (nus[keep] + P) / (nus[keep] + d2)
    f = np.log if defect == "log" else np.log1p
    sums = np.array([model_sum(f(d2 / v)) for v in nus])
    return dict(d2=d2, w=w, sums=sums, sum_w=model_sum(w))


def loglik_t_from(sums, th, nus, p, q, N):
    """l_t per nu from the row sums, fp64, as the library's host code forms it."""
    P = p + q
    logdet = float(logdet_parts(th, p, q, np.float64)[0])
    return np.array([(N * t_constant(float(v), P)[0] - 0.5 * N * logdet) - 0.5 * (float(v) + P) * s
                     for v, s in zip(np.atleast_1d(nus), sums)])


# ------------------------------------------------------------------------------------ the loop, from the oracle
def dense_d2_logdet(X, Y, th):
    """Every row's d2 = d' Sigma^-1 d and log det Sigma on the oracle's dense covariance (sse_xy_w)."""
    from oracle import ppls_oracle as o
    W, C, b, t, sE, sF, sH = rb.theta_parts(th)
    Sig = o.sse_xy_w(W, C, np.diag(b), sE, sF, sH, np.diag(t))
    D = np.hstack([X, Y])
    d2 = np.einsum("ij,ij->i", D, np.linalg.solve(Sig, D.T).T)
    sign, logdet = np.linalg.slogdet(Sig)
    assert sign > 0
    return d2, float(logdet)


def dense_loglik_t(X, Y, th, nu):
    """l_t written out on the dense covariance: scipy's multivariate_t when it is there, the formula otherwise."""
    D = np.hstack([X, Y])
    try:
        from scipy.stats import multivariate_t
        from oracle import ppls_oracle as o
        W, C, b, t, sE, sF, sH = rb.theta_parts(th)
        Sig = o.sse_xy_w(W, C, np.diag(b), sE, sF, sH, np.diag(t))
        return float(multivariate_t(loc=np.zeros(D.shape[1]), shape=Sig, df=nu).logpdf(D).sum())
    except ImportError:
        d2, logdet = dense_d2_logdet(X, Y, th)
        N, P = D.shape
        return float(N * t_constant(nu, P)[0] - 0.5 * N * logdet - 0.5 * (nu + P) * np.log1p(d2 / nu).sum())


def nu_grid(lo, hi, m=16):
    return np.exp(np.linspace(math.log(lo), math.log(hi), m))


def best_nu(d2, logdet, N, P, lo=1.0, hi=1000.0, rounds=4, m=16):
    """The nu in [lo, hi] that maximises l_t at fixed d2: ``rounds`` rounds of an m-point log-spaced grid, each
    bracketing the previous best point.  Returns (nu, l_t(nu), the last grid's ratio of neighbouring points)."""
    def lt(v):
        return N * t_constant(v, P)[0] - 0.5 * N * logdet - 0.5 * (v + P) * np.log1p(d2 / v).sum()
    for _ in range(rounds):
        g = nu_grid(lo, hi, m)
        v = [lt(x) for x in g]
        k = int(np.argmax(v))
        lo, hi = max(1.0, g[max(k - 1, 0)]), min(1000.0, g[min(k + 1, m - 1)])
    return float(g[k]), float(v[k]), float(g[1] / g[0])


def em_steps(X, Y, th, steps):
    from oracle import ppls_oracle as o
    for _ in range(steps):
        f = o.expect_m(X, Y, th["W"], th["C"], th["B"], th["sigE"], th["sigF"], th["sigH"], th["sigT"])
        th = o.maximiz_m(f, X, Y)
    return th


def oracle_loop(X, Y, th, nu=4.0, outer=50, inner=5, atol=1e-4, divisor="N"):
    """robust_PPLS_simult written out with the oracle's Expect_M and Maximiz_M on rows scaled by sqrt(u), N kept
    as the row count.  divisor="sum_u": the defect that divides S_u by sum u (the rows rescaled by
    sqrt(N / sum u) on top).  Returns dict(theta, loglik, nu, weights, d2, steps, converged)."""
    N, P = X.shape[0], X.shape[1] + Y.shape[1]
    estimate = nu == "estimate"
    ll, steps, converged = [], 0, False
    while True:
        d2, logdet = dense_d2_logdet(X, Y, th)
        if estimate:
            nu_k, l, _ = best_nu(d2, logdet, N, P)
        else:
            nu_k = float(nu)
            l = float(N * t_constant(nu_k, P)[0] - 0.5 * N * logdet - 0.5 * (nu_k + P) * np.log1p(d2 / nu_k).sum())
        u = (nu_k + P) / (nu_k + d2)
        ll.append(l)
        if len(ll) > 1 and ll[-1] - ll[-2] < atol:
            converged = True
            break
        if steps >= outer:
            break
        s = np.sqrt(u * (N / u.sum() if divisor == "sum_u" else 1.0))[:, None]
        th = em_steps(X * s, Y * s, th, inner)
        steps += 1
    return dict(theta=th, loglik=np.array(ll), nu=nu_k, weights=u, d2=d2, steps=steps, converged=converged)


def contaminated(seed, n=300, p=12, q=9, r=2, nout=12, scale=4.0):
    """make_problem(n, p, q, r, seed) with nout rows replaced by scale N(0, 1): X, Y, theta0 and the true W, C."""
    from conftest import make_problem
    X, Y, th0 = make_problem(n, p, q, r, seed)
    rng = np.random.default_rng(seed)            # make_problem's first two draws are the true loadings

    def polar(M):
        Uu, _, Vt = np.linalg.svd(M, full_matrices=False)
        return Uu @ Vt

    Wt, Ct = polar(rng.standard_normal((p, r))), polar(rng.standard_normal((q, r)))
    rng = np.random.default_rng(seed + 99)
    idx = rng.choice(n, nout, replace=False)
    X, Y = X.copy(), Y.copy()
    X[idx] = scale * rng.standard_normal((nout, p))
    Y[idx] = scale * rng.standard_normal((nout, q))
    return X, Y, th0, Wt, Ct


def t_mixed(seed, n=2000, p=12, q=9, r=2, df=5.0):
    """make_problem's rows, each scaled by sqrt(df / chi2_df): multivariate t_df about the model."""
    from conftest import make_problem
    X, Y, th0 = make_problem(n, p, q, r, seed)
    s = np.sqrt(df / np.random.default_rng(seed + 99).chisquare(df, n))[:, None]
    return X * s, Y * s, th0


def space_error(A, B):
    """||A A' - B B'||_F: 0 for equal column spaces, sqrt(2 r) for orthogonal ones."""
    return float(np.linalg.norm(A @ A.T - B @ B.T))
