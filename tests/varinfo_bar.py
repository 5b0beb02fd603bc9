"""Reference, a-priori error bar and a host model of ppls_varinfo_batched, shared by
tests/test_varinfo_bar_host.py and tests/test_gpu_variances_xprod.py.

For component i and the p x p block g of S the kernel forms, every operation rounded once (no
contraction), in this order:

    sse[a][b] = (((ctt g[a][b] - (x_a k1) w_b) - (w_a k1) x_b) + (w_a k2) w_b) / s4 / N
    J[a][b]   = sse[a][b] - delta_ab bstar
    star[a][b] = ((x_a - w_a ctt) (x_b - w_b ctt)) / s4

Reference: the same expressions in long double from the same fp64 inputs (s4 = (sigE sigE)(sigE sigE)
is one of them: the entry point forms it in fp64 and so does ``make_case``).

Bar for J: gamma(8) ((|ctt g| + k1 |x_a w_b| + k1 |w_a x_b| + |k2 w_a w_b|) / s4 / N + delta_ab bstar).
The count is the largest number of roundings any term passes through.  The first cross term has all
eight: 2 in its products, the 3 additions (it enters the first), the 2 divisions and the diagonal
subtraction.  The others have fewer (ctt g: 1 product; the last term: 1 addition; bstar: the subtraction
only), so K_J = 8 cannot be tightened for this order and is what the issue states.  SSt_exp is J without
the last step: K_EXP = 7 and no bstar term.

Bar for SSt_star: each factor f_a = x_a - w_a ctt comes out as f_a + e_a with |e_a| <= 2u F_a,
F_a = |x_a| + |w_a ctt| (the product's and the subtraction's roundings); the product of the two factors
is then off by at most 4u F_a F_b (+ O(u^2)), and its own rounding and the division add one each:
K_STAR = 7 covers 6u plus the second-order terms, on F_a F_b / s4.
"""
import numpy as np

L = np.longdouble
U = 2.0 ** -53
K_J, K_EXP, K_STAR = 8, 7, 7


def gamma(k):
    return k * U / (1.0 - k * U)


def make_case(p, off, a, seed=0, nan_outside=True):
    """A block of cross-products inside a P x P matrix (P = off + p, + 1 for odd p) whose every other
    entry is NaN, a components' Cxt and w, and scalars of the sizes variances.PPLS_simult meets."""
    rng = np.random.default_rng(1000 * p + 10 * off + a + seed)
    P = off + p + (p & 1)
    n = 40
    D = rng.standard_normal((n, p)) * (0.5 + np.arange(p) % 5)
    g = D.T @ D
    g = np.tril(g) + np.tril(g, -1).T
    S = np.full((P, P), np.nan if nan_outside else 0.0)
    S[off:off + p, off:off + p] = g
    w = np.linalg.qr(rng.standard_normal((p, a)))[0] if p >= a else rng.standard_normal((p, a))
    cxt = w * rng.uniform(20.0, 40.0, a) + rng.standard_normal((p, a))
    N = float(n)
    sigE = 0.7
    ctt = N * rng.uniform(0.3, 1.2, a)
    mu2 = ctt * rng.uniform(0.3, 0.9, a)
    Vt = ctt - mu2
    s2 = sigE * sigE
    return dict(S=S, P=P, off=off, p=p, a=a, g=g, cxt=np.asfortranarray(cxt), w=np.asfortranarray(w), ctt=ctt,
                k1=ctt + 2.0 * Vt, k2=ctt * ctt + 4.0 * mu2 * Vt + 2.0 * Vt * Vt, bstar=ctt / s2 / N, sigE=sigE,
                s4=s2 * s2, N=N)


def _terms(c, i, T):
    """(ctt g, x_a k1 w_b, w_a k1 x_b, w_a k2 w_b) of component i in number type T."""
    g = c["g"].astype(T)
    x, w = c["cxt"][:, i].astype(T), c["w"][:, i].astype(T)
    ctt, k1, k2 = T(c["ctt"][i]), T(c["k1"][i]), T(c["k2"][i])
    return ctt * g, (x * k1)[:, None] * w[None, :], (w * k1)[:, None] * x[None, :], (w * k2)[:, None] * w[None, :]


def reference(c):
    """(J, sse, star) in long double, a x p x p each, entry [i, a, b]."""
    p, s4, N = c["p"], L(c["s4"]), L(c["N"])
    J, E, S = [], [], []
    for i in range(c["a"]):
        t1, t2, t3, t4 = _terms(c, i, L)
        sse = (t1 - t2 - t3 + t4) / s4 / N
        f = c["cxt"][:, i].astype(L) - c["w"][:, i].astype(L) * L(c["ctt"][i])
        E.append(sse)
        J.append(sse - np.eye(p, dtype=L) * L(c["bstar"][i]))
        S.append(f[:, None] * f[None, :] / s4)
    return np.stack(J), np.stack(E), np.stack(S)


def bars(c):
    """The a-priori bars of (J, sse, star), fp64, same shapes as ``reference``."""
    p, s4, N = c["p"], c["s4"], c["N"]
    bj, be, bs = [], [], []
    for i in range(c["a"]):
        mag = sum(np.abs(t) for t in _terms(c, i, np.float64)) / s4 / N
        F = np.abs(c["cxt"][:, i]) + np.abs(c["w"][:, i] * c["ctt"][i])
        bj.append(gamma(K_J) * (mag + np.eye(p) * c["bstar"][i]))
        be.append(gamma(K_EXP) * mag)
        bs.append(gamma(K_STAR) * F[:, None] * F[None, :] / s4)
    return np.stack(bj), np.stack(be), np.stack(bs)


def kernel_order(c, defect=None):
    """J in plain fp64 in the kernel's order (numpy's elementwise operations round once each), lower
    triangle computed and mirrored as the kernel does.  defect: "one_k1" (k1 on one of the two cross
    terms only), "transposed" (x and w indexed transposed in one term), "diag_sign" (the diagonal term
    added instead of subtracted)."""
    p, s4, N = c["p"], c["s4"], c["N"]
    out = []
    for i in range(c["a"]):
        x, w = c["cxt"][:, i], c["w"][:, i]
        ctt, k1, k2 = c["ctt"][i], c["k1"][i], c["k2"][i]
        t1 = ctt * c["g"]
        t2 = (x * k1)[:, None] * w[None, :]
        t3 = (w * k1)[:, None] * x[None, :]
        if defect == "one_k1":
            t3 = w[:, None] * x[None, :]
        if defect == "transposed":
            t2 = (x * k1)[None, :] * w[:, None]
        t4 = (w * k2)[:, None] * w[None, :]
        sse = (((t1 - t2) - t3) + t4) / s4 / N
        sse = np.tril(sse) + np.tril(sse, -1).T
        d = np.eye(p) * c["bstar"][i]
        out.append(sse + d if defect == "diag_sign" else sse - d)
    return np.stack(out)


def inside(got, ref, bar):
    """Whether got lies within bar of ref (the difference taken in long double), and the largest error
    as a share of the bar."""
    err = np.asarray(np.abs(np.asarray(got, dtype=np.float64).astype(L) - ref), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return bool(np.all(err <= bar)), float(np.nanmax(ratio)) if ratio.size else 0.0
