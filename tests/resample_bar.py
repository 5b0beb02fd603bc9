"""Reference, error bar and a host model of the weighted MFMA Gram, shared by
tests/test_resample_host.py and tests/test_gpu_resample.py.

The kernel forms S_c = sum_i c_i d_i d_i' over the rows d_i of D with integer counts c_i >= 0: per item
(row split x 64 x 64 quadrant) the rows go through v_mfma_f64_16x16x4_f64 four at a time, the A operand
of row i multiplied by (double) c_i first, and the split partials are added last, in split order.

Reference: S_ref = sum_i c_i d_i d_i' in long double.

Bar: K_W gamma(n) outer(d, d), d = sqrt(diag(S_ref)), n the rows, counted the way
tests/test_stream_host.py counts K_STAGES:
  * the product c x_a: one rounding per term, a relative perturbation u <= gamma(n) of a sum whose
    absolute terms add to sum_i c_i |x_ia| |x_ib|                                              (1)
  * the MFMA accumulation with the split sums: at most n - 1 + nsplit - 1 additions behind any term (the
    products themselves are fused), gamma(n) of the same absolute sum for nsplit <= n + 1         (1)
and Cauchy-Schwarz bounds sum_i c_i |x_ia| |x_ib| = sum_i (sqrt(c_i) |x_ia|)(sqrt(c_i) |x_ib|) by d_a d_b.
K_W = 2; one more stage where a cross-rank sum follows (K_W_SHARDED).  The unweighted Gram of the
repeated rows (N' = sum c rows) has the second stage only: gamma(N') outer(d, d).
"""
import numpy as np

from test_stream_host import L, gamma, gram_bar

K_W = 2
K_W_SHARDED = K_W + 1
COUNT_POOL = (0, 0, 1, 1, 2, 7)


def draw_counts(n, seed):
    """n counts from COUNT_POOL, at least one of them positive."""
    rng = np.random.default_rng(seed)
    c = rng.choice(COUNT_POOL, size=n).astype(np.int32)
    if not c.any():
        c[rng.integers(n)] = 2
    return c


def weighted_ref(D, c):
    """S_ref = sum_i c_i d_i d_i' in long double."""
    D = np.asarray(D, dtype=np.float64).astype(L)
    w = np.asarray(c).astype(L)
    return (D * w[:, None]).T @ D


def weighted_bar(S_ref, n, k=K_W):
    return gram_bar(S_ref, max(int(n), 1), k)


def split_bounds(n, nsplit):
    """The equal row splits the Gram plans for a requested split count."""
    return [n * s // nsplit for s in range(nsplit + 1)]


def kernel_order(D, c, nsplit=1, both=False):
    """A plain fp64 evaluation in the kernel's order: per split, k-steps of 4 rows, each row's term
    (c x_a) x_b added in row order; the split partials added last.  both: the defect that weights
    both operands."""
    D = np.asarray(D, dtype=np.float64)
    w = np.asarray(c, dtype=np.float64)
    P = D.shape[1]
    parts = []
    b = split_bounds(D.shape[0], nsplit)
    for r0, r1 in zip(b[:-1], b[1:]):
        acc = np.zeros((P, P))
        for k0 in range(r0, r1, 4):
            for i in range(k0, min(k0 + 4, r1)):
                a = D[i] * w[i]
                acc = acc + np.outer(a, a if both else D[i])
        parts.append(acc)
    G = np.zeros((P, P))
    for part in parts:
        G = G + part
    return G


def inside(G, S_ref, n, k=K_W):
    """Whether G lies within the bar of S_ref, and the largest error in units of the bar."""
    bar = weighted_bar(S_ref, n, k)
    err = np.asarray(np.abs(np.asarray(G, dtype=np.float64).astype(L) - S_ref), dtype=np.float64)   # (in long double)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return bool(np.all(err <= bar)), float(ratio.max())
