"""Reference, error bar and a host model of the permuted cross block, shared by
tests/test_permute_host.py and tests/test_gpu_permute.py.

The kernel forms C_pi = sum_i x_i y_pi(i)' (p x q) over the rows as the context stores them: per item (row
split x 64 x 64 quadrant) the rows go through v_mfma_f64_16x16x4_f64 four at a time, X's row i against Y's
row perm[i], and the split partials are added last, in split order.

Reference: C_ref = sum_i x_i y_perm[i]' in long double (for fp32 storage over the rows rounded to fp32).

Bar: K_P gamma(n + nsplit) outer(dx, dy), dx_a = sqrt(sum_i x_ia^2), dy_b = sqrt(sum_i y_ib^2) (a
permutation leaves dy as it is), counted the way tests/test_stream_host.py counts K_STAGES: the products
are fused, so the only roundings are the additions, at most n - 1 + nsplit - 1 behind any term -- one
stage, gamma(n + nsplit) of the absolute sum sum_i |x_ia| |y_perm[i]b|, which Cauchy-Schwarz bounds by
dx_a dy_b.  K_P = 1; one more stage where a cross-rank sum follows (K_P_SHARDED).
"""
import numpy as np

from test_stream_host import L, gamma

K_P = 1
K_P_SHARDED = K_P + 1
AUTO_SPLITS = 64   # nsplit = 0 (auto): the plan makes at most this many splits ...
AUTO_MIN_ROWS = 256   # ... none of them under this many rows, so fewer than 512 rows stay in one split


def splits_of(n, nsplit):
    """The split count the bar takes for a requested one (0 = auto: what the plan can make at most)."""
    if nsplit > 0:
        return nsplit
    return 1 if n < 2 * AUTO_MIN_ROWS else AUTO_SPLITS


def permuted_ref(X, Y, perm):
    """C_ref = sum_i x_i y_perm[i]' in long double."""
    X = np.asarray(X, dtype=np.float64).astype(L)
    Y = np.asarray(Y, dtype=np.float64).astype(L)
    return X.T @ Y[np.asarray(perm, dtype=np.int64)]


def permuted_bar(X, Y, n, nsplit=1, k=K_P):
    """k gamma(n + nsplit) outer(dx, dy) as float64 (nsplit 0, auto: splits_of)."""
    dx = np.sqrt((np.asarray(X, dtype=np.float64).astype(L) ** 2).sum(axis=0))
    dy = np.sqrt((np.asarray(Y, dtype=np.float64).astype(L) ** 2).sum(axis=0))
    return np.asarray(k * gamma(max(int(n), 1) + splits_of(n, nsplit)) * np.outer(dx, dy), dtype=np.float64)


def split_bounds(n, nsplit):
    """The equal row splits the kernel plans for a requested split count."""
    return [n * s // nsplit for s in range(nsplit + 1)]


def kernel_order(X, Y, perm, nsplit=1):
    """A plain fp64 evaluation in the kernel's order: per split, k-steps of 4 rows, each row's term
    x_i y_perm[i]' added in row order; the split partials added last, in split order."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    perm = np.asarray(perm, dtype=np.int64)
    parts = []
    b = split_bounds(X.shape[0], nsplit)
    for r0, r1 in zip(b[:-1], b[1:]):
        acc = np.zeros((X.shape[1], Y.shape[1]))
        for k0 in range(r0, r1, 4):
            for i in range(k0, min(k0 + 4, r1)):
                acc = acc + np.outer(X[i], Y[perm[i]])
        parts.append(acc)
    C = np.zeros((X.shape[1], Y.shape[1]))
    for part in parts:
        C = C + part
    return C


def inside(C, C_ref, bar):
    """Whether C lies within the bar of C_ref, and the largest error in units of the bar."""
    err = np.asarray(np.abs(np.asarray(C, dtype=np.float64).astype(L) - C_ref), dtype=np.float64)   # (in long double)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    return bool(np.all(err <= bar)), float(ratio.max())


def permutations(n, seed):
    """The identity, the reversal, the cyclic shift by 1 and a seeded random permutation of n rows -- for
    n >= 3 the first draw that is not its own inverse (an involution cannot tell perm from its inverse)."""
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    rnd = rng.permutation(n).astype(np.int64)
    while n >= 3 and np.array_equal(rnd[rnd], i):
        rnd = rng.permutation(n).astype(np.int64)
    return dict(identity=i, reversal=i[::-1].copy(), shift=np.roll(i, -1), random=rnd)
