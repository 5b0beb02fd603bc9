"""Host side of the streamed-data path: the pairwise-merge algebra restated in numpy,
the error bars the GPU tests use, and the argument checks of ``stream_data`` that need no device.

The device forms S = Z'Z of Z = scale([X Y], center, scale) from row chunks: per chunk c (n_c rows,
mean m_c, Gram G_c of the chunk centred about m_c), with N rows and mean m merged so far,

    S += G_c + (N n_c / (N + n_c)) d d',  d = m_c - m;   m += d n_c / (N + n_c);   N += n_c

(Chan, Golub & LeVeque's pairwise update), then S_ij / (d_i d_j) with d_j = sqrt(S_jj / (N - 1)).
The one-pass alternative S_raw - N m m' cancels (mean / sd)^2 of its digits; the pairwise form loses
only about u |mean| / sd, through d.  ``merge_stream`` below is that algebra in fp64, which pins the
bar of tests/test_gpu_stream.py::test_ill_conditioned independently of the device code.
"""
import numpy as np
import pytest

U = 2.0 ** -53
L = np.longdouble
CHUNKS = [1, 63, 64, 65]      # then the rest: a one-row chunk, and 64 +- 1 rows


def gamma(n):
    return n * U / (1.0 - n * U)


# Rounding stages of the streamed S, each bounded entrywise by gamma_n sqrt(S_jj S_ll) for data whose
# column means are within a few sd of zero: the chunk Grams (1, by Cauchy-Schwarz over the chunks),
# the merge's additions (at most 2 per chunk: split partials and the rank-1 term; 2), chunk mean and
# centring (a relative perturbation of <= gamma_{n_c} + u of each entry; 2, for the two factors), the
# rank-1 term itself (1) and standardise (sqrt, product, division: 1): 7 on one context.  Sharded
# streams add the cross-rank merge (1).
K_STAGES = 7
K_SHARDED = K_STAGES + 1


def split_rows(n, sizes=CHUNKS):
    """Row boundaries of the chunks ``sizes`` followed by the rest."""
    b = [0]
    for s in sizes:
        if b[-1] + s < n:
            b.append(b[-1] + s)
    b.append(n)
    return b


def scale_ref(x, center, scale):
    """R's scale(x, center, scale), two passes, in long double: (z, centre, scale)."""
    x = np.asarray(x, dtype=np.float64).astype(L)
    n = x.shape[0]
    cen = x.sum(axis=0) / L(n) if center else np.zeros(x.shape[1], dtype=L)
    xc = x - cen
    sd = np.sqrt((xc * xc).sum(axis=0) / L(max(1, n - 1))) if scale else np.ones(x.shape[1], dtype=L)
    return xc / sd, cen, sd


def s_ref(X, Y, center, scale):
    """(S, centre, scale) of the joint [X Y]: R's two-pass scale(), then the Gram, in long double."""
    z, cen, sd = scale_ref(np.hstack([X, Y]), center, scale)
    return z.T @ z, cen, sd


def gram_bar(S, n, k=K_STAGES):
    d = np.sqrt(np.abs(np.diag(np.asarray(S, dtype=np.float64))))
    return k * gamma(n) * np.outer(d, d)


def ill_conditioned(seed=3):
    """n = 300, P = 21: X columns 1e6 + N(0, 1), Y columns 2e5 + 3 N(0, 1), one column 5 + 1e-3 N(0, 1)."""
    rng = np.random.default_rng(seed)
    X = 1e6 + rng.standard_normal((300, 12))
    Y = 2e5 + 3.0 * rng.standard_normal((300, 9))
    Y[:, 4] = 5.0 + 1e-3 * rng.standard_normal(300)
    return X, Y


def ill_bar(X, Y):
    D = np.hstack([X, Y])
    return 64 * U * np.max(np.abs(D.mean(axis=0)) / D.std(axis=0, ddof=1))


def merge_stream(D, bounds, center=True):
    """The pairwise merge over the chunks D[bounds[i]:bounds[i+1]] in fp64: (S, mean, N)."""
    P = D.shape[1]
    S, m, N = np.zeros((P, P)), np.zeros(P), 0.0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        c = D[lo:hi]
        nc = float(hi - lo)
        if center:
            mc = c.sum(axis=0) / nc
            c = c - mc
            d = mc - m
            S = S + c.T @ c + (N * nc / (N + nc)) * np.outer(d, d)
            m = m + d * (nc / (N + nc))
        else:
            S = S + c.T @ c
        N += nc
    return S, m, N


def standardise(S, N):
    d = np.sqrt(np.diag(S) / (N - 1.0))
    return S / np.outer(d, d), d


def test_pairwise_merge_meets_the_bar_and_one_pass_does_not():
    X, Y = ill_conditioned()
    D = np.hstack([X, Y])
    n = D.shape[0]
    ref, cen, sd = s_ref(X, Y, True, True)
    ref = np.asarray(ref / L(n - 1), dtype=np.float64)
    bar = ill_bar(X, Y)
    assert 1e-9 < bar < 1e-7                                  # ~64 u 1e6
    # two passes in fp64
    z = (D - D.mean(axis=0)) / D.std(axis=0, ddof=1)
    two = np.abs(z.T @ z / (n - 1) - ref).max()
    # the pairwise merge over [1, 63, 64, 65, 107]
    S, m, N = merge_stream(D, split_rows(n))
    Sz, d = standardise(S, N)
    pair = np.abs(Sz / (n - 1) - ref).max()
    # one pass: S_raw - N m m'
    m1 = D.sum(axis=0) / n
    S1 = D.T @ D - n * np.outer(m1, m1)
    with np.errstate(invalid="ignore", divide="ignore"):
        S1z, _ = standardise(S1, float(n))
        one = np.nanmax(np.abs(S1z / (n - 1) - ref)) if np.isfinite(S1z).any() else np.inf
    print(f"two-pass {two:.3g}, pairwise {pair:.3g}, one-pass {one:.3g}, bar {bar:.3g}")
    assert N == n
    assert two < 1e-13
    assert pair < bar
    assert not (one < bar)                                    # fails it by orders of magnitude
    assert one > 1e3 * bar
    assert np.abs(m - np.asarray(cen, dtype=np.float64)).max() <= 4 * U * np.abs(m).max()
    assert np.abs(d / np.asarray(sd, dtype=np.float64) - 1).max() < bar


@pytest.mark.parametrize("center", [True, False])
def test_merge_is_chunking_invariant_within_the_gram_bar(center):
    rng = np.random.default_rng(5)
    D = rng.standard_normal((257, 11)) * (0.5 + np.arange(11) % 3) + 0.3
    ref, _, _ = s_ref(D[:, :6], D[:, 6:], center, False)
    ref = np.asarray(ref, dtype=np.float64)
    bar = gram_bar(ref, 257)
    for bounds in ([0, 257], split_rows(257), list(range(0, 257, 64)) + [257], [0, 1, 2, 3, 4, 5, 257]):
        S, _, N = merge_stream(D, bounds, center)
        assert N == 257
        assert np.all(np.abs(S - ref) <= bar)


def test_split_rows():
    assert split_rows(300) == [0, 1, 64, 128, 193, 300]
    assert split_rows(2) == [0, 1, 2]
    assert split_rows(1) == [0, 1]


# ------------------------------------------------------------------------------ stream_data's arguments
def test_stream_data_argument_checks_need_no_device():
    from ppls_amd import stream_data
    X, Y = np.zeros((4, 3)), np.zeros((4, 2))
    with pytest.raises(ValueError, match="empty"):
        stream_data([])
    with pytest.raises(TypeError, match="iterable"):
        stream_data(X)
    with pytest.raises(TypeError, match="iterable"):
        stream_data(5)
    with pytest.raises(TypeError, match="pair"):
        stream_data([X])
    with pytest.raises(TypeError, match="pair"):
        stream_data([(X, Y, X)])
    with pytest.raises(ValueError, match="same number of rows"):
        stream_data([(X, Y[:3])])
    with pytest.raises(ValueError, match="same number of rows"):
        stream_data(iter([(X[0], Y[0])]))
