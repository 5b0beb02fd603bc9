"""Host side of cross-validation on streamed data: no GPU.

The algebra restated in numpy and checked against a long-double two-pass reference, the error bars the
GPU tests use, the argument errors raised before any device call, and the entry points in the header
and the ctypes table.

A stream opened with K folds keeps one Chan state (N_k, mean_k, S_k) per fold.  At the end, with
N = sum N_k and m = sum N_k mean_k / N (fold order),

    S_k <- (S_k + N_k (mean_k - m)(mean_k - m)') / (d d'),   d_j = sqrt(sum_k S_k,jj / (N - 1)),

the training cross-products of fold k are sum_{l != k} S_l (by addition), and the held-out error of a
fit (W, B, C) on fold k is, with A = W' S_k,xx W, D_m = w_m' S_k,xy c_m, G = C'C,

    sse_j = tr(S_k,yy) - 2 sum_{m<=j} b_m D_m + sum_{m,l<=j} b_m b_l A_ml G_ml.

Error bars.  The rounding stages of a fold matrix, each bounded entrywise by gamma_n sqrt(S_jj S_ll)
with n the fold's rows: the 7 of the plain stream (test_stream_host.K_STAGES), the recentring term
N_k e e' (1) and its addition (1): K_FOLD = 9; a sharded stream adds the cross-rank merge (1).  A
selection adds the fold-order sum, K - 1 <= n additions (1 stage of gamma_n by Cauchy-Schwarz over the
folds): K_SELECT = 10 over the selected rows.

The quadratic form: every elementary product s_ij w_im w_jl c_.m c_.l b_m b_l of the expansion passes
through at most 2p + q + k^2 + 8 roundings on its way into sse_j (two sums over p, one over q, the
k^2-term sum, the products), so evaluating it from a given S_k costs at most gamma_{2p+q+k^2+8} mag_j,
mag_j being the same sum over absolute values.  The entries of S_k themselves carry K_FOLD stages of
gamma_{n_k} (relative to their magnitude, in the convention above).  Both are covered by

    |sse_j - direct| <= K_SSE gamma_{n_k + 2p + q + k^2 + 8} mag_j,   K_SSE = K_FOLD (+ 1 sharded).
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, make_problem
from test_stream_host import K_STAGES, L, gamma, gram_bar, merge_stream, scale_ref, split_rows

K_FOLD = K_STAGES + 2
K_FOLD_SHARDED = K_FOLD + 1
K_SELECT = K_FOLD + 1
K_SELECT_SHARDED = K_SELECT + 1
K_SSE = K_FOLD
K_SSE_SHARDED = K_FOLD_SHARDED

ENTRY_POINTS = ["ppls_stream_begin_folds", "ppls_stream_rows_folds", "ppls_stream_rows_from_folds",
                "ppls_stream_fold_info", "ppls_stream_select", "ppls_heldout_sse_fold", "ppls_cv_ppls_stream"]


def seeded_labels(n, K, seed=0):
    """Fold labels from a seeded permutation: cv_PPLS's folds for folds = rng.permutation(n)."""
    from ppls_amd import fold_labels
    return fold_labels(n, K, folds=np.random.default_rng(seed).permutation(n))


def fold_refs(X, Y, labels, K, center, scale):
    """Long-double reference: per fold the Gram of its rows after the *global* two-pass scale(), as
    float64, and (centre, scale)."""
    z, cen, sd = scale_ref(np.hstack([X, Y]), center, scale)
    return [np.asarray(z[labels == k].T @ z[labels == k], dtype=np.float64) for k in range(K)], cen, sd


def fold_stream(D, bounds, labels, K, center, scale):
    """The device's algebra in fp64 numpy: per chunk the stable fold order and one pairwise merge per
    fold segment; then recentring to the global mean, the scale from the fold-order sum, standardising.
    Returns (list of S_k, fold means, fold counts, global mean, d)."""
    P = D.shape[1]
    S = [np.zeros((P, P)) for _ in range(K)]
    m = [np.zeros(P) for _ in range(K)]
    N = [0.0] * K
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        order = np.argsort(labels[lo:hi], kind="stable")
        rows, lab = D[lo:hi][order], labels[lo:hi][order]
        for k in range(K):
            seg = rows[lab == k]
            if seg.shape[0] == 0:
                continue
            Sc, mc, nc = merge_stream(seg, [0, seg.shape[0]], center)
            if center:
                d = mc - m[k]
                S[k] = S[k] + Sc + (N[k] * nc / (N[k] + nc)) * np.outer(d, d)
                m[k] = m[k] + d * (nc / (N[k] + nc))
            else:
                S[k] = S[k] + Sc
            N[k] += nc
    Nt = sum(N)
    mg = np.zeros(P)
    for k in range(K):
        mg = mg + N[k] * m[k]
    mg = mg / Nt
    if center:
        S = [S[k] + N[k] * np.outer(m[k] - mg, m[k] - mg) for k in range(K)]
    d = np.ones(P)
    if scale:
        acc = np.zeros(P)
        for k in range(K):
            acc = acc + np.diag(S[k])
        d = np.sqrt(acc / (Nt - 1.0))
        S = [Sk / np.outer(d, d) for Sk in S]
    return S, m, N, mg, d


def sse_quadratic(Sk, p, W, C, B):
    """(sse, mag) for every prefix of the components from one fold's cross-products (joint [X Y]
    layout without padding), term for term what the device forms."""
    W, C, B = np.asarray(W, dtype=float), np.asarray(C, dtype=float), np.ravel(np.asarray(B, dtype=float))
    k = W.shape[1]
    Sxx, Sxy, Syy = Sk[:p, :p], Sk[:p, p:], Sk[p:, p:]
    A, Am = W.T @ (Sxx @ W), np.abs(W).T @ (np.abs(Sxx) @ np.abs(W))
    Dv = np.einsum("im,im->m", W, Sxy @ C)
    Dm = np.einsum("im,im->m", np.abs(W), np.abs(Sxy) @ np.abs(C))
    G, Gm = C.T @ C, np.abs(C).T @ np.abs(C)
    tr = np.trace(Syy)
    sse, mag = np.zeros(k), np.zeros(k)
    for j in range(1, k + 1):
        b = B[:j]
        sse[j - 1] = tr - 2 * np.sum(b * Dv[:j]) + np.sum(np.outer(b, b) * A[:j, :j] * G[:j, :j])
        mag[j - 1] = abs(tr) + 2 * np.sum(np.abs(b) * Dm[:j]) + np.sum(np.abs(np.outer(b, b)) * Am[:j, :j] * Gm[:j, :j])
    return sse, mag


def sse_direct(Xf, Yf, W, C, B):
    """sum_i ||y_i - x_i W_j diag(B_j) C_j'||^2 for every prefix j, in long double."""
    Xf, Yf = np.asarray(Xf, dtype=L), np.asarray(Yf, dtype=L)
    W, C, B = np.asarray(W, dtype=L), np.asarray(C, dtype=L), np.ravel(np.asarray(B, dtype=L))
    out = []
    for j in range(1, W.shape[1] + 1):
        R = Yf - (Xf @ W[:, :j]) * B[:j] @ C[:, :j].T
        out.append(float((R * R).sum()))
    return np.array(out)


def sse_bar(mag, n_f, p, q, k, k_sse=K_SSE):
    return k_sse * gamma(n_f + 2 * p + q + k * k + 8) * np.asarray(mag)


# ------------------------------------------------------------------------------ the algebra
@pytest.mark.parametrize("center,scale", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["cs", "c", "s", "none"])
@pytest.mark.parametrize("n,P,K", [(257, 11, 3), (300, 21, 5)])
def test_fold_states_meet_the_bars(n, P, K, center, scale):
    rng = np.random.default_rng(7 + n)
    D = rng.standard_normal((n, P)) * (0.5 + np.arange(P) % 3) + 0.3
    labels = seeded_labels(n, K, seed=n)
    refs, cen, sd = fold_refs(D[:, :6], D[:, 6:], labels, K, center, scale)
    for bounds in (split_rows(n), [0, n], list(range(0, n, 64)) + [n]):
        S, m, N, mg, d = fold_stream(D, bounds, labels, K, center, scale)
        assert N == [float((labels == k).sum()) for k in range(K)]
        if center:
            assert np.abs(mg - np.asarray(cen, dtype=float)).max() <= 8 * 2.0 ** -53 * max(1.0, np.abs(mg).max())
        assert np.abs(d / np.asarray(sd, dtype=float) - 1).max() <= K_FOLD * gamma(n)
        for k in range(K):
            assert np.all(np.abs(S[k] - refs[k]) <= gram_bar(refs[k], int(N[k]), K_FOLD)), (bounds, k)
            tr_ref = sum(refs[l] for l in range(K) if l != k)
            tr = np.zeros((P, P))
            for l in range(K):
                if l != k:
                    tr = tr + S[l]
            assert np.all(np.abs(tr - tr_ref) <= gram_bar(tr_ref, n - int(N[k]), K_SELECT))
            assert np.array_equal(tr, tr.T)
        allS = np.zeros((P, P))
        for l in range(K):
            allS = allS + S[l]
        assert np.all(np.abs(allS - sum(refs)) <= gram_bar(sum(refs), n, K_SELECT))


@pytest.mark.parametrize("noise", [None, 1e-3], ids=["default", "noise1e-3"])
@pytest.mark.parametrize("n,p,q,K", [(203, 12, 9, 4), (130, 33, 7, 3), (300, 130, 7, 5)])
def test_sse_quadratic_form_against_direct_residuals(n, p, q, K, noise):
    kw = {} if noise is None else dict(sigE=noise, sigF=noise, sigH=noise)
    X, Y, th0 = make_problem(n, p, q, 3, seed=4, **kw)
    Z = np.asarray(scale_ref(np.hstack([X, Y]), True, True)[0], dtype=np.float64)
    labels = seeded_labels(n, K, seed=1)
    # a fit good enough to make the expansion cancel: least squares on the other folds, rank 3
    worst = 0.0
    for f in range(K):
        tr, ho = Z[labels != f], Z[labels == f]
        coef = np.linalg.lstsq(tr[:, :p], tr[:, p:], rcond=None)[0]
        U, s, Vt = np.linalg.svd(coef, full_matrices=False)
        W, C, B = U[:, :3], Vt[:3].T, s[:3]
        sse, mag = sse_quadratic(ho.T @ ho, p, W, C, B)
        direct = sse_direct(ho[:, :p], ho[:, p:], W, C, B)
        bar = sse_bar(mag, ho.shape[0], p, q, 3)
        worst = max(worst, float(np.max(np.abs(sse - direct) / bar)))
        print(f"fold {f}: rel err {np.max(np.abs(sse - direct) / direct):.3g}, mag/sse {np.max(mag / sse):.3g}, "
              f"err/bar {np.max(np.abs(sse - direct) / bar):.3g}")
        assert np.all(np.abs(sse - direct) <= bar)
        assert np.all(mag >= np.abs(sse))
    assert worst < 1.0


# ------------------------------------------------------------------------------ interface
def test_header_declares_and_lib_binds_the_entry_points():
    from ppls_amd import _lib
    with open(os.path.join(ROOT, "include", "ppls.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "include", "ppls_debug.h")) as f:
        debug = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"\bint\s+ppls_stream_fold_get\s*\(", debug) and "ppls_stream_fold_get" in _lib.SIGNATURES
    lib = _lib.lib()
    for name in ENTRY_POINTS + ["ppls_stream_fold_get"]:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_exports():
    import ppls_amd
    assert "fold_labels" in ppls_amd.__all__ and callable(ppls_amd.fold_labels)
    for name in ("stream_select", "stream_fold_info", "heldout_sse_fold", "cv_ppls_stream", "stream_fold_get"):
        assert callable(getattr(ppls_amd.Context, name))


class _Streamed:
    """Stands in for a context streamed with 3 folds: any device call is an error."""
    p, q, n_local, n_total, row0, _stream_folds = 8, 6, 0, 30, 0, 3

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the arguments were checked")


def test_cv_argument_errors_need_no_device():
    from ppls_amd import crossval_PPLS, cv_PPLS
    c = _Streamed()
    with pytest.raises(ValueError, match="streamed with 3 folds"):
        cv_PPLS(None, None, 2, 4, ctx=c)
    with pytest.raises(ValueError, match="folds= cannot be given"):
        cv_PPLS(None, None, 2, 3, ctx=c, folds=np.arange(30))
    with pytest.raises(NotImplementedError):
        cv_PPLS(None, None, 2, 3, ctx=c, initialGuess="o2m")
    for shared in (True, False):
        with pytest.raises(ValueError, match="streamed with 3 folds"):
            crossval_PPLS(None, None, [1, 2], 5, ctx=c, shared_folds=shared)
        with pytest.raises(ValueError, match="folds= cannot be given"):
            crossval_PPLS(None, None, [1, 2], 3, ctx=c, shared_folds=shared, folds=np.arange(30))


def test_stream_data_fold_argument_checks_need_no_device():
    from ppls_amd import stream_data
    X, Y = np.zeros((4, 3)), np.zeros((4, 2))
    with pytest.raises(TypeError, match="triple"):
        stream_data([(X, Y)], nr_folds=2)
    with pytest.raises(TypeError, match="pair"):
        stream_data([(X, Y, np.zeros(4, dtype=int))])
    with pytest.raises(ValueError, match="one label per row"):
        stream_data([(X, Y, np.zeros(3, dtype=int))], nr_folds=2)
    with pytest.raises(ValueError, match="one label per row"):
        stream_data([(X, Y, np.zeros((4, 1), dtype=int))], nr_folds=2)
    with pytest.raises(TypeError, match="integers"):
        stream_data([(X, Y, np.zeros(4))], nr_folds=2)
    with pytest.raises(ValueError, match=r"0 \.\. 1"):
        stream_data([(X, Y, np.array([0, 1, 2, 0]))], nr_folds=2)
    with pytest.raises(ValueError, match=r"0 \.\. 1"):
        stream_data([(X, Y, np.array([0, -1, 1, 0]))], nr_folds=2)
    with pytest.raises(ValueError, match="1 fold does not make sense"):
        stream_data([(X, Y, np.zeros(4, dtype=int))], nr_folds=1)


@pytest.mark.parametrize("N,K", [(10, 3), (203, 4), (57, 56)])
def test_fold_labels_is_cv_runs_construction(N, K):
    from ppls_amd import cv_blocks, fold_labels
    perm = np.random.default_rng(N).permutation(N)
    lab = fold_labels(N, K, folds=perm)
    want = np.empty(N, dtype=np.int32)
    want[perm] = cv_blocks(N, K) - 1
    assert lab.dtype == np.int32 and np.array_equal(lab, want)
    for i in range(K):                               # fold i holds rows folds[blocks == i]
        assert sorted(np.flatnonzero(lab == i)) == sorted(perm[cv_blocks(N, K) == i + 1])
    # the default permutation comes from rng, as in _cv_run
    a = fold_labels(N, K, rng=np.random.default_rng(5))
    assert np.array_equal(a, fold_labels(N, K, folds=np.random.default_rng(5).permutation(N)))
    with pytest.raises(ValueError, match="permutation"):
        fold_labels(N, K, folds=np.zeros(N, dtype=int))
    with pytest.raises(ValueError, match="1 fold"):
        fold_labels(N, 1)
    with pytest.raises(ValueError, match="nr_folds"):
        fold_labels(K - 1, K)
