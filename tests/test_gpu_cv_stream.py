"""Cross-validation from row chunks on the device: a stream opened with folds keeps one
cross-product matrix per fold; selections, held-out errors and cv_PPLS / crossval_PPLS read only them.

References: the long-double two-pass Gram of each fold's rows after the *global* scale()
(test_cv_stream_host.fold_refs), and the resident path -- scale_data, then cv_PPLS / heldout_sse /
fits on gathered rows -- on the same folds and starts.  Bars: test_cv_stream_host's stage counts for
S, the project's 1e-8 / 1e-10 / 1e-12 for fits, RMSEP and sharding.
"""
import ctypes as ct
import functools
import threading
import warnings

import numpy as np
import pytest

from conftest import make_problem
from test_cv_stream_host import (K_FOLD, K_FOLD_SHARDED, K_SELECT, K_SSE, fold_refs, seeded_labels, sse_bar)
from test_gpu_stream import ThreadAllReduce, _ctx, _data, _relerr, _stream
from test_stream_host import gram_bar, split_rows

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
STREAMED = "the rows were streamed and are not resident"
SHAPES = [(300, 12, 9, 2), (257, 33, 7, 3), (400, 130, 7, 5), (350, 5, 140, 3)]     # n, p, q, K


def _stream_folds(c, X, Y, labels, K, bounds, center=True, scale=True, order="C"):
    c.stream_begin(X.shape[1], Y.shape[1], center, scale, nr_folds=K)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        c.stream_rows(np.array(X[lo:hi], order=order), np.array(Y[lo:hi], order=order), labels[lo:hi])
    return c.stream_end()


@functools.lru_cache(maxsize=None)
def _refs(n, p, q, K, center, scale):
    """Long-double fold references of _data(n, p, q) under seeded labels, computed once and shared."""
    X, Y = _data(n, p, q)
    labels = seeded_labels(n, K, seed=n)
    refs, cen, sd = fold_refs(X, Y, labels, K, center, scale)
    for r in refs:
        r.setflags(write=False)
    labels.setflags(write=False)
    return refs, labels, np.asarray(cen, dtype=float), np.asarray(sd, dtype=float)


def _within(tag, S, ref, n, k):
    bar = gram_bar(ref, n, k)
    err = np.abs(S - ref)
    print(f"{tag}: max |S - ref| {err.max():.3g}, max err / bar {np.max(err / bar):.3g}")
    assert S.shape == ref.shape and np.all(err <= bar), tag


def _check_padded(c, k, p, q):
    Sp, _, _ = c.stream_fold_get(k, padded=True)
    _, ldx = c.xprod_matrix(padded=True)
    live = np.zeros(Sp.shape[0], dtype=bool)
    live[:p] = True
    live[ldx:ldx + q] = True
    assert np.array_equal(Sp, Sp.T)
    assert not Sp[~live].any() and not Sp[:, ~live].any()


# ------------------------------------------------------------------------------ 1. fold matrices
@pytest.mark.parametrize("n,p,q,K", SHAPES)
def test_fold_matrices(n, p, q, K):
    X, Y = _data(n, p, q)
    bounds = split_rows(n)
    with _ctx() as c, _ctx() as plain:
        for center, scale, order in [(True, True, "C"), (True, True, "F"), (True, False, "C"), (False, True, "C"),
                                     (False, False, "C")]:
            refs, labels, cen, sd = _refs(n, p, q, K, center, scale)
            out = _stream_folds(c, X, Y, labels, K, bounds, center, scale, order)
            counts = np.bincount(labels, minlength=K)
            assert out["n"] == n and np.array_equal(out["fold_total"], counts)
            info = c.stream_fold_info()
            assert info["nr_folds"] == K and info["selected"] == -1 and np.array_equal(info["fold_total"], counts)
            got_c = np.r_[out["centerX"], out["centerY"]]
            got_s = np.r_[out["scaleX"], out["scaleY"]]
            assert np.abs(got_c - cen).max() <= 8 * 2.0 ** -53 * max(1.0, np.abs(cen).max())
            assert _relerr(got_s, sd) <= 1e-12
            for k in range(K):
                S, mean, nk = c.stream_fold_get(k)
                assert nk == counts[k]
                _within(f"{center},{scale},{order} fold {k}", S, refs[k], int(counts[k]), K_FOLD)
                _check_padded(c, k, p, q)
                if center:
                    D = np.hstack([X, Y])[labels == k]
                    # <= 6 chunk updates of <= 4 roundings each, of values bounded by max |D|
                    assert np.abs(mean - D.mean(axis=0)).max() <= 32 * 2.0 ** -53 * np.abs(D).max()
            S_all = c.xprod_matrix()
            ref_all = sum(refs)
            _within("all folds", S_all, ref_all, n, K_SELECT)
            Sp, _ = c.xprod_matrix(padded=True)
            assert np.array_equal(Sp, Sp.T)
            _stream(plain, X, Y, bounds, center, scale, order)
            assert np.all(np.abs(S_all - plain.xprod_matrix()) <= gram_bar(ref_all, n, K_SELECT))
            assert c.stream_info()["n_total"] == n and c.streamed


# ------------------------------------------------------------------------------ 2. select
@pytest.mark.parametrize("n,p,q,K", [SHAPES[1], SHAPES[2]])
def test_select(n, p, q, K):
    X, Y = _data(n, p, q)
    refs, labels, _, _ = _refs(n, p, q, K, True, True)
    counts = np.bincount(labels, minlength=K)
    one = [dict(W=np.eye(p)[:, :1], C=np.eye(q)[:, :1], B=1.0, sigE=1.0, sigF=1.0, sigH=0.5, sigT=1.0)] * 2
    with _ctx() as c:
        _stream_folds(c, X, Y, labels, K, split_rows(n))
        first = c.ppls(2, 20, -1.0, one)
        for k in list(range(K)) + [-1]:
            c.stream_select(k)
            ref = sum(refs[l] for l in range(K) if l != k)
            nt = n - (counts[k] if k >= 0 else 0)
            S = c.xprod_matrix()
            _within(f"select {k}", S, ref, int(nt), K_SELECT)
            assert c.stream_info()["n_total"] == nt == c.n_total and c.stream_fold_info()["selected"] == k
            ssq = c.ssq()
            assert ssq[0] == pytest.approx(np.trace(S[:p, :p]), rel=1e-14)
            assert ssq[1] == pytest.approx(np.trace(S[p:, p:]), rel=1e-14)
        c.stream_select(1)
        other = c.ppls(2, 20, -1.0, one)
        assert not np.array_equal(other["W"], first["W"])
        c.stream_select(-1)
        again = c.ppls(2, 20, -1.0, one)
        for key in ("W", "C", "B", "sig"):
            assert np.array_equal(again[key], first[key]), key
        assert np.array_equal(again["Other_output"]["Loglikelihoods"], first["Other_output"]["Loglikelihoods"])


# ------------------------------------------------------------------------------ 3. held-out error
@pytest.mark.parametrize("n,p,q,K", SHAPES)
def test_heldout_error_against_resident_rows(n, p, q, K):
    r = 3
    X, Y, th0 = make_problem(n, p, q, r, seed=11)
    labels = seeded_labels(n, K, seed=n)
    with _ctx() as c, _ctx() as res:
        _stream_folds(c, X, Y, labels, K, split_rows(n))
        res.set_data(X, Y)
        res.scale_data(True, True)
        inits = [dict(W=th0["W"][:, j:j + 1], C=th0["C"][:, j:j + 1], B=1.0, sigE=1.0, sigF=1.0, sigH=0.5, sigT=1.0)
                 for j in range(r)]
        worst = 0.0
        for f in range(K):
            c.stream_select(f)
            fit = c.ppls(r, 15, -1.0, inits)
            rows = np.flatnonzero(labels == f)
            want = res.heldout_sse(fit["W"], fit["C"], fit["B"], rows)
            sse, mag = c.heldout_sse_fold(fit["W"], fit["C"], fit["B"], f)
            sse2, mag2 = c.heldout_sse_fold(fit["W"], fit["C"], fit["B"], f)
            assert np.array_equal(sse, sse2) and np.array_equal(mag, mag2)
            bar = sse_bar(mag, rows.shape[0], p, q, r, K_SSE)
            ratio = np.abs(sse - want) / bar
            worst = max(worst, float(ratio.max()))
            print(f"fold {f}: rel err {np.max(np.abs(sse - want) / want):.3g}, mag/sse {np.max(mag / sse):.3g}, "
                  f"err/bar {ratio.max():.3g}")
            assert np.all(mag >= np.abs(sse))
            assert np.all(np.abs(sse - want) <= bar)
        print(f"worst err / bar {worst:.3g}")


# ------------------------------------------------------------------------------ 4. CV parity
@pytest.mark.parametrize("n,p,q,K", SHAPES)
def test_cv_parity_with_resident_rows(n, p, q, K):
    from ppls_amd import cv_PPLS
    a = 3
    X, Y, _ = make_problem(n, p, q, a, seed=12)
    perm = np.random.default_rng(n).permutation(n)
    labels = seeded_labels(n, K, seed=n)
    with _ctx() as c, _ctx() as res:
        _stream_folds(c, X, Y, labels, K, split_rows(n))
        res.set_data(X, Y)
        res.scale_data(True, True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            mean, err = cv_PPLS(None, None, a, K, ctx=c, per_fold=True, EMsteps=30, atol=-1.0)
        mean_r, err_r = cv_PPLS(None, None, a, K, folds=perm, ctx=res, per_fold=True, EMsteps=30, atol=-1.0)
        print(f"per-fold RMSEP rel err {_relerr(err, err_r):.3g}")
        assert np.all(np.abs(err - err_r) <= 1e-8 * np.abs(err_r))
        assert abs(mean - mean_r) <= 1e-8 * abs(mean_r)
        assert c.stream_fold_info()["selected"] == -1 and c.n_total == n


def test_fit_after_select_and_stop_rule():
    from ppls_amd import cv_PPLS, initial_guess
    n, p, q, K, a = 257, 33, 7, 3, 2
    X, Y, _ = make_problem(n, p, q, a, seed=13)
    perm = np.random.default_rng(n).permutation(n)
    labels = seeded_labels(n, K, seed=n)
    inits = [initial_guess(p, q, "equal") for _ in range(a)]
    with _ctx() as c, _ctx() as res, _ctx() as train:
        _stream_folds(c, X, Y, labels, K, split_rows(n))
        res.set_data(X, Y)
        res.scale_data(True, True)
        train.set_data_from(res, np.flatnonzero(labels != 1))
        for steps, atol in ((30, -1.0), (100, 1e-4)):
            c.stream_select(1)
            got = c.ppls(a, steps, atol, inits)
            want = train.ppls(a, steps, atol, inits)
            assert np.array_equal(got["Other_output"]["Number_steps"], want["Other_output"]["Number_steps"])
            assert np.abs(got["W"] - want["W"]).max() < 1e-8 and np.abs(got["C"] - want["C"]).max() < 1e-8
            assert _relerr(got["B"], want["B"]) < 1e-8 and _relerr(got["sig"], want["sig"]) < 1e-8
            assert _relerr(got["Other_output"]["Loglikelihoods"], want["Other_output"]["Loglikelihoods"]) < 1e-10
            c.stream_select(-1)
        _, err = cv_PPLS(None, None, a, K, ctx=c, per_fold=True, EMsteps=100, atol=1e-4)
        _, err_r = cv_PPLS(None, None, a, K, folds=perm, ctx=res, per_fold=True, EMsteps=100, atol=1e-4)
        assert np.all(np.abs(err - err_r) <= 1e-8 * np.abs(err_r))


def test_crossval_shared_and_separate_folds_agree():
    from ppls_amd import crossval_PPLS
    n, p, q, K = 300, 12, 9, 5
    X, Y, _ = make_problem(n, p, q, 3, seed=14)
    labels = seeded_labels(n, K, seed=n)
    from ppls_amd import stream_data
    b = split_rows(n)
    with _ctx() as c:
        out = stream_data(((X[lo:hi], Y[lo:hi], labels[lo:hi]) for lo, hi in zip(b[:-1], b[1:])), ctx=c, nr_folds=K)
        assert out["n"] == n and np.array_equal(out["fold_total"], np.bincount(labels, minlength=K))
        args = dict(EMsteps=30, atol=-1.0)
        shared = crossval_PPLS(None, None, [1, 2, 3], K, shared_folds=True, ctx=c, **args)
        sep = crossval_PPLS(None, None, [1, 2, 3], K, shared_folds=False, ctx=c, **args)
        assert np.all(np.abs(shared["errors"] - sep["errors"]) <= 1e-12 * np.abs(sep["errors"]))
        assert shared["a_min"] == sep["a_min"] and shared["class"] == "cvPPLS"
        rnd = crossval_PPLS(None, None, [2], K, shared_folds=True, ctx=c, initialGuess="random",
                            rng=np.random.default_rng(3), **args)
        assert np.isfinite(rnd["errors"]).all()


# ------------------------------------------------------------------------------ 5. chunking, repeatability
def test_chunking_invariance_and_repeatability():
    n, p, q, K = 300, 12, 9, 3
    X, Y = _data(n, p, q)
    refs, labels, _, _ = _refs(n, p, q, K, True, True)
    labels = np.array(labels)
    # fold 2 arrives in one chunk only (rows 128..193), and is absent from every other chunk
    labels[labels == 2] = np.arange((labels == 2).sum()) % 2
    labels[130:190] = 2
    refs = fold_refs(X, Y, labels, K, True, True)[0]
    counts = np.bincount(labels, minlength=K)
    bounds = split_rows(n)
    with _ctx() as c, _ctx() as c2, _ctx() as src:
        _stream_folds(c, X, Y, labels, K, bounds)
        base = [c.stream_fold_get(k)[0] for k in range(K)]
        for k in range(K):
            _within(f"fold {k}", base[k], refs[k], int(counts[k]), K_FOLD)
        _stream_folds(c2, X, Y, labels, K, bounds)                       # the same bits in a second context
        for k in range(K):
            assert np.array_equal(c2.stream_fold_get(k)[0], base[k])
        assert np.array_equal(c2.xprod_matrix(), c.xprod_matrix())
        for other in ([0, n], list(range(0, n, 64)) + [n]):
            _stream_folds(c2, X, Y, labels, K, other)
            for k in range(K):
                assert np.all(np.abs(c2.stream_fold_get(k)[0] - base[k]) <= gram_bar(refs[k], int(counts[k]), K_FOLD))
        # device chunks with labels
        c2.stream_begin(p, q, True, True, nr_folds=K)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            src.set_data(X[lo:hi], Y[lo:hi])
            c2.stream_rows_from(src, labels[lo:hi])
        c2.stream_end()
        for k in range(K):
            assert np.all(np.abs(c2.stream_fold_get(k)[0] - base[k]) <= gram_bar(refs[k], int(counts[k]), K_FOLD))


# ------------------------------------------------------------------------------ 6. shards
def _run_fold_ranks(X, Y, labels, K, chunks, work):
    """Three contexts on GPU 0 with the host reducer; rank i streams the row index lists chunks[i]."""
    red = ThreadAllReduce(3)
    out, errs = [None] * 3, []

    def body(rank):
        try:
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                c.stream_begin(X.shape[1], Y.shape[1], True, True, nr_folds=K)
                for idx in chunks[rank]:
                    c.stream_rows(X[idx], Y[idx], labels[idx])
                out[rank] = work(c, rank)
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
    if errs:
        raise errs[0]
    return out


def test_sharded_fold_stream_equals_one_context():
    from ppls_amd import cv_PPLS
    n, p, q, K, a = 300, 12, 9, 3, 2
    X, Y, _ = make_problem(n, p, q, a, seed=15)
    labels = seeded_labels(n, K, seed=n)
    late = np.arange(150, n)
    # rank 0: two chunks, all folds; rank 1: no row of fold 0; rank 2: no rows
    chunks = [[np.arange(0, 1), np.r_[np.arange(1, 150), late[labels[late] == 0]]], [late[labels[late] != 0]], []]

    def work(c, rank):
        out = c.stream_end()
        mats = [c.stream_fold_get(k)[0] for k in range(K)]
        _, err = cv_PPLS(None, None, a, K, ctx=c, per_fold=True, EMsteps=30, atol=-1.0)
        return out, mats, err

    outs = _run_fold_ranks(X, Y, labels, K, chunks, work)
    refs = fold_refs(X, Y, labels, K, True, True)[0]
    counts = np.bincount(labels, minlength=K)
    with _ctx() as one:
        one.stream_begin(p, q, True, True, nr_folds=K)
        for ch in chunks:
            for idx in ch:
                one.stream_rows(X[idx], Y[idx], labels[idx])
        one.stream_end()
        _, err1 = cv_PPLS(None, None, a, K, ctx=one, per_fold=True, EMsteps=30, atol=-1.0)
    for rank, (out, mats, err) in enumerate(outs):
        assert out["n"] == n and np.array_equal(out["fold_total"], counts)
        for k in range(K):
            assert np.array_equal(mats[k], outs[0][1][k])                    # every rank: the same bits
            _within(f"rank {rank} fold {k}", mats[k], refs[k], int(counts[k]), K_FOLD_SHARDED)
        assert np.array_equal(err, outs[0][2])
        assert np.all(np.abs(err - err1) <= 1e-12 * np.abs(err1))


def test_sharded_empty_fold_is_refused_on_every_rank():
    from ppls_amd import PplsError
    n, p, q, K = 120, 12, 9, 3
    X, Y = (np.array(v) for v in _data(n, p, q))
    labels = (np.arange(n) % 2).astype(np.int32)                              # fold 2 never appears
    chunks = [[np.arange(0, 50)], [np.arange(50, n)], []]

    def work(c, rank):
        try:
            c.stream_end()
        except PplsError as e:
            return e.code, str(e), c.stream_info()["state"], c.stream_fold_info()["nr_folds"]
        return 0, "", "", -1

    for code, msg, state, nf in _run_fold_ranks(X, Y, labels, K, chunks, work):
        assert code == E_ARG and "fold 2 " in msg and state == "none" and nf == 0


# ------------------------------------------------------------------------------ 7. state
def test_fold_stream_state_and_refusals():
    from ppls_amd import PplsError, Theta, cv_PPLS, crossval_PPLS
    from ppls_amd._lib import dptr
    n, p, q, r, K = 120, 12, 9, 2, 3
    X, Y, th0 = make_problem(n, p, q, r, seed=2)
    th = Theta(th0["W"], th0["C"], th0["B"], th0["sigE"], th0["sigF"], th0["sigH"], th0["sigT"])
    one = dict(W=th0["W"][:, :1], C=th0["C"][:, :1], B=1.0, sigE=1.0, sigF=1.0, sigH=0.5, sigT=1.0)
    labels = seeded_labels(n, K, seed=1)
    i32 = ct.POINTER(ct.c_int32)
    with _ctx() as c, _ctx() as other, _ctx() as plain:
        other.set_data(X[:50], Y[:50])
        # while open: the unlabelled calls are refused, a bad label leaves the stream usable
        c.stream_begin(p, q, True, True, nr_folds=K)
        c.stream_rows(X[:50], Y[:50], labels[:50])
        for call in (lambda: c.stream_rows(X[50:], Y[50:]), lambda: c.stream_rows_from(other)):
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE
        bad = np.array(labels[50:], dtype=np.int32)
        bad[7] = K
        Xc, Yc = np.ascontiguousarray(X[50:]), np.ascontiguousarray(Y[50:])
        assert c._L.ppls_stream_rows_folds(c.h, dptr(Xc), dptr(Yc), n - 50, 1, bad.ctypes.data_as(i32)) == E_ARG
        assert c._L.ppls_stream_rows_from_folds(c.h, other.h, (np.zeros(50, dtype=np.int32) - 1).ctypes.data_as(i32)) == E_ARG
        with pytest.raises(ValueError):
            c.stream_rows(X[50:], Y[50:], bad)
        assert c.stream_info()["rows_local"] == 50 and c.stream_fold_info()["nr_folds"] == K
        c.stream_rows(X[50:], Y[50:], labels[50:])
        c.stream_end()
        est, ll, _, _ = c.em_run(th, 5, -np.inf, 0, want_mu=False)
        calls = dict(
            scores=lambda: c.scores(th0["W"], th0["C"]),
            variances=lambda: c.variances(np.zeros((0, r)), np.ones(r), 0.5, 0),
            heldout_sse=lambda: c.heldout_sse(th0["W"], th0["C"], np.diag(th0["B"]), []),
            cv_ppls=lambda: c.cv_ppls(1, [], [60, 60], 5, 1e-4, [[one], [one]]),
            set_data_from=lambda: other.set_data_from(c, []),
            xprod_downdate=lambda: other.xprod_downdate(c, [0]),
            scale_data=lambda: c.scale_data(),
            meta_ppls=lambda: c.meta_ppls([60, 60], 3, 1e-4, one),
            get_data=lambda: c.get_data(0, 0),
        )
        for name, call in calls.items():
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE and STREAMED in str(e.value), f"{name}: {e.value}"
        with pytest.raises(PplsError) as e:
            c.stream_select(K)
        assert e.value.code == E_ARG
        with pytest.raises(PplsError) as e:
            c.heldout_sse_fold(th0["W"], th0["C"], np.diag(th0["B"]), -1)
        assert e.value.code == E_ARG
        c.em_begin(th)                                   # a session on the selected S: no select, no CV
        for call in (lambda: c.stream_select(0), lambda: cv_PPLS(None, None, 1, K, ctx=c)):
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE
        assert c.stream_fold_info()["selected"] == -1
        # none of the refusals disturbed the state: the same run again, bit for bit
        est2, ll2, _, _ = c.em_run(th, 5, -np.inf, 0, want_mu=False)
        assert np.array_equal(ll, ll2) and np.array_equal(est.W, est2.W)
        assert np.isfinite(cv_PPLS(None, None, 1, K, ctx=c, EMsteps=5))
        # a plain stream: no folds, CV refused as before, the fold calls PPLS_E_STATE
        _stream(plain, X, Y, [0, 50, n], True, True)
        info = plain.stream_fold_info()
        assert info["nr_folds"] == 0 and info["fold_total"].shape == (0,) and info["selected"] == -1
        for call in (lambda: cv_PPLS(None, None, 1, 2, ctx=plain, rng=np.random.default_rng(0)),
                     lambda: crossval_PPLS(None, None, [1], 2, ctx=plain)):
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE and STREAMED in str(e.value)
        for call in (lambda: plain.stream_select(0), lambda: plain.stream_fold_get(0),
                     lambda: plain.heldout_sse_fold(th0["W"], th0["C"], np.diag(th0["B"]), 0)):
            with pytest.raises(PplsError) as e:
                call()
            assert e.value.code == E_STATE
        plain.stream_begin(p, q, True, True)
        with pytest.raises(PplsError) as e:
            plain.stream_rows(X[:50], Y[:50], labels[:50])
        assert e.value.code == E_STATE
        # xprod_release ends the state and frees the folds
        c.xprod_release()
        assert c.stream_info()["state"] == "none" and c.stream_fold_info()["nr_folds"] == 0
        with pytest.raises(PplsError) as e:
            c.stream_select(-1)
        assert e.value.code == E_STATE
