"""Host side of the cross-validation interface (crossval_PPLS.R:12-114): no GPU.

The fold construction restated from R's cut.default, the argument errors of crossval_PPLS and
predict_PPLS (raised before any device call: a machine without a GPU sees them), and the five entry
points in the header and the ctypes table.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

CV_ENTRY_POINTS = ["ppls_set_data_from", "ppls_xprod_downdate", "ppls_predict", "ppls_heldout_sse", "ppls_cv_ppls"]


def _api():
    from ppls_amd import api
    return api


@pytest.mark.parametrize("N,K,sizes", [(10, 3, [4, 3, 3]), (203, 4, [51, 51, 50, 51])])
def test_cv_blocks_sizes(N, K, sizes):
    b = _api().cv_blocks(N, K)
    assert b.shape == (N,) and b.min() == 1 and b.max() == K
    assert np.bincount(b, minlength=K + 1)[1:].tolist() == sizes
    assert np.all(np.diff(b) >= 0)


@pytest.mark.parametrize("N", [2, 7, 23, 100])
def test_cv_blocks_leave_one_out(N):
    assert _api().cv_blocks(N, N).tolist() == list(range(1, N + 1))


@pytest.mark.parametrize("N,K", [(11, 2), (130, 3), (1000, 7), (57, 56)])
def test_cv_blocks_labels_non_decreasing_and_complete(N, K):
    b = _api().cv_blocks(N, K)
    assert np.all(np.diff(b) >= 0) and np.all(np.diff(b) <= 1)
    assert sorted(set(b.tolist())) == list(range(1, K + 1))
    sizes = np.bincount(b)[1:]
    assert sizes.max() - sizes.min() <= 1


def _data(n=30, p=8, q=6, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    Y = rng.standard_normal((n, q))
    return X - X.mean(0), Y - Y.mean(0)


def test_crossval_one_fold_is_an_error():
    X, Y = _data()
    with pytest.raises(ValueError, match="Cross-validation with 1 fold does not make sense, use 2 folds or more"):
        _api().crossval_PPLS(X, Y, [1, 2], 1)
    with pytest.raises(ValueError, match="1 fold does not make sense"):
        _api().cv_PPLS(X, Y, 1, 1)


def test_crossval_a_too_large_and_bad_counts():
    api = _api()
    X, Y = _data()
    with pytest.raises(ValueError, match=r"ncol\(Y\) > max\(a\)"):
        api.crossval_PPLS(X, Y, [1, 6], 3)          # ncol(Y) = 6 is not > 6
    with pytest.raises(ValueError, match=r"ncol\(X\) > max\(a\)"):
        api.crossval_PPLS(X, Y, [8], 3)
    with pytest.raises(ValueError, match="nr_folds"):
        api.crossval_PPLS(X, Y, [1], 31)            # more folds than rows
    with pytest.raises(ValueError, match="nr_cores"):
        api.crossval_PPLS(X, Y, [1], 3, nr_cores=1.5)
    with pytest.raises(NotImplementedError):
        api.crossval_PPLS(X, Y, [1], 3, initialGuess="o2m")
    with pytest.raises(TypeError):
        api.crossval_PPLS(X, Y, [1], 3, constraints=[None])


def test_crossval_warns_on_uncentred_data_before_the_checks():
    X, Y = _data()
    with pytest.warns(UserWarning, match="Data is not centered, proceeding..."):
        with pytest.raises(ValueError):
            _api().crossval_PPLS(X + 1.0, Y, [1], 1)


def test_predict_column_mismatch():
    api = _api()
    fit = dict(W=np.ones((8, 2)), C=np.ones((6, 2)), B=np.ones(2))
    with pytest.raises(ValueError, match="Number of columns mismatch!"):
        api.predict_PPLS(fit, np.zeros((4, 6)), "X")
    with pytest.raises(ValueError, match="Number of columns mismatch!"):
        api.predict_PPLS(fit, np.zeros((4, 8)), "Y")
    with pytest.raises(ValueError, match="Number of columns mismatch!"):
        api.predict_PPLS(fit, np.zeros(7))            # a vector is one row, t(newdata)
    with pytest.raises(ValueError, match="should be one of"):
        api.predict_PPLS(fit, np.zeros((4, 8)), "Z")


def test_header_declares_and_lib_binds_the_entry_points():
    from ppls_amd import _lib
    with open(os.path.join(ROOT, "include", "ppls.h")) as f:
        header = f.read()
    for name in CV_ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.lib()
    for name in CV_ENTRY_POINTS:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the header cites the reference lines each of them replaces
    assert "crossval_PPLS.R:12-114" in header and "mean((x - y)^2)" in header


def test_exports():
    import ppls_amd
    for name in ("cv_blocks", "predict_PPLS", "cv_PPLS", "crossval_PPLS"):
        assert name in ppls_amd.__all__ and callable(getattr(ppls_amd, name))
    for name in ("set_data_from", "xprod_downdate", "predict", "heldout_sse", "cv_ppls"):
        assert callable(getattr(ppls_amd.Context, name))
