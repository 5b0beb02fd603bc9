"""Host side of the bootstrap: no GPU.

The bar of the weighted Gram (tests/resample_bar.py) is shown to admit a plain fp64 evaluation in the
kernel's order -- k-steps of 4 rows, the weight on one operand, the split partials added last -- and to
reject three seeded defects: the weight on both operands (c^2), the counts shifted by one row, one
count off by one.  Then the host pieces of ``bootstrap_PPLS_simult``: the counts, the sign alignment
and the se / ci aggregation against numpy on a hand-made list of replicates.
"""
import numpy as np
import pytest

from ppls_amd import align_signs, bootstrap_counts, bootstrap_summary
from resample_bar import K_W, draw_counts, inside, kernel_order, weighted_ref

SHAPES = [(1, 3, 2), (5, 3, 2), (27, 5, 3), (257, 13, 3), (64, 7, 6)]


def _rows(n, P, seed=0):
    rng = np.random.default_rng(100 * n + P + seed)
    j = np.arange(P)
    return rng.standard_normal((n, P)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7


@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("n,p,q", SHAPES)
def test_kernel_order_lies_inside_the_bar(n, p, q, nsplit):
    D = _rows(n, p + q)
    c = draw_counts(n, seed=n + nsplit)
    ok, worst = inside(kernel_order(D, c, nsplit), weighted_ref(D, c), n)
    print(f"n={n} P={p + q} nsplit={nsplit}: max err / bar {worst:.3g} (K_W = {K_W})")
    assert ok


def test_fp32_stored_rows_lie_inside_the_bar():
    D = _rows(27, 8).astype(np.float32).astype(np.float64)
    c = draw_counts(27, seed=4)
    assert inside(kernel_order(D, c, 3), weighted_ref(D, c), 27)[0]


@pytest.mark.parametrize("n,p,q", [s for s in SHAPES if s[0] > 1])
def test_seeded_defects_lie_outside_the_bar(n, p, q):
    D = _rows(n, p + q)
    c = draw_counts(n, seed=n)
    c[0], c[1] = 7, 0              # (so that c^2 != c and a shift moves something, whatever was drawn)
    ref = weighted_ref(D, c)
    assert inside(kernel_order(D, c, 2), ref, n)[0]
    assert not inside(kernel_order(D, c, 2, both=True), ref, n)[0]            # weight on both operands
    assert not inside(kernel_order(D, np.roll(c, 1), 2), ref, n)[0]           # counts shifted by one row
    off = c.copy()
    off[n // 2] += 1
    assert not inside(kernel_order(D, off, 2), ref, n)[0]                     # one count off by one


def test_all_zero_split_and_unit_counts():
    D = _rows(27, 8)
    c = draw_counts(27, seed=9)
    c[9:18] = 0                    # the whole middle split of three
    assert inside(kernel_order(D, c, 3), weighted_ref(D, c), 27)[0]
    one = np.ones(27, dtype=np.int32)
    assert inside(kernel_order(D, one, 3), np.asarray(D.T.astype(np.longdouble) @ D.astype(np.longdouble)), 27)[0]


# ------------------------------------------------------------------------------ the host pieces
def test_bootstrap_counts():
    c = bootstrap_counts(37, 5, 11)
    assert c.shape == (5, 37) and c.dtype == np.int32
    assert np.all(c.sum(axis=1) == 37) and c.min() >= 0
    assert np.array_equal(c, bootstrap_counts(37, 5, 11))                       # the same seed, the same array
    assert np.array_equal(c, bootstrap_counts(37, 5, np.random.default_rng(11)))
    assert not np.array_equal(c, bootstrap_counts(37, 5, 12))
    assert len({tuple(r) for r in c}) == 5
    rng = np.random.default_rng(3)
    a, b = bootstrap_counts(9, 2, rng), bootstrap_counts(9, 2, rng)             # a Generator is drawn from, not copied
    assert not np.array_equal(a, b)
    assert bootstrap_counts(4, 0).shape == (0, 4)
    big = bootstrap_counts(2000, 50, 1)                                         # about exp(-1) of the rows left out
    assert abs((big == 0).mean() - np.exp(-1.0)) < 0.01
    with pytest.raises(ValueError):
        bootstrap_counts(0, 3)


def test_align_signs():
    W0 = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, -1.0], [0.0, 0.0, 0.5]])
    W = W0 * np.array([-1.0, 1.0, -1.0]) + 0.01
    out = align_signs(W, W0)
    assert np.array_equal(out, W * np.array([-1.0, 1.0, -1.0]))
    assert np.all(np.diag(out.T @ W0) > 0)
    Z = np.array([[1.0, 1.0], [1.0, -1.0]])
    assert np.array_equal(align_signs(Z, Z[:, ::-1]), Z)       # zero inner products count as +1, nothing is reordered
    assert align_signs(np.array([1.0, -2.0]), np.array([-1.0, 2.0])).shape == (1, 2)
    with pytest.raises(ValueError):
        align_signs(np.ones((3, 2)), np.ones((3, 1)))


def _replicates(nrep=7, p=4, q=3, a=2, seed=5):
    rng = np.random.default_rng(seed)
    return [dict(W=rng.standard_normal((p, a)), C=rng.standard_normal((q, a)), B=np.diag(rng.uniform(1, 2, a)),
                 sigE=float(rng.uniform()), sigF=float(rng.uniform()), sigH=np.array([[rng.uniform()]]),
                 sigT=np.diag(rng.uniform(0.5, 1, a))) for _ in range(nrep)]


@pytest.mark.parametrize("level", [0.95, 0.5])
def test_summary_against_numpy(level):
    reps = _replicates()
    se, ci = bootstrap_summary(reps, level)
    assert sorted(se) == sorted(ci) == sorted(["W", "C", "B", "sigE", "sigF", "sigH", "sigT"])
    lo_q, hi_q = (1 - level) / 2, (1 + level) / 2
    for k in ("W", "C"):
        A = np.stack([r[k] for r in reps])
        assert np.array_equal(se[k], A.std(axis=0, ddof=1)) and se[k].shape == reps[0][k].shape
        assert np.array_equal(ci[k][0], np.quantile(A, lo_q, axis=0)) and np.array_equal(ci[k][1], np.quantile(A, hi_q, axis=0))
    for k in ("B", "sigT"):                       # as their diagonals
        A = np.stack([np.diag(r[k]) for r in reps])
        assert se[k].shape == (2,) and np.array_equal(se[k], A.std(axis=0, ddof=1))
        assert np.array_equal(ci[k][0], np.quantile(A, lo_q, axis=0)) and np.array_equal(ci[k][1], np.quantile(A, hi_q, axis=0))
    for k in ("sigE", "sigF", "sigH"):
        A = np.array([float(np.ravel(r[k])[0]) for r in reps])
        assert np.ndim(se[k]) == 0 and se[k] == A.std(ddof=1)
        assert ci[k][0] == np.quantile(A, lo_q) and ci[k][1] == np.quantile(A, hi_q)
        assert ci[k][0] <= ci[k][1]


def test_summary_needs_two_replicates():
    with pytest.raises(ValueError, match="needs two"):
        bootstrap_summary(_replicates(1))
    with pytest.raises(ValueError, match="level"):
        bootstrap_summary(_replicates(3), 1.0)


def test_entry_points_are_declared():
    import os
    from conftest import ROOT
    from ppls_amd import _lib
    with open(os.path.join(ROOT, "include", "ppls.h")) as f:
        assert "int ppls_xprod_resample(ppls_ctx* dst, ppls_ctx* src, const int32_t* count" in f.read()
    with open(os.path.join(ROOT, "include", "ppls_debug.h")) as f:
        dbg = f.read()
    assert "int ppls_gram_weighted(" in dbg and "int ppls_gram_occupancy_weighted(int f32);" in dbg
    for name in ("ppls_xprod_resample", "ppls_gram_weighted", "ppls_gram_occupancy_weighted"):
        assert name in _lib.SIGNATURES
