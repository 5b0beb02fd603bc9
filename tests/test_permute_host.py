"""Host side of the permutation test: no GPU.

The bar of the permuted cross block (tests/permute_bar.py) is shown to admit a plain fp64 evaluation in
the kernel's order -- k-steps of 4 rows, X's row i against Y's row perm[i], the split partials added
last -- for every shape, storage type and permutation tests/test_gpu_permute.py runs, and to reject four
seeded defects: Y gathered by the inverse permutation, no permutation at all, both operands permuted,
the mirror block written without the transposition.  The defects use the cyclic shift and the random
permutation: the identity and the reversal are involutions and cannot tell perm from its inverse.  Then
the host pieces of ``permutation_PPLS``: the permutations and the p-value formula on hand-made arrays.
"""
import numpy as np
import pytest

from ppls_amd import permutation_indices, permutation_pvalues
from permute_bar import K_P, inside, kernel_order, permutations, permuted_bar, permuted_ref

SHAPES = [(1, 3, 2), (5, 3, 2), (27, 5, 3), (257, 130, 3), (64, 70, 61), (33, 3, 130)]
PERMS = ("identity", "reversal", "shift", "random")


def _rows(n, p, q, f32):
    """tests/test_gpu_resample.py::_kernel_rows, as the context stores them."""
    rng = np.random.default_rng(1000 * n + 10 * p + q)

    def block(m):
        j = np.arange(m)
        return rng.standard_normal((n, m)) * (0.5 + j % 7) + (j % 5 - 2) * 0.7
    X, Y = block(p), block(q)
    if f32:
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    return X, Y


def _inverse(perm):
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    return inv


def _mirror(C, transposed=True):
    """The q x p block below the diagonal as written from C (p x q, column-major): S[ldx + b, a] = C[a, b];
    the defect copies C's memory as it lies."""
    return C.T.copy() if transposed else np.reshape(np.asfortranarray(C), C.shape[::-1], order="F")


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n,p,q", SHAPES)
def test_kernel_order_lies_inside_the_bar(n, p, q, f32, nsplit):
    X, Y = _rows(n, p, q, f32)
    bar = permuted_bar(X, Y, n, nsplit)
    for name, perm in permutations(n, seed=7 * n + p).items():
        C = kernel_order(X, Y, perm, nsplit)
        ref = permuted_ref(X, Y, perm)
        ok, worst = inside(C, ref, bar)
        print(f"n={n} p={p} q={q} {name} nsplit={nsplit}: max err / bar {worst:.3g} (K_P = {K_P})")
        assert ok
        assert inside(_mirror(C), ref.T, bar.T)[0]


@pytest.mark.parametrize("which", ["shift", "random"])
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n,p,q", [s for s in SHAPES if s[0] >= 5])
def test_seeded_defects_lie_outside_the_bar(n, p, q, f32, which):
    X, Y = _rows(n, p, q, f32)
    perm = permutations(n, seed=7 * n + p)[which]
    inv, ident = _inverse(perm), np.arange(n)
    assert not np.array_equal(perm, inv) and not np.array_equal(perm, ident)
    ref, bar = permuted_ref(X, Y, perm), permuted_bar(X, Y, n, 3)
    good = kernel_order(X, Y, perm, 3)
    assert inside(good, ref, bar)[0]
    worst = {}
    worst["inverse"] = inside(kernel_order(X, Y, inv, 3), ref, bar)            # Y gathered by the inverse permutation
    worst["none"] = inside(kernel_order(X, Y, ident, 3), ref, bar)             # no permutation at all
    worst["both"] = inside(kernel_order(X[perm], Y, perm, 3), ref, bar)        # both operands permuted
    worst["mirror"] = inside(_mirror(good, transposed=False), ref.T, bar.T)    # the mirror block not transposed
    print(f"n={n} p={p} q={q} {which}: " + ", ".join(f"{k} {v[1]:.3g} bars" for k, v in worst.items()))
    for k, (ok, _) in worst.items():
        assert not ok, k


def test_helper_permutations():
    for n in (1, 2, 5, 33):
        ps = permutations(n, seed=n)
        assert sorted(ps) == sorted(PERMS)
        for perm in ps.values():
            assert perm.dtype == np.int64 and np.array_equal(np.sort(perm), np.arange(n))
    ps = permutations(5, seed=3)
    assert np.array_equal(ps["shift"], [1, 2, 3, 4, 0]) and np.array_equal(ps["reversal"], [4, 3, 2, 1, 0])
    assert not np.array_equal(ps["random"], _inverse(ps["random"]))           # not an involution


# ------------------------------------------------------------------------------ the host pieces
def test_permutation_indices():
    P = permutation_indices(37, 5, 11)
    assert P.shape == (5, 37) and P.dtype == np.int64
    assert np.array_equal(np.sort(P, axis=1), np.tile(np.arange(37), (5, 1)))   # every row a permutation
    assert np.array_equal(P, permutation_indices(37, 5, 11))                    # the same seed, the same array
    assert np.array_equal(P, permutation_indices(37, 5, np.random.default_rng(11)))
    assert np.array_equal(P[0], np.random.default_rng(11).permutation(37))      # row b is rng.permutation(N)
    assert not np.array_equal(P, permutation_indices(37, 5, 12))
    assert len({tuple(r) for r in P}) == 5
    rng = np.random.default_rng(3)
    a, b = permutation_indices(9, 2, rng), permutation_indices(9, 2, rng)       # a Generator is drawn from, not copied
    assert not np.array_equal(a, b)
    assert permutation_indices(4, 0).shape == (0, 4)
    assert np.array_equal(permutation_indices(1, 3), np.zeros((3, 1), dtype=np.int64))
    with pytest.raises(ValueError):
        permutation_indices(0, 3)


def test_pvalue_formula():
    nan = np.nan
    #                 k = 0: plain   1: ties   2: a NaN   3: all below   4: all above
    null = np.array([[0.1, 2.0, 1.0, 0.0, 9.0],
                     [0.5, 1.0, nan, 0.1, 8.0],
                     [0.9, 2.0, 3.0, 0.2, 7.0],
                     [0.3, 3.0, 0.5, 0.3, 6.0]])
    observed = np.array([0.4, 2.0, 2.0, 5.0, 1.0])
    pv = permutation_pvalues(observed, null)
    # k = 0: 0.5, 0.9 >= 0.4 -> 3 / 5; k = 1: the ties 2.0, 2.0 and 3.0 count -> 4 / 5; k = 2: three replicates
    # have a value, one of them >= 2 -> 2 / 4; k = 3: none -> 1 / 5, never 0; k = 4: all -> 5 / 5
    assert np.array_equal(pv, [3 / 5, 4 / 5, 2 / 4, 1 / 5, 5 / 5])
    # a skipped replicate (a row of NaN) counts on neither side
    skipped = np.vstack([null, np.full((1, 5), nan)])
    assert np.array_equal(permutation_pvalues(observed, skipped), pv)
    # one component, 19 replicates all below: 1 / 20
    assert permutation_pvalues([3.0], np.linspace(0, 1, 19)[:, None])[0] == 1 / 20
    # a component no replicate reached, or that the observed fit lacks: NaN, not a number that looks like a result
    none = null.copy()
    none[:, 0] = nan
    out = permutation_pvalues(np.array([0.4, nan, 2.0, 5.0, 1.0]), none)
    assert np.isnan(out[0]) and np.isnan(out[1]) and np.array_equal(out[2:], pv[2:])
    assert permutation_pvalues(2.0, np.array([1.0, 2.0, 3.0])).shape == (1,)


def test_sharded_rows_need_perms():
    """A rank that holds part of the rows cannot draw for the others: it passes its own permutations."""
    from types import SimpleNamespace
    from ppls_amd import permutation_PPLS
    shard = SimpleNamespace(n_local=50, n_total=120)
    fit = dict(B=np.array([1.2]), sig=np.ones((1, 4)), Other_output=dict(Loglikelihoods=np.array([-3.0])))
    with pytest.raises(ValueError, match="perms"):
        permutation_PPLS(fit, None, None, 3, ctx=shard)
    with pytest.raises(ValueError, match="perms"):
        permutation_PPLS(fit, None, None, ctx=shard, perms=np.zeros((3, 49), dtype=np.int64))
    with pytest.raises(ValueError, match="no component"):
        permutation_PPLS(dict(B=np.zeros(0)), None, None, ctx=shard)


def test_entry_points_are_declared():
    import os
    from conftest import ROOT
    from ppls_amd import _lib
    with open(os.path.join(ROOT, "include", "ppls.h")) as f:
        assert "int ppls_xprod_permute(ppls_ctx* dst, ppls_ctx* src, const int64_t* perm" in f.read()
    with open(os.path.join(ROOT, "include", "ppls_debug.h")) as f:
        assert "int ppls_xgram_permuted(ppls_ctx* ctx, int nsplit, const int64_t* perm, double* C" in f.read()
    for name in ("ppls_xprod_permute", "ppls_xgram_permuted", "ppls_xperm_occupancy"):
        assert name in _lib.SIGNATURES
