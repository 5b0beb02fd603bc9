"""The sweep matrix's error bar (tests/sweep_bar.py) is neither vacuous nor too tight -- no GPU.

For every shape and row count of tests/test_gpu_sweep_matrix.py (R subsampled):
  * the same statistics in plain fp64 numpy, columns and rows visited in a shuffled order, lie
    within the bar (a correct kernel passes whatever its summation order);
  * four seeded defects in that fp64 computation each leave it, on the statistics alone:
      drop   one row left out of the sums;
      clamp  the last column pair of X that holds data (the end of the split sweep's padded row)
             holds the previous pair's values (the row-end clamp of the LDS copy gone wrong);
      stale  one row's a = x W taken from the previous row (a ring slot read before it landed;
             needs two rows);
      swap   beta and gamma exchanged.
"""
import zlib

import numpy as np
import pytest

import sweep_bar as sb

DEFECTS = ("drop", "clamp", "stale", "swap")


def fp64_stats(X, Y, th, seed, defect=None):
    """[SX, SY, G, mu] of one sweep in fp64, in a shuffled visiting order, optionally defective."""
    rng = np.random.default_rng(seed)
    n, p = X.shape
    q = Y.shape[1]
    al, be, ga, de = sb.coefficients(th)
    W, C = np.asarray(th["W"]), np.asarray(th["C"])
    if defect == "clamp":   # the pair (ldx - 2, ldx - 1) <- the pair before it
        ldx = (p + 1) & ~1   # the split sweep's padded width: its last pair holds data
        Xp = np.zeros((n, ldx))
        Xp[:, :p] = X
        Xp[:, ldx - 2:] = Xp[:, ldx - 4:ldx - 2]
        X = Xp[:, :p]
    px, py, pr = rng.permutation(p), rng.permutation(q), rng.permutation(n)
    a, b = X[:, px] @ W[px], Y[:, py] @ C[py]
    if defect == "stale":
        k = int(rng.integers(1, n))
        a[k] = a[k - 1]
    if defect == "swap":
        be, ga = ga, be
    mu_T, mu_U = a * al + b * be, a * ga + b * de
    if defect == "drop":
        pr = pr[pr != int(rng.integers(0, n))]
    z = np.hstack([a, b])[pr]
    return X[pr].T @ mu_T[pr], Y[pr].T @ mu_U[pr], z.T @ z, np.hstack([mu_T, mu_U])


def _inside_and_outside(label, p, q, r, ldx, ldy, rows, f32=False):
    worst = 0.0
    for n in rows:
        seed = zlib.crc32(f"{label}/{r}/{n}".encode())
        X, Y, th = sb.sweep_problem(n, p, q, r, seed)
        if f32:   # the data as fp32 storage holds them
            X, Y = (M.astype(np.float32).astype(np.float64) for M in (X, Y))
        ref = sb.Reference(X, Y, th, ldx, ldy)
        rat = ref.ratios(*fp64_stats(X, Y, th, seed + 1))
        worst = max(worst, *rat.values())
        assert max(rat.values()) <= 1.0, (label, r, n, rat)
        for d in DEFECTS:
            if d == "stale" and n < 2:
                continue
            rat = ref.ratios(*fp64_stats(X, Y, th, seed + 1, defect=d)[:3])
            assert max(rat.values()) > 1.0, (label, r, n, d, rat)
    print(f"{label} r={r}: worst fp64 err/bar {worst:.3g}")


CASES = [(s, r) for s in sb.SHAPES for r in sorted({1, 3, sb.RMAX_OF[s]})]


@pytest.mark.parametrize("shape,r", CASES, ids=[f"{s}-r{r}" for s, r in CASES])
def test_fp64_inside_bar_and_defects_outside(shape, r):
    p, q = sb.shape_pq(shape, r)
    _inside_and_outside(shape, p, q, r, sb.padded_width(p), sb.padded_width(q), [n for n, _ in sb.ROWS])


PANEL_CASES = [(s, r, f32) for s in sb.PANEL_SHAPES for r in (1, 16) for f32 in (False, True)]


@pytest.mark.parametrize("shape,r,f32", PANEL_CASES,
                         ids=[f"{s}-r{r}-{'fp32' if f else 'fp64'}" for s, r, f in PANEL_CASES])
def test_fp64_inside_bar_and_defects_outside_panel(shape, r, f32):
    p, q = sb.panel_pq(shape, r)
    _inside_and_outside(f"panel {shape}", p, q, r, sb.padded_width(p, f32), sb.padded_width(q, f32),
                        sb.PANEL_ROWS, f32)


def test_split_table_is_the_dispatchers_name_set():
    """The GPU matrix's literal name table against its restatement of the dispatcher's rules: every
    (shape, r, options) entry is what the rules give at that shape, and the table holds all 60
    names the rules can produce (the GPU test then asserts each name against the library)."""
    import test_gpu_sweep_matrix as m
    for shape, r in m.SPLIT_CASES:
        p, q = sb.shape_pq(shape, r)
        ldx, ldy = sb.padded_width(p), sb.padded_width(q)
        for rp, pipe, name in m.split_options(shape, r):
            assert m.dispatch_name(r, ldx, ldy, rp, pipe) == name, (shape, r, rp, pipe)
    table = {nm for s, r in m.SPLIT_CASES for _, _, nm in m.split_options(s, r)}
    assert table == m.dispatchable_names() and len(table) == 60
