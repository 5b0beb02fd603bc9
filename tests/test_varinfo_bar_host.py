"""Host side of the observed-information kernel's error bar: no GPU.

The a-priori bar of tests/varinfo_bar.py is shown to admit a plain fp64 evaluation in the kernel's
order, and to reject three seeded defects: k1 applied to one of the two cross terms only, x and w
indexed transposed in one term, and the diagonal term added instead of subtracted.
"""
import numpy as np
import pytest

from varinfo_bar import K_J, bars, inside, kernel_order, make_case, reference

SHAPES = [(1, 0, 1), (2, 0, 1), (2, 38, 3), (37, 0, 3), (37, 38, 16), (65, 38, 3), (129, 0, 1)]


@pytest.mark.parametrize("p,off,a", SHAPES)
def test_kernel_order_lies_inside_the_bar(p, off, a):
    c = make_case(p, off, a)
    ok, worst = inside(kernel_order(c), reference(c)[0], bars(c)[0])
    print(f"p={p} off={off} a={a}: max err / bar {worst:.3g} (K_J = {K_J})")
    assert ok


@pytest.mark.parametrize("p,off,a", [s for s in SHAPES if s[0] > 1])
def test_seeded_defects_lie_outside_the_bar(p, off, a):
    c = make_case(p, off, a)
    ref, bar = reference(c)[0], bars(c)[0]
    assert inside(kernel_order(c), ref, bar)[0]
    for defect in ("one_k1", "transposed", "diag_sign"):
        assert not inside(kernel_order(c, defect), ref, bar)[0], defect


def test_p1_defects():
    """p = 1: a transposition is no defect there; the other two are."""
    c = make_case(1, 0, 3)
    ref, bar = reference(c)[0], bars(c)[0]
    assert not inside(kernel_order(c, "one_k1"), ref, bar)[0]
    assert not inside(kernel_order(c, "diag_sign"), ref, bar)[0]


def test_reference_matches_the_literal_form():
    """The long-double reference restates variances.PPLS_simult's :844-851 (oracle order) -- checked
    against a dense fp64 evaluation of those lines to fp64 accuracy."""
    c = make_case(37, 0, 3)
    J, E, S = reference(c)
    p, N, s4 = c["p"], c["N"], c["s4"]
    for i in range(3):
        x, w = c["cxt"][:, [i]], c["w"][:, [i]]
        ctt, k1, k2 = c["ctt"][i], c["k1"][i], c["k2"][i]
        sse = (ctt * c["g"] - x * k1 @ w.T - w * k1 @ x.T + w * k2 @ w.T) / s4 / N
        d = x - w * ctt
        assert np.allclose(np.asarray(E[i], dtype=float), sse, rtol=1e-12, atol=0)
        assert np.allclose(np.asarray(J[i], dtype=float), sse - np.eye(p) * c["bstar"][i], rtol=1e-12, atol=1e-12)
        assert np.allclose(np.asarray(S[i], dtype=float), d @ d.T / s4, rtol=1e-9, atol=1e-9)
