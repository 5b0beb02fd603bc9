"""The a-priori bar of the 'o2m_xprod' pass (tests/o2m_bar.py) on the CPU: plain fp64 in the kernel's
summation order lies inside it and every seeded defect outside; and the numpy restatement of the
deflated one-pass operator with Lanczos equals the oracle's o2m values on the explicitly deflated data
(the tolerance of tests/test_o2m_host.py).  CPU only."""
import numpy as np
import pytest

import o2m_bar as ob
from conftest import make_problem
from oracle import ppls_oracle as O

SHAPES = [dict(rows=30, L=20, col0=30, ld=52), dict(rows=25, L=18, row0=18, ld=44), dict(rows=31, L=21, col0=32, ld=54),
          dict(rows=40, L=129, ld=140), dict(rows=257, L=127, col0=2, ld=130), dict(rows=3, L=1), dict(rows=1, L=2),
          dict(rows=70, L=300, ld=310)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s.values()))
@pytest.mark.parametrize("d_zero", [False, True], ids=["d", "d0"])
def test_fp64_in_kernel_order_is_inside_the_bar(shape, d_zero):
    case = ob.make_case(d_zero=d_zero, **shape)
    ref_u, ref_z = ob.reference(case)
    bar_u, bar_z = ob.bars(case)
    u, z = ob.model(case)
    assert ob.inside(u, ref_u, bar_u) <= 1.0
    assert ob.inside(z, ref_z, bar_z) <= 1.0


@pytest.mark.parametrize("defect,shape", [
    ("last_row", dict(rows=30, L=20, col0=30, ld=52)),
    ("tail_cols", dict(rows=40, L=129, ld=140)),
    ("tail_cols", dict(rows=70, L=300, ld=310)),
    ("no_d", dict(rows=25, L=18, row0=18, ld=44)),
    ("stride_L", dict(rows=31, L=21, col0=32, ld=54)),
    ("lost_partial", dict(rows=257, L=127, col0=2, ld=130)),
])
def test_seeded_defects_are_outside_the_bar(defect, shape):
    case = ob.make_case(**shape)
    ref_u, ref_z = ob.reference(case)
    bar_u, bar_z = ob.bars(case)
    u, z = ob.model(case, defect=defect)
    worst = max(ob.inside(u, ref_u, bar_u), ob.inside(z, ref_z, bar_z))
    assert worst > 1.0, (defect, worst)


WIDE = [dict(rows=70, L=600, ld=610), dict(rows=37, L=1100, col0=2, ld=1110)]
TWOPHASE = [dict(rows=70, L=300, ld=310), dict(rows=257, L=127, col0=2, ld=130), dict(rows=40, L=2100, ld=2110)]
OTHER_KINDS = [("wide", sh) for sh in WIDE] + [("twophase", sh) for sh in TWOPHASE]


@pytest.mark.parametrize("kind,shape", OTHER_KINDS, ids=lambda v: v if isinstance(v, str) else "x".join(str(x) for x in v.values()))
def test_wide_and_two_phase_orders_are_inside_the_bar_and_their_defects_outside(kind, shape):
    """The kernel for rows of more than 512 values (rows shared by four waves) and the two-phase path
    sum in other orders than the narrow fused kernel: the same bar holds for them and catches the same
    five seeded defects."""
    case = ob.make_case(**shape)
    ref_u, ref_z = ob.reference(case)
    bar_u, bar_z = ob.bars(case)
    u, z = ob.model(case, kind=kind)
    assert ob.inside(u, ref_u, bar_u) <= 1.0 and ob.inside(z, ref_z, bar_z) <= 1.0
    plan = ob.wide_plan if kind == "wide" else ob.twophase_plan
    assert plan(case["rows"], case["L"])[1 if kind == "twophase" else 2] >= 2        # several partials
    for defect in ("last_row", "tail_cols", "no_d", "stride_L", "lost_partial"):
        if defect == "tail_cols" and case["L"] % 128 == 0:
            continue
        u, z = ob.model(case, kind=kind, defect=defect)
        worst = max(ob.inside(u, ref_u, bar_u), ob.inside(z, ref_z, bar_z))
        assert worst > 1.0, (kind, defect, worst)


def test_fused_plan_has_several_workgroups_where_the_defect_needs_them():
    assert ob.fused_plan(257, 127)[2] >= 2
    assert ob.fused_plan(70, 300)[0] == 4


def test_compact_form_of_the_deflation_products():
    rng = np.random.default_rng(4)
    Lv = rng.standard_normal((12, 3))
    Lv *= np.array([1.0, 0.7, 1.3]) / np.linalg.norm(Lv, axis=0)   # not unit, not orthogonal
    Pl = np.eye(12)
    for j in range(3):
        Pl = (np.eye(12) - np.outer(Lv[:, j], Lv[:, j])) @ Pl
    assert np.abs(Pl.T @ Pl - (np.eye(12) - Lv @ ob.compact_T(Lv) @ Lv.T)).max() < 1e-12


def _align(g, ref):
    if float(g["W"] @ ref["W"]) < 0:
        g = dict(g, W=-g["W"], C=-g["C"])
    return g


@pytest.mark.parametrize("n,p,q", [(600, 25, 18), (600, 18, 25)])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_pass_operator_with_lanczos_equals_oracle_on_deflated_data(n, p, q, k):
    X, Y, _ = make_problem(n, p, q, 3, seed=11 + k)
    rng = np.random.default_rng(k)
    Wp = rng.standard_normal((p, k))
    Cp = rng.standard_normal((q, k))
    Wp /= np.linalg.norm(Wp, axis=0) if k else 1.0
    Cp /= np.linalg.norm(Cp, axis=0) if k else 1.0
    Xc, Yc = X.copy(), Y.copy()
    for j in range(k):
        Xc = Xc - np.outer(Xc @ Wp[:, j], Wp[:, j])
        Yc = Yc - np.outer(Yc @ Cp[:, j], Cp[:, j])
    ref = O.initial_guess_o2m(Xc, Yc)
    ldx = p + (p & 1) + 2                                  # a padded layout: zero columns between X's and Y's
    D = np.zeros((n, ldx + q + (q & 1)))
    D[:, :p], D[:, ldx:ldx + q] = X, Y
    g, info = ob.o2m_start_numpy(D.T @ D, n, p, q, ldx, Wp, Cp)
    assert info["side"] == (0 if q <= p else 1) and info["passes"] <= 32
    assert g["W"][np.argmax(np.abs(g["W"]))] > 0
    g = _align(g, ref)
    for key in ("W", "C"):
        assert np.abs(g[key] - np.ravel(ref[key])).max() < 1e-9, key
    for key in ("B", "sigE", "sigF", "sigH", "sigT"):
        assert abs(g[key] - ref[key]) <= 1e-9 * max(1.0, abs(ref[key])), (key, g[key], ref[key])
