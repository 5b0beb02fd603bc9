"""The finalize bars mean something (tests/finalize_bar.py; no GPU).

Plain fp64 results -- numpy's SVD polar factor, an fp64 transliteration of Cholesky-QR2 with a small
SVD, the library's host finalize for the scalars -- lie inside every bar at every shape of the GPU
matrix, so no bar is too tight; seeded defects of the kinds a kernel could have lie outside at
least one, so no bar is too loose to see them; and the inputs that are meant to select a polar path
sit clear of the kernel's thresholds.  The long-double reference is checked against itself.
"""
import ctypes as ct
import zlib

import numpy as np
import pytest

import finalize_bar as fb

LD = fb.LD
PATH_R = (1, 2, 5, 8, 10)


def _seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode())


def _svd_polar(S):
    Uu, _, Vt = np.linalg.svd(S, full_matrices=False)
    return Uu @ Vt


def _cholqr(S, passes, drop=None):
    """Cholesky-QR1 or -QR2 + the small polar factor by an SVD, in fp64; drop = (i0, i1): those rows
    are left out of the first Gram (a team member whose partial is lost)."""
    rows = np.ones(S.shape[0], dtype=bool)
    if drop:
        rows[drop[0]:drop[1]] = False
    R = np.linalg.cholesky(S[rows].T @ S[rows]).T
    Q = np.linalg.solve(R.T, S.T).T
    if passes == 2:
        R2 = np.linalg.cholesky(Q.T @ Q).T
        Q = np.linalg.solve(R2.T, Q.T).T
        R = R2 @ R
    return Q @ _svd_polar(R)


def _rows_of_matrix():
    """(m, r) of every polar block of the GPU matrix."""
    out = set()
    for r in PATH_R:
        for p, q, *_ in fb.GEOMETRY.values():
            out.update({(p, r), (max(q, r), r)})
        out.add((fb.unstaged_p(r), r))
    for r in range(1, 11):
        out.update({(9, r), (12, r)} if r <= 9 else {(12, r)})
    out.add((fb.TEAM_UNSTAGED[0], 10))
    for r in (11, 13, 16):
        out.update({(r + 3, r), (500, r)})
    return sorted(x for x in out if x[0] >= x[1])


ROWS = _rows_of_matrix()


# ---------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("kappa", [3.0, 1e4, 1e10, 1e13])
def test_reference_is_a_polar_factor(kappa):
    """Q_ref has orthonormal columns and Q_ref'S is symmetric, both to long-double rounding: 2^-11 of
    what an fp64 result can reach."""
    for m, r in ((9, 2), (500, 5), (2053, 10), (40, 16)):
        S = fb.with_condition(np.random.default_rng(_seed("ref", m, r, kappa)), m, r, kappa)
        ref = fb.PolarRef(S)
        got, pos = ref.measure(ref.Q)
        assert pos
        assert got["orth"] < 64 * r * LD(2.0) ** -64, (m, r, got)
        assert got["sym"] < 64 * r * LD(2.0) ** -64 * ref.normS * max(1.0, min(kappa, 1e3)), (m, r, got)
        bars = ref.bars()   # and its own error is 2^-11 of the fp64 bars: a thousandth is room enough
        assert got["orth"] < bars["orth"] / 1000 and got["sym"] < bars["sym"] / 1000
        assert abs(ref.kappa2 / kappa - 1) < 1e-3


def test_reference_qr_sign():
    S = fb.with_condition(np.random.default_rng(5), 30, 3, 10.0)
    for sg in (1.0, -1.0):
        ref = fb.PolarRef(S * sg, "QR")
        H = ref.Q.T @ ref.S
        assert H[0, 0] > 0 and fb.fro(np.tril(H, -1)) < 1e-17 * ref.normS
        Qn = np.linalg.qr(S * sg)[0]
        Qn = Qn * np.sign(Qn[:, 0] @ (S[:, 0] * sg))
        assert np.abs(Qn - np.asarray(ref.Q, dtype=np.float64)).max() < 1e-14


# ---------------------------------------------------------------------------- fp64 lies inside
@pytest.mark.parametrize("m,r", ROWS, ids=[f"{m}x{r}" for m, r in ROWS])
def test_fp64_polar_inside(m, r):
    worst = {}
    for path in ("fast", "qr2", "fb10", "fb13"):
        if r == 1 and path != "fast":
            continue
        bound = fb.polar1_bound(r)
        S = fb.path_input(np.random.default_rng(_seed(m, r, path)), m, r, path, bound)
        ref = fb.PolarRef(S)
        cands = {"svd": _svd_polar(S)}
        if path in ("fast", "qr2"):
            cands["cholqr2"] = _cholqr(S, 2)
        if path == "fast":
            assert ref.kF <= 0.5 * bound, (ref.kF, bound)
            cands["cholqr1"] = _cholqr(S, 1)
        elif path == "qr2":
            assert ref.kF >= 2 * bound and ref.kappa2 <= 1e5 * (1 + 1e-6), (ref.kF, ref.kappa2)
        else:   # Cholesky-QR2 must refuse: a pivot fails or Q1'Q1 is off I by far more than 0.1
            assert abs(ref.kappa2 / (1e10 if path == "fb10" else 1e13) - 1) < 1e-2
            try:
                R1 = np.linalg.cholesky(S.T @ S).T
                Q1 = np.linalg.solve(R1.T, S.T).T
                # (sigma_r^2 lies below the Gram's rounding: the last diagonal entry is noise, not near 1)
                assert np.abs(Q1.T @ Q1 - np.eye(r)).max() > 5 * 0.1
            except np.linalg.LinAlgError:
                pass
        for name, Q in cands.items():
            rat, pos = ref.ratios(Q, fast=(name == "cholqr1"))
            assert pos and max(rat.values()) <= 1.0, (path, name, rat)
            for k, v in rat.items():
                worst[k] = max(worst.get(k, 0.0), v)
        if m <= 600:
            refq = fb.PolarRef(S, "QR")
            Qn = np.linalg.qr(S)[0]
            Qn = Qn * np.sign(Qn[:, 0] @ S[:, 0])
            rat, pos = refq.ratios(Qn)
            assert pos and max(rat.values()) <= 1.0, (path, "qr", rat)
    print(f"{m}x{r}: worst fp64 err/bar {worst}")


@pytest.mark.parametrize("m,r", [(9, 2), (253, 5), (2053, 10)])
def test_gram_and_v_bars_hold_for_fp64(m, r):
    rng = np.random.default_rng(_seed("gram", m, r))
    Q = _svd_polar(rng.standard_normal((m, r)))
    assert fb.gram_ratio(Q.T @ Q, Q) <= 1.0
    acc = np.zeros((r, r))
    for i in range(m):   # a row-by-row sum, the worst order
        acc += np.outer(Q[i], Q[i])
    assert fb.gram_ratio(acc, Q) <= 1.0
    V = np.linalg.qr(rng.standard_normal((r, r)))[0]
    assert fb.v_ratio(V) <= 1.0 and fb.v_ratio(np.eye(r)) == 0.0


# ---------------------------------------------------------------------------- seeded defects lie outside
def _well(m, r, seed):
    return fb.with_condition(np.random.default_rng(seed), m, r, 3.0)


@pytest.mark.parametrize("m,r", [(9, 2), (253, 5), (2053, 10), (500, 1)])
def test_defect_row_from_neighbour(m, r):
    S = _well(m, r, _seed("row", m, r))
    ref = fb.PolarRef(S)
    Q = _svd_polar(S)
    Q[m // 2] = Q[m // 2 + 1]
    rat, _ = ref.ratios(Q)
    assert max(rat.values()) > 1.0, rat


@pytest.mark.parametrize("m,r,K", [(253, 5, 4), (2053, 10, 32), (2053, 1, 32)])
def test_defect_member_rows_dropped(m, r, K):
    """One team member's partial missing from S'S on the one-pass path (the second Gram of
    Cholesky-QR2 would repair it, so the fast path is where it shows)."""
    S = _well(m, r, _seed("drop", m, r))
    ref = fb.PolarRef(S)
    k = K - 2
    Q = _cholqr(S, 1, drop=(m * k // K, m * (k + 1) // K))
    rat, _ = ref.ratios(Q, fast=True)
    assert max(rat.values()) > 1.0, rat


@pytest.mark.parametrize("m,r", [(9, 2), (253, 5), (2053, 10)])
def test_defect_rotation_1e11(m, r):
    S = _well(m, r, _seed("rot", m, r))
    ref = fb.PolarRef(S)
    Q = np.asarray(ref.Q, dtype=LD).copy()
    a = LD(1e-11)
    c, s = np.cos(a), np.sin(a)
    Q[:, 0], Q[:, 1] = c * Q[:, 0] - s * Q[:, 1], s * Q[:, 0] + c * Q[:, 1]
    rat, _ = ref.ratios(Q)
    assert max(rat["orth"], rat["orth_max"]) <= 1.0 and rat["sym_max"] > 1.0, rat
    assert max(rat["dist"], rat["dist_max"]) > 1.0 or m > 1000, rat   # (entries of Q shrink as 1 / sqrt(m))
    refq = fb.PolarRef(S, "QR")
    Q = np.asarray(refq.Q, dtype=LD).copy()
    Q[:, 0], Q[:, 1] = c * Q[:, 0] - s * Q[:, 1], s * Q[:, 0] + c * Q[:, 1]
    rat, _ = refq.ratios(Q)
    assert rat["sym_max"] > 1.0, rat


@pytest.mark.parametrize("r", [2, 7, 10])
def test_defect_v_not_reorthonormalised(r):
    rng = np.random.default_rng(r)
    V = np.linalg.qr(rng.standard_normal((r, r)))[0]
    assert fb.v_ratio(V) <= 1.0
    assert fb.v_ratio(V + 1e-6 * rng.standard_normal((r, r))) > 1.0


def test_defect_padding_and_gram():
    rng = np.random.default_rng(3)
    Q = _svd_polar(rng.standard_normal((253, 5)))
    G = Q.T @ Q
    G[1, 3] += 1e-13   # a Gram that misses one row pair of one member by that much
    assert fb.gram_ratio(G, Q) > 1.0


# ---------------------------------------------------------------------------- the scalar block
def _host_finalize(pr, r):
    from ppls_amd import _lib
    from ppls_amd._lib import Expect, Theta, dptr
    L = _lib.lib()
    th = Theta(**pr["th"])
    nx = Theta.empty(pr["p"], pr["q"], r)
    ex = Expect(r)
    t, n, e = th.struct(), nx.struct(), ex.struct()
    n.W = n.C = None   # scalars only
    ll = np.zeros(1)
    G = np.asfortranarray(pr["G"])
    rc = L.ppls_finalize_host(None, None, dptr(G), pr["ssqX"], pr["ssqY"], pr["N"], pr["p"], pr["q"], r, ct.byref(t),
                              0, ct.byref(n), ct.byref(e), dptr(ll))
    assert rc == 0
    coef = np.zeros(4 * r)
    assert L.ppls_mu_coefficients(ct.byref(t), r, dptr(coef)) == 0
    nx.pull(n)
    ncoef = np.zeros(4 * r)
    n2 = nx.struct()
    assert L.ppls_mu_coefficients(ct.byref(n2), r, dptr(ncoef)) == 0
    got = dict(Ctt=ex.Ctt, Cuu=ex.Cuu, Cut=ex.Cut, Cee=[e.Cee], Cff=[e.Cff], Chh=ex.Chh.ravel(order="F"),
               loglik=ll, B=nx.B, sigT=nx.sigT, sigE=[n.sigE], sigF=[n.sigF], sigH=[n.sigH],
               alpha=ncoef[:r], beta=ncoef[r:2 * r], gamma=ncoef[2 * r:3 * r], delta=ncoef[3 * r:])
    return got, coef.reshape(4, r)


def scalar_ref(pr, coef):
    th = pr["th"]
    return fb.ScalarRef(pr["G"], pr["WtW"], pr["CtC"], pr["ssqX"], pr["ssqY"], pr["N"], pr["p"], pr["q"],
                        np.diag(th["B"]), np.diag(th["sigT"]), th["sigE"], th["sigF"], th["sigH"], coef)


SCALAR_CASES = [(9, 12, r) for r in range(1, 10)] + [(500, 390, r) for r in (1, 5, 8, 10, 11, 13, 16)] + [(20, 16, 16)]


@pytest.mark.parametrize("p,q,r", SCALAR_CASES, ids=[f"{p}x{q}-r{r}" for p, q, r in SCALAR_CASES])
def test_host_finalize_scalars_inside(p, q, r):
    q = max(q, r)
    pr = fb.scalar_problem(p, q, r, _seed("scal", p, q, r))
    got, coef = _host_finalize(pr, r)
    rat = scalar_ref(pr, coef).ratios(got)
    print(f"scalars {p}x{q} r={r}: fp64 err/bar {rat}")
    assert max(rat.values()) <= 1.0, rat


@pytest.mark.parametrize("r", [2, 3, 7, 9, 10, 13])
def test_defect_scalars(r):
    p, q = 40, max(30, r)
    pr = fb.scalar_problem(p, q, r, _seed("scaldef", r))
    got, coef = _host_finalize(pr, r)
    ref = scalar_ref(pr, coef)
    assert max(ref.ratios(got).values()) <= 1.0
    # one Chh pair transposed (the Gram handed in is not symmetric, so Chh is not either)
    Chh = np.array(got["Chh"]).reshape(r, r).T.copy()
    assert Chh[0, 1] != Chh[1, 0]
    Chh[0, 1], Chh[1, 0] = Chh[1, 0], Chh[0, 1]
    assert ref.ratios(dict(Chh=Chh.ravel(order="F")))["Chh"] > 1.0
    # one off-diagonal entry of W'W taken as 0
    pr2 = dict(pr, th=pr["th"])
    bad = dict(pr)
    bad["WtW"] = pr["WtW"].copy()
    bad["WtW"][1, 0] = 0.0
    assert pr["WtW"][1, 0] != 0.0
    shifted = scalar_ref(bad, coef)   # what a kernel that dropped the entry would compute
    Cee_bad = np.asarray(shifted.out["Cee"][0], dtype=np.float64)
    rat = ref.ratios(dict(Cee=Cee_bad))
    assert rat["Cee"] > 1.0, rat
    del pr2


# ---------------------------------------------------------------------------- the fused Gram
@pytest.mark.parametrize("p,q,r", [(33, 7, 3), (2, 700, 2), (300, 260, 8), (40, 1100, 5)])
def test_fused_gram_bar(p, q, r):
    q = max(q, r)
    rng = np.random.default_rng(_seed("fg", p, q, r))
    ldx, ldy = fb.padded_width(p), fb.padded_width(q)
    W, C = rng.standard_normal((p, r)), rng.standard_normal((q, r))
    M = rng.standard_normal((ldx + ldy, 2 * r))
    Bp = np.zeros((ldx + ldy, 2 * r))
    Bp[:p, :r] = W
    Bp[ldx:ldx + q, r:] = C
    full = Bp.T @ M
    G = np.triu(full) + np.triu(full, 1).T
    assert fb.fused_gram_ratio(G, W, C, M, ldx, ldy) <= 1.0
    bad = G.copy()
    bad[0, r], bad[0, r + 1 if r > 1 else 0] = G[0, r + 1 if r > 1 else 0], G[0, r]   # swapped with its neighbour
    assert fb.fused_gram_ratio(bad, W, C, M, ldx, ldy) > 1.0
