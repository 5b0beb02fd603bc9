"""The device finalize alone, every instantiation, against long double (tests/finalize_bar.py).

``Context.finalize_stats`` runs one production finalize on statistics handed in, through the function
the EM loop uses and under the context's options, so teams, LDS staging and mode bits are
production's.  Every case first asserts the launch plan (``finalize_plan``: templated or runtime-r
kernel, workgroups per factor, staged or not) and the form each polar block reports it took (1
Cholesky-QR1, 2 Cholesky-QR2, 3 Householder, 4 QR type), then the bars of finalize_bar.py: (a)
orthogonality, (b) distance to the long-double factor, (c) the polar property, (d) padding rows
exactly 0, (e) the Gram of the new loadings, (f) the carried Jacobi V; the scalar block's moments,
log-likelihood and next scalars against k u times their absolute evaluation; the Gram the scalar
block forms from M = S B against B'M.  Data are loaded only to give p, q, the padded widths, the
sums of squares and N: three rows are enough, the statistics are handed in.

Shapes (finalize_bar.GEOMETRY): one block staged at (9, 12) and (500, 390); one block unstaged at
the smallest p over the budget the plan reports; teams at team_rows = 64 with p = 253 (4 uneven
members, odd: one padding row) and p = 2053 (33 members asked, 32 given; 507 padding rows), q one
block or a team of 2; a team of 2 at the default team_rows whose members cannot stage at r = 10.
p = max(p, r) and q = max(q, r) where a fit needs ncol >= r.  team_rows accepts any positive count;
64 is the smallest at which the issue's 4 T - 3 rows still hold 10 components.

The cases team2 and team16 (the rows of team4 over 2 and 16 members) are here because they found a
defect: at R = 10, with both Cholesky factorisations of the polar run by one thread in registers, a
team of K > 1 members lost orthogonality in proportion to kappa (max|W'W - I| = 5.2e-13 at kappa_2 =
1e4 with K = 16, orth_max 5.19, where one block gave 0.0175 and r = 8, 9 gave 0.02 in any team).
R = 10 now takes the wave forms of the factorisations (PPLS_REG_RMAX 9), with which the same inputs
give 0.009 to 0.02 for K = 1, 2, 4, 16.

The last test asserts that every templated R, the runtime-r kernel, the four path codes, staged 0
and 1 and K = 1, 4, 32 each appeared in an asserted case, and prints the worst err / bar per
quantity and path.
"""
import ctypes as ct
import itertools
import zlib

import numpy as np
import pytest

import finalize_bar as fb

pytestmark = pytest.mark.gpu

PATH_R = (1, 2, 5, 8, 10)
DEFAULTS = dict(team_rows=0, polar1=1, polar1_kappa=0, exact_gram=1, vorth=8)
PATH_NAME = {1: "cholqr1", 2: "cholqr2", 3: "householder", 4: "qr"}

SEEN = dict(R=set(), generic=set(), code=set(), staged=set(), K=set())
WORST = {}     # (quantity, path name) -> worst err / bar
RAN = set()


def _seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode())


def _note(quantity, path, ratio):
    k = (quantity, path)
    WORST[k] = max(WORST.get(k, 0.0), float(ratio))


@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    c._shape = None
    yield c
    c.close()


def _restore(ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


def _load(ctx, p, q, XY=None):
    """Three rows of data for the shape (kept while the shape stays), or the given rows."""
    if XY is not None:
        ctx.set_data(*XY)
        ctx._shape = None
        return
    if ctx._shape != (p, q):
        rng = np.random.default_rng(_seed("data", p, q))
        ctx.set_data(rng.standard_normal((3, p)), rng.standard_normal((3, q)))
        ctx._shape = (p, q)


def _plain_theta(p, q, r):
    from ppls_amd import Theta
    return Theta(W=np.eye(p, r), C=np.eye(q, r), B=np.linspace(1.2, 0.7, r), sigE=2.0, sigF=1.7, sigH=0.9,
                 sigT=np.linspace(1.1, 0.6, r))


def _plain_gram(r):
    return np.eye(2 * r) * 3.0 + 0.5


def _expect_plan(ctx, r, typ, p, q, team_rows, generic=False):
    """The plan the launcher must report for the shape, restated: asserts it and returns it."""
    plan = ctx.finalize_plan(r, 1 if typ == "QR" else 0)
    if generic:
        assert plan["templated"] == 0 and (plan["KX"], plan["KY"], plan["staged"]) == (1, 1, 0), plan
        SEEN["generic"].add(r)
        SEEN["K"].add(1)
        return plan
    assert plan["templated"] == 1, plan
    assert 100 * 1024 <= plan["stage_budget"] <= fb.STAGE_MAX, plan
    tr = team_rows if team_rows > 0 else 2048
    K = lambda rows: 1 if typ == "QR" else min(32, max(1, -(-rows // tr)))   # noqa: E731
    KX, KY = K(p), K(q)
    stage = r * max(-(-p // KX), -(-q // KY)) * 8
    staged = int(stage <= plan["stage_budget"] and typ != "QR")
    assert (plan["KX"], plan["KY"], plan["staged"]) == (KX, KY, staged), (plan, KX, KY, staged)
    SEEN["R"].add(r)
    SEEN["staged"].add(staged)
    SEEN["K"].update({KX, KY})
    return plan


def _check_polar(res, refs, p, q, codes, label, exact_gram=True):
    """Bars (a) to (f) of both factors of one launch; codes: the expected path codes (W, C)."""
    assert res["path"] == codes, f"{label}: path codes {res['path']}, expected {codes}"
    SEEN["code"].update(codes)
    for which, rows, ref, code, G, V in (("W", p, refs[0], codes[0], res["gram_nxt"][0], res["vstate"][0]),
                                        ("C", q, refs[1], codes[1], res["gram_nxt"][1], res["vstate"][1])):
        if ref is None:
            continue
        Q = res[which]
        name = PATH_NAME[code]
        assert np.array_equal(Q[rows:], np.zeros_like(Q[rows:])), f"{label} {which}: padding rows not 0"   # (d)
        rat, pos = ref.ratios(Q[:rows], fast=(code == 1))
        for k, v in rat.items():
            _note(k, name, v)
        print(f"{label} {which} ({name}): " + " ".join(f"{k} {v:.3g}" for k, v in rat.items()))
        assert pos and max(rat.values()) <= 1.0, f"{label} {which} ({name}): err / bar {rat}, positive {pos}"
        r = ref.r
        if r <= 10:   # (e); the runtime-r kernel keeps no Gram and no V
            if exact_gram:
                g = fb.gram_ratio(G, Q[:rows])
                _note("gram_nxt", name, g)
                assert g <= 1.0, f"{label} {which} ({name}): gram_nxt err / bar {g}"
            else:
                assert np.array_equal(G, np.eye(r)), f"{label} {which}: gram_nxt not I with exact_gram = 0"
            v = fb.v_ratio(V)   # (f)
            _note("vstate", name, v)
            assert v <= 1.0, f"{label} {which} ({name}): V'V - I err / bar {v}"


def _path_cases(r):
    """(name, path input, polar1, expected code)."""
    out = [("fast", "fast", 1, 1), ("polar1=0", "fast", 0, 2)]
    if r >= 2:
        out += [("qr2", "qr2", 1, 2), ("fallback 1e10", "fb10", 1, 3), ("fallback 1e13", "fb13", 1, 3)]
    return out


def _run_paths(ctx, geo, p, q, r, team_rows):
    p, q = max(p, r), max(q, r)
    _load(ctx, p, q)
    th = _plain_theta(p, q, r)
    bound = fb.polar1_bound(r)
    try:
        ctx.set_option("team_rows", team_rows)
        for name, kind, polar1, code in _path_cases(r):
            ctx.set_option("polar1", polar1)
            _expect_plan(ctx, r, "SVD", p, q, team_rows)
            SX = fb.path_input(np.random.default_rng(_seed(geo, "x", r, kind)), p, r, kind, bound)
            SY = fb.path_input(np.random.default_rng(_seed(geo, "y", r, kind)), q, r, kind, bound)
            refs = (fb.PolarRef(SX), fb.PolarRef(SY))
            res = ctx.finalize_stats(th, SX, SY, _plain_gram(r))
            assert res["status"] == 0, (geo, r, name, res["status"])
            _check_polar(res, refs, p, q, (code, code), f"{geo} {p}x{q} r={r} {name}")
            if name == "fast":
                first = (SX, SY, refs)
        ctx.set_option("polar1", 1)
        ctx.set_option("exact_gram", 0)   # the Gram of the new loadings taken as I: a team's pass 3 has no exchange
        res = ctx.finalize_stats(th, first[0], first[1], _plain_gram(r))
        assert res["status"] == 0
        _check_polar(res, first[2], p, q, (1, 1), f"{geo} {p}x{q} r={r} exact_gram=0", exact_gram=False)
    finally:
        _restore(ctx)
    RAN.add((geo, r))


# ---------------------------------------------------------------------------- paths by geometry
GEO_CASES = [(g, r) for g in fb.GEOMETRY for r in PATH_R]


@pytest.mark.parametrize("geo,r", GEO_CASES, ids=[f"{g}-r{r}" for g, r in GEO_CASES])
def test_paths_by_geometry(ctx, geo, r):
    p, q, team_rows, KX, KY = fb.GEOMETRY[geo]
    _load(ctx, max(p, r), max(q, r))
    ctx.set_option("team_rows", team_rows)
    plan = ctx.finalize_plan(r)
    _restore(ctx)
    assert (plan["KX"], plan["KY"], plan["staged"]) == (KX, KY, 1), plan   # the table's own K, written out
    _run_paths(ctx, geo, p, q, r, team_rows)


@pytest.mark.parametrize("r", PATH_R)
def test_paths_one_block_unstaged(ctx, r):
    """The smallest p one block cannot stage (r p 8 over the budget the plan reports), and one row less."""
    _load(ctx, max(9, r), max(12, r))
    budget = ctx.finalize_plan(r)["stage_budget"]
    p = fb.unstaged_p(r, budget)
    assert r * p * 8 > budget >= r * (p - 1) * 8
    big = 1 << 20
    try:
        ctx.set_option("team_rows", big)
        _load(ctx, p - 1, max(12, r))
        assert ctx.finalize_plan(r)["staged"] == 1
        _load(ctx, p, max(12, r))
        plan = ctx.finalize_plan(r)
        assert (plan["KX"], plan["KY"], plan["staged"]) == (1, 1, 0), plan
    finally:
        _restore(ctx)
    _run_paths(ctx, "unstaged", p, 12, r, big)


def test_team_unstaged_r10(ctx):
    p, q, team_rows, KX, KY = fb.TEAM_UNSTAGED
    _load(ctx, p, q)
    plan = ctx.finalize_plan(10)
    assert (plan["KX"], plan["KY"], plan["staged"]) == (KX, KY, 0), plan
    assert 10 * (p // 2) * 8 > plan["stage_budget"]
    _run_paths(ctx, "team-unstaged", p, q, 10, team_rows)


# ---------------------------------------------------------------------------- every instantiation
@pytest.mark.parametrize("r", range(1, 11))
def test_every_templated_r(ctx, r):
    _run_paths(ctx, "small", 9, 12, r, 0)


@pytest.mark.parametrize("p,q", [(20, 18), (500, 390)])
@pytest.mark.parametrize("r", [11, 13, 16])
def test_generic_kernel(ctx, r, p, q):
    _load(ctx, p, q)
    th = _plain_theta(p, q, r)
    _expect_plan(ctx, r, "SVD", p, q, 0, generic=True)
    for kind in ("fast", "qr2", "fb13"):
        SX = fb.path_input(np.random.default_rng(_seed("gen-x", p, r, kind)), p, r, kind, 40)
        SY = fb.path_input(np.random.default_rng(_seed("gen-y", q, r, kind)), q, r, kind, 40)
        res = ctx.finalize_stats(th, SX, SY, _plain_gram(r))
        assert res["status"] == 0
        _check_polar(res, (fb.PolarRef(SX), fb.PolarRef(SY)), p, q, (3, 3), f"generic {p}x{q} r={r} {kind}")


@pytest.mark.parametrize("p,q,team_rows", [(9, 12, 0), (500, 390, 64)])
@pytest.mark.parametrize("r", [1, 3, 10, 12])
def test_qr_type(ctx, r, p, q, team_rows):
    """type = "QR": one block per factor whatever team_rows says, nothing staged, code 4."""
    p, q = max(p, r), max(q, r)
    _load(ctx, p, q)
    th = _plain_theta(p, q, r)
    try:
        ctx.set_option("team_rows", team_rows)
        plan = _expect_plan(ctx, r, "QR", p, q, team_rows, generic=r > 10)
        assert (plan["KX"], plan["KY"], plan["staged"]) == (1, 1, 0)
        for kappa in (3.0, 1e6) if r > 1 else (1.0,):
            SX = fb.with_condition(np.random.default_rng(_seed("qr-x", p, r, kappa)), p, r, kappa)
            SY = -fb.with_condition(np.random.default_rng(_seed("qr-y", q, r, kappa)), q, r, kappa)
            res = ctx.finalize_stats(th, SX, SY, _plain_gram(r), type=1)
            assert res["status"] == 0
            _check_polar(res, (fb.PolarRef(SX, "QR"), fb.PolarRef(SY, "QR")), p, q, (4, 4), f"QR {p}x{q} r={r} {kappa}")
    finally:
        _restore(ctx)


@pytest.mark.parametrize("geo", ["mid", "team4x2"])
def test_zero_column_reports_rank_deficiency(ctx, geo):
    p, q, team_rows, _, _ = fb.GEOMETRY[geo]
    r = 3
    _load(ctx, p, q)
    try:
        ctx.set_option("team_rows", team_rows)
        SX = fb.with_condition(np.random.default_rng(1), p, r, 3.0)
        SX[:, 1] = 0.0
        SY = fb.with_condition(np.random.default_rng(2), q, r, 3.0)
        res = ctx.finalize_stats(_plain_theta(p, q, r), SX, SY, _plain_gram(r))   # returns cleanly
        assert res["status"] == -3, res["status"]
        assert res["path"] == (3, 1), res["path"]
        _check_polar(res, (None, fb.PolarRef(SY)), p, q, (3, 1), f"zero column {geo}")
        SX = fb.with_condition(np.random.default_rng(3), p, r, 3.0)
        ok = ctx.finalize_stats(_plain_theta(p, q, r), SX, SY, _plain_gram(r))   # the next call is clean again
        assert ok["status"] == 0 and ok["path"] == (1, 1)
    finally:
        _restore(ctx)


# ---------------------------------------------------------------------------- warm start and cadence
@pytest.mark.parametrize("geo", ["mid", "team4x2"])
@pytest.mark.parametrize("r", [1, 2, 7, 10])
def test_warm_start(ctx, geo, r):
    """The four V inputs of (f) under vorth in {1, 8} at iter 0, 8 (re-orthonormalising) and 3 (not, at
    vorth 8: only orthonormal V then).  The polar factor meets (a) to (c) for all of them."""
    p, q, team_rows, _, _ = fb.GEOMETRY[geo]
    _load(ctx, p, q)
    th = _plain_theta(p, q, r)
    rng = np.random.default_rng(_seed("warm", geo, r))
    bound = fb.polar1_bound(r)
    kinds = ("fast", "qr2") if r >= 2 else ("fast",)
    S = {k: (fb.path_input(rng, p, r, k, bound), fb.path_input(rng, q, r, k, bound)) for k in kinds}
    refs = {k: (fb.PolarRef(S[k][0]), fb.PolarRef(S[k][1])) for k in kinds}
    orthV = tuple(np.linalg.qr(rng.standard_normal((r, r)))[0] for _ in range(2))
    offV = tuple(v + 1e-6 * rng.standard_normal((r, r)) for v in orthV)
    assert r == 1 or min(fb.v_ratio(v) for v in offV) > 1.0
    try:
        ctx.set_option("team_rows", team_rows)
        for kind, vorth, it in itertools.product(kinds, (1, 8), (0, 8, 3)):
            ctx.set_option("vorth", vorth)
            code = 1 if kind == "fast" else 2
            prev = None
            for vname in ("identity", "previous", "random", "off"):
                if vname == "off" and it == 3:
                    continue
                V = {"identity": None, "previous": prev, "random": orthV, "off": offV}[vname]
                res = ctx.finalize_stats(th, S[kind][0], S[kind][1], _plain_gram(r), iter=it, vstate=V)
                assert res["status"] == 0
                _check_polar(res, refs[kind], p, q, (code, code), f"warm {geo} r={r} {kind} vorth={vorth} iter={it} V={vname}")
                prev = res["vstate"]
    finally:
        _restore(ctx)


# ---------------------------------------------------------------------------- the scalar block
def _device_inputs(ctx, th, r):
    """The sums of squares the context holds and the alpha..delta the library stages for theta."""
    from ppls_amd import _lib
    sx, sy = ct.c_double(), ct.c_double()
    ctx._chk(ctx._L.ppls_data_ssq(ctx.h, ct.byref(sx), ct.byref(sy)))
    coef = np.zeros(4 * r)
    t = th.struct()
    assert ctx._L.ppls_mu_coefficients(ct.byref(t), r, _lib.dptr(coef)) == 0
    return sx.value, sy.value, coef.reshape(4, r)


def _scalar_got(res):
    m = res["moments"]
    got = dict(Ctt=m.Ctt, Cuu=m.Cuu, Cut=m.Cut, Cee=[m.Cee], Cff=[m.Cff], Chh=m.Chh.ravel(order="F"),
               B=res["B"], sigT=res["sigT"], sigE=[res["sigE"]], sigF=[res["sigF"]], sigH=[res["sigH"]],
               alpha=res["alpha"], beta=res["beta"], gamma=res["gamma"], delta=res["delta"])
    if res["loglik"] is not None:
        got["loglik"] = [res["loglik"]]
    return got


SCALAR_R = tuple(range(1, 11)) + (11, 13, 16)


@pytest.mark.parametrize("p,q", [(9, 12), (500, 390)])
@pytest.mark.parametrize("r", SCALAR_R)
def test_scalar_block(ctx, r, p, q):
    from ppls_amd import Theta
    p, q = max(p, r), max(q, r)
    pr = fb.scalar_problem(p, q, r, _seed("scal", p, q, r))
    _load(ctx, p, q, (pr["X"], pr["Y"]))
    th = Theta(**pr["th"])
    ssqX, ssqY, coef = _device_inputs(ctx, th, r)
    t = pr["th"]
    ref = fb.ScalarRef(pr["G"], pr["WtW"], pr["CtC"], ssqX, ssqY, pr["N"], p, q, np.diag(t["B"]), np.diag(t["sigT"]),
                       t["sigE"], t["sigF"], t["sigH"], coef)
    rng = np.random.default_rng(r)
    SX, SY = fb.with_condition(rng, p, r, 3.0), fb.with_condition(rng, q, r, 3.0)
    _expect_plan(ctx, r, "SVD", p, q, 0, generic=r > 10)
    fam = "scalars templated" if r <= 10 else "scalars runtime-r"
    for gram in ("given", "own"):
        res = ctx.finalize_stats(th, SX, SY, pr["G"], iter=0,
                                 gram_cur=(pr["WtW"], pr["CtC"]) if gram == "given" else None)
        assert res["status"] == 0
        rat = ref.ratios(_scalar_got(res))
        for k, v in rat.items():
            _note(k, fam, v)
        print(f"scalars {p}x{q} r={r} gram {gram}: err/bar {rat}")
        assert max(rat.values()) <= 1.0, f"scalars {p}x{q} r={r} gram_cur {gram}: err / bar {rat}"
        assert np.array_equal(res["gram_stats"], pr["G"])   # no cross-product M: the Gram slot is left alone


# ---------------------------------------------------------------------------- the fused Gram
FUSED_SHAPES = [(33, 7), (2, 700), (300, 260), (40, 1100)]   # ldy = 260 > 256 threads; 1100: a second batch at r <= 5


@pytest.mark.parametrize("p,q", FUSED_SHAPES)
@pytest.mark.parametrize("r", range(1, 9))
def test_fused_gram(ctx, r, p, q):
    from ppls_amd import Theta
    p, q = max(p, r), max(q, r)
    pr = fb.scalar_problem(p, q, r, _seed("fused", p, q, r))
    _load(ctx, p, q, (pr["X"], pr["Y"]))
    th = Theta(**pr["th"])
    ldx, ldy = fb.padded_width(p), fb.padded_width(q)
    rng = np.random.default_rng(_seed("M", p, q, r))
    M = rng.standard_normal((ldx + ldy, 2 * r)) * 10.0 ** rng.uniform(-1, 1, (1, 2 * r))   # padding rows too
    SX, SY = fb.with_condition(rng, p, r, 3.0), fb.with_condition(rng, q, r, 3.0)
    res = ctx.finalize_stats(th, SX, SY, np.full((2 * r, 2 * r), np.nan), iter=0, gram_cur=(pr["WtW"], pr["CtC"]), xpM=M)
    assert res["status"] == 0
    G = res["gram_stats"]
    assert np.array_equal(G, G.T)
    g = fb.fused_gram_ratio(G, pr["th"]["W"], pr["th"]["C"], M, ldx, ldy)
    _note("fused Gram", f"R={r}", g)
    assert g <= 1.0, f"fused Gram {p}x{q} r={r}: err / bar {g}"
    # and the moments the block then computes are those of that Gram
    ssqX, ssqY, coef = _device_inputs(ctx, th, r)
    t = pr["th"]
    ref = fb.ScalarRef(G, pr["WtW"], pr["CtC"], ssqX, ssqY, pr["N"], p, q, np.diag(t["B"]), np.diag(t["sigT"]),
                       t["sigE"], t["sigF"], t["sigH"], coef)
    got = _scalar_got(res)
    for k in ("B", "sigT", "sigE", "sigF", "sigH", "alpha", "beta", "gamma", "delta"):   # a random M is no Gram:
        got.pop(k)                                                                        # Ctt may vanish
    rat = ref.ratios(got)
    assert max(rat.values()) <= 1.0, f"moments from the fused Gram {p}x{q} r={r}: err / bar {rat}"


def test_fused_gram_needs_r_at_most_8(ctx):
    from ppls_amd import PplsError
    p, q, r = 20, 18, 9
    _load(ctx, p, q)
    with pytest.raises(PplsError):
        ctx.finalize_stats(_plain_theta(p, q, r), np.ones((p, r)), np.ones((q, r)), _plain_gram(r),
                           xpM=np.zeros((fb.padded_width(p) + fb.padded_width(q), 2 * r)))


# ---------------------------------------------------------------------------- coverage
def test_coverage_and_worst():
    """Every templated R, the runtime-r kernel, the four path codes, staged 0 and 1 and K = 1, 4, 32
    appeared in an asserted case (this test follows them in the file: run the module as a whole)."""
    for k in sorted(WORST):
        print(f"worst err/bar {k[0]:>10s} {k[1]:<18s} {WORST[k]:.3g}")
    print("covered:", {k: sorted(v) for k, v in SEEN.items()})
    if not {(g, r) for g, r in GEO_CASES} <= RAN:   # (a -k selection leaves nothing to check here)
        return
    assert SEEN["R"] == set(range(1, 11))
    assert SEEN["generic"] >= {11, 13, 16}
    assert SEEN["code"] == {1, 2, 3, 4}
    assert SEEN["staged"] == {0, 1}
    assert SEEN["K"] >= {1, 4, 32}
