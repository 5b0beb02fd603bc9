"""Reference, a-priori error bars and a host model of the cross-validation scoring kernel (DESIGN §14;
ppls_cv.hip: ppls_cv_score_kernel, ppls_cv_sse_reduce_kernel), shared by tests/test_cv_bar_host.py and
tests/test_gpu_cv_matrix.py.

For the rows i of a list and a fit (W p x k, C q x k, B k) the kernel forms the scores t_i = x_i W, scales them,
ts_im = t_im s_m (s = B, or 1 / B for predictions of X from Y), and returns either the prediction rows
sum_m ts_im c_m or, for every prefix j = 1 .. k of the components, SSE_j = sum_i ||y_i - sum_{m<=j} ts_im c_m||^2.

Reference (``reference``, ``reference_predict``): the same quantities in long double from the W, C, B actually
passed (fp64 values, orthonormal or not), for fp32 storage over the rows rounded to fp32.  ``ppls_predict`` stages
its new rows in fp64 whatever the context stores, so its reference never rounds them.  For xory = 1 the reference
divides by B in long double, where the library passes the fp64 quotient 1 / B: one rounding more (below).

The kernel's order and the bars (``bars``, ``bars_predict``), with u = 2^-53 and gamma(n) = n u / (1 - n u).
A wave owns RW = 64 / KT rows at a time (KT = 8 for k <= 8, else 16), its lanes the 16-byte units of a row
(VE = 2 doubles or 4 floats each).

* score.  Lane l adds the VE products of its units l, l + 64, .. to one accumulator: L1 = VE ceil(units / 64)
  additions behind the first term and, unfused, the product's own rounding; then the six levels of the
  reduce-scatter tree:
      Et_m = gamma(L1 + 6 + 1) sum_j |x_j| |w_jm|.
  (The compiler fuses the product into the addition; the count is the unfused one, which bounds both.)
  The product with s_m rounds once more, relative to the computed score, |t_m| + Et_m at most:
      Ets_m = (Et_m (1 + u) + u |t_m|) |s_m|           (xory = 1: 2 u |t_m|, for the rounding of 1 / B_m).
* residual.  e(j) = y - sum_{m<=j} ts_m c_m, component after component: j subtractions behind y, j behind the
  first product and its own rounding, of the computed ts_m (|ts_m| + Ets_m at most), plus what the error of
  ts_m moves the exact chain:
      de_c(j) = gamma(j + 1) (|y_c| + sum_{m<=j} (|ts_m| + Ets_m) |c_cm|) + sum_{m<=j} Ets_m |c_cm|.
* sum.  Behind one square on its way into SSE_j (``n_sum``): the square itself (1); the RW VE squares a lane
  adds into r2 for one component and trip; one addition into the lane's sse[m] per ``base`` trip
  (ceil(units of Y / 64) of them) and per row group of the wave (ceil(groups / (4 grid)), the grid-stride);
  the six levels of wave_total; in the reduce kernel the ``per`` = ceil(4 grid / 256) partials a thread adds in
  sequence and the 256 threads' values added in sequence:
      N_sum = 1 + RW VE + trips groups_per_wave + 6 + per + 256,
      bar(SSE_j) = gamma(N_sum) sum (|e| + de)^2 + sum (2 |e| de + de^2)        (sums over rows and columns).
  The first term bounds the summation of the computed squares, each at most (|e| + de)^2, the second what the
  residual's own error moves a square.  On an exact fit (Y = X W diag(B) C' to rounding) e is rounding noise and
  the bar is an absolute one of the size of de^2: the residual is formed directly, so nothing cancels.
* predict.  pred_c = sum_m ts_m b_cm from zero, k products and additions:
      bar(pred_c) = gamma(k + 1) sum_m (|ts_m| + Ets_m) |b_cm| + sum_m Ets_m |b_cm|.

The host model (``model``, ``model_predict``) is the kernel's arithmetic in fp64 numpy, products and sums rounded
separately: lane partials per unit, the tree, t s, the sequential residual per ``base`` trip with the lanes past
the row's end masked, r2, the lanes' sums over the trips and the grid-stride groups of a wave for a given grid,
wave_total, then the reduce kernel's order.  ``defect=`` seeds one of DEFECTS.
"""
import numpy as np

from rowdiag_bar import L, U, gamma, inside, lane_terms, stored  # noqa: F401  (inside: re-exported for the tests)
# the streamed-fold path (ppls_heldout_sse_fold) and the downdate have their references and bars already
from test_cv_stream_host import K_SSE, fold_refs, seeded_labels, sse_bar, sse_direct, sse_quadratic  # noqa: F401
from test_stream_host import K_STAGES, gram_bar, scale_ref  # noqa: F401

WAVES = 4      # PPLS_CV_WAVES
K_TREE = 6     # levels of the wave trees
REDUCE = 256   # threads of ppls_cv_sse_reduce_kernel

DEFECTS = {
    1: "the residual loop stops after the first 64 units of the second factor",
    2: "in the KT = 16 tile the scores are read from lane rr * 8 + m",
    3: "a partial last row group counts all RW rows: the repeated first row is scored",
    4: "row groups beyond the grid are dropped: no grid-stride",
    5: "the reduce kernel adds only the first 256 partials",
    6: "only the first row of every group is scored (the bug DESIGN §14 records)",
}


# ------------------------------------------------------------------------------------ launch geometry
def rows_per_wave(k):
    """ppls_cv_rows_per_wave."""
    return 8 if k <= 8 else 4


def cv_grid(nrows, k, num_cus):
    """ppls_cv_grid: one workgroup per 4 RW rows, at most 4 per compute unit (256 units when unknown), at least 1."""
    per = rows_per_wave(k) * WAVES
    blocks, cap = -(-int(nrows) // per), (num_cus if num_cus > 0 else 256) * 4
    return 1 if blocks < 1 else min(blocks, cap)


def n_sum(nrows, q, k, f32, grid):
    """Roundings behind one square of SSE_j (module docstring)."""
    rw, ve = rows_per_wave(k), 4 if f32 else 2
    _, trips, _ = lane_terms(q, f32)
    groups = -(-int(nrows) // rw)
    per_wave = -(-groups // (WAVES * grid))
    per = -(-(WAVES * grid) // REDUCE)
    return 1 + rw * ve + trips * max(per_wave, 1) + K_TREE + per + REDUCE


# ------------------------------------------------------------------------------------ reference and bars
def _fit(W, C, B):
    W = np.array(W, dtype=np.float64, ndmin=2)
    C = np.array(C, dtype=np.float64, ndmin=2)
    B = np.asarray(B, dtype=np.float64)
    B = np.diag(B).copy() if B.ndim == 2 else np.ravel(B).copy()
    assert W.shape[1] == C.shape[1] == B.shape[0]
    return W, C, B


def _rows_of(X, Y, rows, f32):
    rows = np.ravel(np.asarray(rows, dtype=np.int64))
    return stored(X, f32)[rows].astype(L), stored(Y, f32)[rows].astype(L)


def reference(X, Y, W, C, B, rows, f32=False, residuals=True):
    """Long double: t (n x k), ts = t B, sse (k) and, with ``residuals``, e (k x n x q), e[j - 1] = e(j)."""
    W, C, B = _fit(W, C, B)
    Xs, Ys = _rows_of(X, Y, rows, f32)
    Cl = C.astype(L)
    t = Xs @ W.astype(L)
    ts = t * B.astype(L)
    cur, sse, e = Ys.copy(), [], []
    for m in range(W.shape[1]):
        cur = cur - ts[:, m:m + 1] * Cl[None, :, m]
        sse.append((cur * cur).sum())
        if residuals:
            e.append(cur)
    out = dict(t=t, ts=ts, sse=np.array(sse, dtype=L))
    if residuals:
        out["e"] = np.array(e, dtype=L).reshape(W.shape[1], Xs.shape[0], Ys.shape[1])
    return out


def _score_bar(aX, t, A, s_abs, f32, s_roundings=1):
    """Ets (n x k): the bar of the scaled scores from |x|, the exact t, the first factor A and |s|."""
    L1, _, _ = lane_terms(A.shape[0], f32)
    Et = gamma(L1 + K_TREE + 1) * (aX @ np.abs(A).astype(L))
    return (Et * (1 + U) + s_roundings * U * np.abs(t)) * s_abs


def bars(X, Y, W, C, B, rows, f32=False, grid=None, num_cus=256):
    """The a-priori bars (module docstring): dict(ts n x k, sse k as float64, n_sum).  ``grid``: the scoring
    grid of the call (default: cv_grid of the row count and ``num_cus``)."""
    W, C, B = _fit(W, C, B)
    Xs, Ys = _rows_of(X, Y, rows, f32)
    n, q, k = Xs.shape[0], Ys.shape[1], W.shape[1]
    grid = cv_grid(n, k, num_cus) if grid is None else grid
    N = n_sum(n, q, k, f32, grid)
    aC = np.abs(C).astype(L)
    t = Xs @ W.astype(L)
    ts = t * B.astype(L)
    Ets = _score_bar(np.abs(Xs), t, W, np.abs(B).astype(L), f32)
    cur, s1, s2, out = Ys.copy(), np.abs(Ys), np.zeros_like(Ys), []
    for m in range(k):
        cur = cur - ts[:, m:m + 1] * C.astype(L)[None, :, m]
        s1 = s1 + (np.abs(ts[:, m:m + 1]) + Ets[:, m:m + 1]) * aC[None, :, m]
        s2 = s2 + Ets[:, m:m + 1] * aC[None, :, m]
        de = gamma(m + 2) * s1 + s2
        ae = np.abs(cur)
        out.append(gamma(N) * ((ae + de) ** 2).sum() + (2 * ae * de + de * de).sum())
    return dict(ts=np.asarray(Ets, dtype=np.float64), sse=np.array(out, dtype=np.float64), n_sum=N)


def _predict_parts(newdata, W, C, B, xory):
    W, C, B = _fit(W, C, B)
    nd = np.asarray(newdata, dtype=np.float64).astype(L)
    A, Bm = (C, W) if xory else (W, C)
    s = 1 / B.astype(L) if xory else B.astype(L)
    return nd, A, Bm, s


def reference_predict(newdata, W, C, B, xory=0):
    """Long double: newdata W diag(B) C' (xory 0) or newdata C diag(1 / B) W' (xory 1); dict(t, ts, pred)."""
    nd, A, Bm, s = _predict_parts(newdata, W, C, B, xory)
    t = nd @ A.astype(L)
    ts = t * s
    return dict(t=t, ts=ts, pred=ts @ Bm.astype(L).T)


def bars_predict(newdata, W, C, B, xory=0):
    """Per-element bar of the prediction (module docstring), float64 n x (q or p).  The rows are fp64."""
    nd, A, Bm, s = _predict_parts(newdata, W, C, B, xory)
    k = A.shape[1]
    t = nd @ A.astype(L)
    ts = t * s
    Ets = _score_bar(np.abs(nd), t, A, np.abs(s), False, 2 if xory else 1)
    aB = np.abs(Bm).astype(L).T
    return np.asarray(gamma(k + 1) * ((np.abs(ts) + Ets) @ aB) + Ets @ aB, dtype=np.float64)


# ------------------------------------------------------------------------------------ host model
def _tree64(v):
    """The xor tree over the last axis of 64 lanes, partners differing in bit 32 first (scatter_step<32> .. <1>,
    wave_total): every lane ends with the same bits, a + b being b + a."""
    idx = np.arange(64)
    for h in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ h]
    return v[..., 0]


def _units(A, ve):
    """n x cols -> n x sweeps x 64 x ve: the 16-byte units of a row by lane sweep, zero beyond the row."""
    n, cols = A.shape
    sweeps = -(-(-(-cols // ve)) // 64)
    P = np.zeros((n, sweeps * 64 * ve))
    P[:, :cols] = A
    return P.reshape(n, sweeps, 64, ve)


def _kernel(Xr, Yr, A, Bm, s, f32, grid, defect, pred):
    """ppls_cv_score_kernel (and, for the sums, ppls_cv_sse_reduce_kernel) on the n rows Xr, Yr in fp64."""
    n, k = Xr.shape[0], A.shape[1]
    qb = Bm.shape[0]
    rw, ve = rows_per_wave(k), 4 if f32 else 2
    kt = 64 // rw
    if n == 0:
        return np.zeros((0, qb)) if pred else np.zeros(k)
    ng = -(-n // rw)
    pos = np.arange(ng * rw).reshape(ng, rw)
    valid = pos < n
    G = np.where(valid, pos, pos[:, :1])                   # rows past the end repeat the group's first
    if defect == 3 and not pred:
        valid = np.ones_like(valid)
    if defect == 6:
        valid = valid & (np.arange(rw) == 0)[None, :]
    # scores: a lane's partial over its units, the tree, the product with s
    Xu, Au = _units(Xr, ve), _units(np.ascontiguousarray(A.T), ve)
    acc = np.zeros((n, 64, k))
    for sw in range(Xu.shape[1]):
        for e in range(ve):
            acc = acc + Xu[:, sw, :, e, None] * Au[:, sw, :, e].T[None]
    v = np.zeros((ng, 64, 64))                             # group, lane, slot rr * KT + m
    for rr in range(rw):
        v[:, :, rr * kt:rr * kt + k] = acc[G[:, rr]]
    sm = np.zeros(64)
    comp = np.arange(64) % kt
    sm[comp < k] = np.asarray(s, dtype=np.float64)[comp[comp < k]]
    tl = _tree64(np.moveaxis(v, 1, -1)) * sm               # lane rr * KT + m: t_rr,m s_m
    stride = 8 if (defect == 2 and kt == 16) else kt
    trm = tl[:, np.arange(rw)[:, None] * stride + np.arange(k)[None, :]]   # group, rr, m
    # second factor
    Cu = _units(np.ascontiguousarray(Bm.T), ve)            # k x trips x 64 x ve
    trips, nb = Cu.shape[1], -(-qb // ve)
    act = (np.arange(trips)[:, None] * 64 + np.arange(64)[None, :]) < nb
    if defect == 1:
        act = act & (np.arange(trips) == 0)[:, None]
    Yg = np.zeros((ng, rw, trips, 64, ve)) if pred else _units(Yr, ve)[G]
    R = np.zeros((k, ng, trips, 64))
    for m in range(k):
        term = trm[:, :, m, None, None, None] * Cu[m][None, None]
        Yg = Yg + term if pred else Yg - term
        if not pred:
            r2 = np.zeros((ng, trips, 64))
            for rr in range(rw):
                for e in range(ve):
                    r2 = np.where(valid[:, rr, None, None], r2 + Yg[:, rr, :, :, e] * Yg[:, rr, :, :, e], r2)
            R[m] = np.where(act[None], r2, 0.0)
    if pred:
        out = np.where(valid[:, :, None, None, None] & act[None, None, :, :, None], Yg, 0.0)
        return out.reshape(ng * rw, trips * 64 * ve)[:n, :qb]
    # a wave's lanes over its groups g = wave, wave + nw, .. and their trips, wave_total, the reduce kernel
    nw = WAVES * grid
    rounds = -(-ng // nw)
    Rp = np.zeros((k, rounds * nw, trips, 64))
    Rp[:, :ng] = R
    Rp = Rp.reshape(k, rounds, nw, trips, 64)
    lane = np.zeros((k, nw, 64))
    for r in range(1 if defect == 4 else rounds):
        for tr in range(trips):
            lane = lane + Rp[:, r, :, tr, :]
    part = _tree64(lane)                                   # k x nparts
    per = 1 if defect == 5 else -(-nw // REDUCE)
    th = np.zeros((k, REDUCE))
    for i in range(per):
        idx = np.arange(REDUCE) * per + i
        th = th + np.where(idx < nw, part[:, np.minimum(idx, nw - 1)], 0.0)
    tot = np.zeros(k)
    for i in range(REDUCE):
        tot = tot + th[:, i]
    return tot


def model(X, Y, W, C, B, rows, f32=False, grid=None, num_cus=256, defect=None):
    """ppls_heldout_sse in the kernel's order, plain fp64: the k prefix sums."""
    W, C, B = _fit(W, C, B)
    rows = np.ravel(np.asarray(rows, dtype=np.int64))
    grid = cv_grid(rows.shape[0], W.shape[1], num_cus) if grid is None else grid
    return _kernel(stored(X, f32)[rows], stored(Y, f32)[rows], W, C, B, f32, grid, defect, False)


def model_predict(newdata, W, C, B, xory=0, defect=None):
    """ppls_predict in the kernel's order, plain fp64 (the rows are staged in fp64; s = 1 / B rounded)."""
    W, C, B = _fit(W, C, B)
    A, Bm = (C, W) if xory else (W, C)
    s = 1.0 / B if xory else B
    return _kernel(np.asarray(newdata, dtype=np.float64), None, A, Bm, s, False, 1, defect, True)


# ------------------------------------------------------------------------------------ test data
# group a of the GPU matrix.  (67, 37, 19): one trip, odd widths, no multiple of 4 for fp32; (70, 261, 259): fp64
# 131 and 130 units, three sweeps of the score loop and three ``base`` trips with a partial last one, fp32 66 and
# 65 units, two trips with one live lane in the last; (40, 6, 128), (40, 6, 256): exactly 64 units of Y in fp64 and
# in fp32; (9, 1, 1)
SSE_SHAPES = [(67, 37, 19), (70, 261, 259), (40, 6, 128), (40, 6, 256), (9, 1, 1)]
SSE_RANKS = [1, 2, 7, 8, 9, 15, 16]
ROW_KINDS = ("third", "all", "last")
PREDICT_SHAPES = [(67, 37, 19), (5, 261, 259), (1, 37, 19)]
PREDICT_RANKS = [1, 8, 9, 16]
# group e (n, p, q, K): the second has p and q odd and beyond 128, so a wave sweeps a row of S more than once
STREAM_SHAPES = [(300, 33, 17, 3), (260, 131, 141, 2)]
STREAM_RANKS = [1, 8, 9, 16]


def make_data(n, p, q, seed=0):
    """n rows of p + q columns of unequal scale with a shared part, so that no fit is exact."""
    rng = np.random.default_rng([seed, n, p, q])
    z = rng.standard_normal((n, 1))
    X = (rng.standard_normal((n, p)) + 0.5 * z) * (0.5 + np.arange(p) % 3)
    Y = (rng.standard_normal((n, q)) - 0.7 * z) * (0.25 + np.arange(q) % 4)
    return X, Y


def fit_parts(p, q, k, seed=0):
    """W, C with orthonormal columns where the shape allows it (a QR's Q; columns of norm ~ 1 where k exceeds
    the rows) and B in +-[0.5, 1.5]: tests/test_gpu_cv.py's _fit_parts for every k <= 16."""
    rng = np.random.default_rng([seed, p, q, k])

    def loadings(rows):
        M = rng.standard_normal((rows, k))
        return np.linalg.qr(M)[0] if rows >= k else M / np.sqrt(rows)

    W, C = loadings(p), loadings(q)
    B = rng.uniform(0.5, 1.5, size=k) * rng.choice([-1.0, 1.0], size=k)
    return W, C, B


def exact_fit(X, W, C, B, f32=False):
    """Y = X W diag(B) C' of the rows as stored, formed in long double and rounded to fp64: a noise-free fit."""
    W, C, B = _fit(W, C, B)
    return np.asarray((stored(X, f32).astype(L) @ W.astype(L) * B.astype(L)) @ C.astype(L).T, dtype=np.float64)


def row_list(kind, n, seed=1):
    """A sorted random third of the rows, all rows, or the single last row."""
    if kind == "third":
        return np.sort(np.random.default_rng(seed).permutation(n)[:max(1, n // 3)])
    return np.arange(n) if kind == "all" else np.array([n - 1])


def residue_rows(n=40, longest=17, seed=2):
    """Group b: the first len entries, len = 1 .. longest, of one sorted random permutation's head."""
    head = np.sort(np.random.default_rng(seed).permutation(n)[:longest])
    return [head[:m] for m in range(1, longest + 1)]


def stream_triples(Z, labels, fold, p, k, seed=0):
    """Group e's fits for one fold of the standardised rows Z = [X Y]: a random triple, and the rank-k truncation
    of the least-squares coefficients of the other folds, which makes the expansion of the quadratic form cancel
    (tests/test_cv_stream_host.py::test_sse_quadratic_form_against_direct_residuals builds it at rank 3)."""
    Z = np.asarray(Z, dtype=np.float64)
    tr = Z[labels != fold]
    Um, s, Vt = np.linalg.svd(np.linalg.lstsq(tr[:, :p], tr[:, p:], rcond=None)[0], full_matrices=False)
    return dict(random=fit_parts(p, Z.shape[1] - p, k, seed=seed + 7),
                lstsq=(Um[:, :k].copy(), Vt[:k].T.copy(), s[:k].copy()))


def wide_rows(k, num_cus):
    """Group c: (nrows_1, nrows_2): more than 256 wave partials (per = 2), and one grid-stride trip with a
    ragged tail on a device of ``num_cus`` compute units."""
    rw = rows_per_wave(k)
    return 64 * WAVES * rw + WAVES * rw + 3, (4 * num_cus) * WAVES * rw + WAVES * rw + 3
