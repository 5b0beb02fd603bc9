"""Reference, a-priori error bar and host models of the 'o2m_xprod' pass and start, shared
by tests/test_o2m_bar_host.py and tests/test_gpu_o2m_xprod.py.

The pass (ppls_o2m.hip), for the rows x L block A at (row0, col0) of a row-major matrix of row length
ld, a vector v (L) and a vector d (rows):

    u_i = a_i . v - d_i,        z_j = sum_i u_i a_ij.

Reference: the same expressions in long double from the same fp64 inputs.

Bar for u_i: gamma(L + 2) (sum_j |a_ij v_j| + |d_i|) -- a dot product of L terms in any order and with
or without fused multiply-adds passes each term through at most L roundings (Higham, Accuracy and
Stability, §3.1), the subtraction adds one, and one more covers the second-order terms.

Bar for z_j: gamma(rows + 2) sum_i |u_i a_ij| for the sum itself in any order, plus the error u
carries in: sum_i bar_u_i |a_ij| (1 + gamma(rows + 2)).  Here u is the reference's; the computed u
differs from it by at most bar_u, which the second term pays for.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FUSED_LMAX = 2048          # PPLS_O2M_FUSED_LMAX
PATH_FUSED, PATH_TWOPHASE = 1, 2


def gamma(k):
    return k * U / (1.0 - k * U)


def make_case(rows, L, row0=0, col0=0, P=None, ld=None, d_zero=False, seed=0):
    """A rows x L block inside a P x ld matrix whose every entry outside the block's rows and its
    columns [col0, col0 + L rounded up to 2) is NaN.  The pad column of an odd L holds finite values
    the pass must read past: its products never enter u or z."""
    Lp = (L + 1) & ~1
    P = row0 + rows if P is None else P
    ld = col0 + Lp if ld is None else ld
    assert ld % 2 == 0 and col0 % 2 == 0 and col0 + Lp <= ld and row0 + rows <= P
    rng = np.random.default_rng(100003 * rows + 101 * L + 7 * row0 + col0 + seed)
    S = np.full((P, ld), np.nan)
    S[row0:row0 + rows, col0:col0 + Lp] = rng.standard_normal((rows, Lp)) * (0.5 + np.arange(Lp) % 7)
    v = rng.standard_normal(L)
    d = np.zeros(rows) if d_zero else rng.standard_normal(rows) * 3.0
    return dict(S=S, rows=rows, L=L, row0=row0, col0=col0, v=v, d=d, d_zero=d_zero)


def block(case):
    r0, c0 = case["row0"], case["col0"]
    return case["S"][r0:r0 + case["rows"], c0:c0 + case["L"]]


def reference(case):
    """(u, z) in long double."""
    A = block(case).astype(LD)
    u = A @ case["v"].astype(LD) - case["d"].astype(LD)
    return u, A.T @ u


def bars(case):
    """(bar_u, bar_z) as the module docstring derives them."""
    A = np.abs(block(case).astype(LD))
    rows, L = case["rows"], case["L"]
    u, _ = reference(case)
    bar_u = gamma(L + 2) * (A @ np.abs(case["v"].astype(LD)) + np.abs(case["d"].astype(LD)))
    g = gamma(rows + 2)
    bar_z = g * (A.T @ np.abs(u)) + (1.0 + g) * (A.T @ bar_u)
    return bar_u, bar_z


def fused_plan(rows, L, num_cus=256):
    """ppls_o2m.hip's fused plan for rows of at most 512 values (one wave per row; longer rows are shared
    by a workgroup's waves): column pairs per lane NJ, rows per wave step R, workgroups nb."""
    assert L <= 512
    Lp = (L + 1) & ~1
    NJ = 1
    while NJ * 128 < Lp:
        NJ *= 2
    R = 8 if NJ <= 2 else 4 if NJ <= 4 else 2
    nb = max(1, min(-(-rows // (4 * R * 2)), num_cus))     # two steps per wave, one workgroup per CU
    return NJ, R, nb


def _butterfly(x):
    """The wave reduction: partner sums at lane distances 32, 16, 8, 4, 2, 1."""
    x = np.array(x, dtype=np.float64)
    for h in (32, 16, 8, 4, 2, 1):
        x = x + x[np.arange(64) ^ h]
    return x[0]


def wide_plan(rows, L, num_cus=256):
    """The fused plan for 512 < L <= 2048 (ppls_o2m_fused_wide_kernel): 128-column chunks per wave NJW,
    rows per workgroup step R, workgroups nb (two steps each where the rows allow)."""
    assert 512 < L <= FUSED_LMAX
    nsteps = -(-rows // 4)
    return (2 if L <= 1024 else 4), 4, max(1, min((nsteps + 1) // 2, 2 * num_cus))


def twophase_plan(rows, L, num_cus=256):
    """The two-phase plan: 128-column slices, row groups nb, rows per group."""
    nslices = -(-((L + 1) & ~1) // 128)
    nb = max(1, min(-(-4 * num_cus // nslices), -(-rows // 32)))
    return nslices, nb, -(-rows // nb)


def model(case, num_cus=256, defect=None, kind="narrow"):
    """Plain fp64 in a kernel's summation order (products and sums rounded separately, where the kernel
    fuses them).

    kind 'narrow' (L <= 512, ppls_o2m_fused_kernel): lane l holds the column pairs 2 (l + 64 j); a row's
    dot is summed per lane over j, then over the wave; wave w of workgroup b takes the row steps
    b * 4 + w, + 4 nb, ... of R rows; the waves of a workgroup are added in order.
    kind 'wide' (512 < L <= 2048, ppls_o2m_fused_wide_kernel): wave w holds the 128-column chunks w,
    w + 4, ...; a row's dot is the four wave sums added in wave order; workgroup b takes the steps b,
    b + nb, ... of four rows; every column of a workgroup's partial belongs to one wave.
    kind 'twophase': u by one wave per row, lane l adding its pairs 2 l, 2 l + 128, ... in order; z over
    row groups, wave w of a group taking its rows w, w + 4, ..., the waves added in order.
    In each the partials are then added in sixteen interleaved groups, the groups in order.

    defect: None, or one of the seeded faults the bar must catch -- 'last_row' (the last row dropped),
    'tail_cols' (the columns past the last multiple of 128 dropped), 'no_d' (d ignored), 'stride_L' (the
    rows read at stride L rounded up to 2 instead of the matrix's), 'lost_partial' (the last partial of
    z dropped)."""
    rows, L = case["rows"], case["L"]
    S, r0, c0, v, d = case["S"], case["row0"], case["col0"], case["v"], case["d"]
    if kind == "narrow":
        NJ, R, nb = fused_plan(rows, L, num_cus)
        ncol = NJ * 128
    elif kind == "wide":
        NJW, R, nb = wide_plan(rows, L, num_cus)
        ncol = NJW * 512
    else:
        nslices, nb, rpg = twophase_plan(rows, L, num_cus)
        ncol = nslices * 128
    flat = S.ravel()
    ld = S.shape[1]
    stride = ((L + 1) & ~1) if defect == "stride_L" else ld
    Lc = (L // 128) * 128 if defect == "tail_cols" else L
    nrows = rows - 1 if defect == "last_row" else rows
    vv = np.zeros(ncol)
    vv[:Lc] = v[:Lc]
    u = np.zeros(rows)
    part = np.zeros((nb, 4, ncol))
    for i in range(nrows):
        a = np.zeros(ncol)
        base = r0 * ld + c0 + i * stride
        a[:Lc] = flat[base: base + Lc]
        prod = (a * vv).reshape(-1, 64, 2)                # chunk, lane, element of the pair
        if kind == "wide":
            waves = []
            for w in range(4):
                lanes = np.zeros(64)
                for j in range(NJW):
                    lanes = (lanes + prod[w + 4 * j, :, 0]) + prod[w + 4 * j, :, 1]
                waves.append(_butterfly(lanes))
            dot = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        else:                                             # narrow and two-phase: lane l, chunks in order
            lanes = np.zeros(64)
            for j in range(prod.shape[0]):
                lanes = (lanes + prod[j, :, 0]) + prod[j, :, 1]
            dot = _butterfly(lanes)
        u[i] = dot - (0.0 if defect == "no_d" else d[i])
        if kind == "narrow":
            gw = (i // R) % (4 * nb)
            part[gw // 4, gw % 4] += u[i] * a
        elif kind == "wide":
            part[(i // R) % nb, 0] += u[i] * a            # each column's owner adds the rows in order
        else:
            part[i // rpg, (i % rpg) % 4] += u[i] * a
    wg = ((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]
    groups = np.zeros((16, ncol))                # the second kernel: partial b goes to group b % 16 ...
    for b in range(nb):
        if defect == "lost_partial" and b == nb - 1:
            continue
        groups[b % 16] = groups[b % 16] + wg[b]
    z = groups[0]
    for g in range(1, 16):                       # ... and the groups are added in order
        z = z + groups[g]
    return u, z[:L]


def inside(got, ref, bar):
    """max over the entries of |got - ref| / bar (a bar of 0 demands equality; a NaN counts as inf)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


# ---- the deflated one-pass operator and the Lanczos solver, restated in numpy ------------------------


def numpy_pass(A, v, d):
    u = A @ v - d
    return u, A.T @ u


def _chain(V, x, first_last):
    """P_k .. P_1 x (first_last) or P_1 .. P_k x for P_j = I - v_j v_j'."""
    order = range(V.shape[1]) if first_last else reversed(range(V.shape[1]))
    x = x.copy()
    for j in order:
        x -= V[:, j] * (V[:, j] @ x)
    return x


def compact_T(Lv):
    """T' with (P_k .. P_1)'(P_k .. P_1) = I - Lv T' Lv'."""
    k = Lv.shape[1]
    G = Lv.T @ Lv
    T = np.zeros((k, k))
    for j in range(k):
        T[j, j] = 1.0
        T[j, :j] = -(G[j, :j] @ T[:j, :j])
    return T + T.T - T.T @ G @ T


def o2m_start_numpy(S, N, p, q, ldx, Wp=None, Cp=None, ssq=None, pass_fn=numpy_pass, cap=200):
    """The 'o2m_xprod' start from the padded cross-products S (X's columns at [0, p), Y's at [ldx, ldx + q)):
    the block with the shorter rows, deflation in d, Lanczos with full reorthogonalisation, the sign
    rule, B and the sigmas from the 2 x 2 Gram.  ssq: (||Xc||^2, ||Yc||^2) of the deflated data
    (default: computed from S as the sequential loop does).  Returns (start dict, info dict)."""
    Wp = np.zeros((p, 0)) if Wp is None else np.asarray(Wp, dtype=np.float64).reshape(p, -1)
    Cp = np.zeros((q, 0)) if Cp is None else np.asarray(Cp, dtype=np.float64).reshape(q, -1)
    k = Wp.shape[1]
    side = 0 if q <= p else 1
    if side == 0:
        A, Lv, Rv = S[0:p, ldx:ldx + q], Wp, Cp
    else:
        A, Lv, Rv = S[ldx:ldx + q, 0:p], Cp, Wp
    rows, L = A.shape
    AW = np.stack([pass_fn(A, np.zeros(L), -Lv[:, j])[1] for j in range(k)], axis=1) if k else np.zeros((L, 0))
    Tp = compact_T(Lv)
    passes = [0]

    def stage(y):
        vp = _chain(Rv, y, False)
        return vp, Lv @ (Tp @ (AW.T @ vp))

    def apply(y):
        vp, d = stage(y)
        passes[0] += 1
        return _chain(Rv, pass_fn(A, vp, d)[1], True)

    Q = [np.full(L, 1.0 / np.sqrt(L))]
    al, be = [], []
    while True:
        m = len(Q)
        r = apply(Q[-1])
        al.append(float(Q[-1] @ r))
        r = r - al[-1] * Q[-1] - (be[-1] * Q[-2] if m > 1 else 0.0)
        for _ in range(2):
            for qv in Q:
                r = r - (qv @ r) * qv
        beta = float(np.linalg.norm(r))
        Tm = np.diag(al) + np.diag(be, 1) + np.diag(be, -1)
        ev, V = np.linalg.eigh(Tm)
        theta, s = float(ev[-1]), V[:, -1]
        est = abs(beta * s[-1])
        if est <= theta * 2.0 ** -43 or m == L or m == cap:
            break
        be.append(beta)
        Q.append(r / beta)
    y = np.stack(Q, axis=1) @ s
    y /= np.linalg.norm(y)
    x = _chain(Lv, pass_fn(A, stage(y)[0], np.zeros(rows))[0], True)
    x /= np.linalg.norm(x)
    w, c = (x, y) if side == 0 else (y, x)
    if w[np.argmax(np.abs(w))] < 0:
        w, c = -w, -c
    zx, zy = _chain(Wp, w, False), _chain(Cp, c, False)
    Sxx, Syy, Sxy = S[0:p, 0:p], S[ldx:ldx + q, ldx:ldx + q], S[0:p, ldx:ldx + q]
    sst, ssu, tu = float(zx @ Sxx @ zx), float(zy @ Syy @ zy), float(zx @ Sxy @ zy)
    if ssq is None:
        ssq = [float(np.trace(Sxx)), float(np.trace(Syy))]
        for j in range(k):
            zj, yj = _chain(Wp[:, :j], Wp[:, j], False), _chain(Cp[:, :j], Cp[:, j], False)
            ssq[0] -= (2.0 - Wp[:, j] @ Wp[:, j]) * float(zj @ Sxx @ zj)
            ssq[1] -= (2.0 - Cp[:, j] @ Cp[:, j]) * float(yj @ Syy @ yj)
    B = tu / sst
    start = dict(W=w, C=c, B=B, sigE=float(np.sqrt((ssq[0] - sst) / N / p)), sigF=float(np.sqrt((ssq[1] - ssu) / N / q)),
                 sigH=float(np.sqrt((ssu - B * B * sst) / N)), sigT=float(np.sqrt(sst / N)))
    return start, dict(side=side, passes=passes[0], resid=est, theta=theta)
