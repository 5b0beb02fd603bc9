"""Every sweep kernel instantiation against long-double statistics (tests/sweep_bar.py).

``Context.sweep_stats`` runs one statistics step through the production dispatch (``sweep_plan``),
so the kernel checked is the one ``sweep_kernel`` names; every case first asserts that name against
the table below, written out literally: if the dispatcher changes, the table fails instead of
silently losing coverage.  The statistics (X'mu_T, Y'mu_U, the Gram of [XW YC]) and the moments are
held entrywise to an a-priori rounding bar -- nothing in it is measured, see sweep_bar.py -- at the
smallest shapes that select each body of ``ppls_sweep_split_kernel`` and at the per-workgroup row
counts where the DMA ring's prologue and tail arithmetic changes branch.  Each case runs the
counted-wait path (no mu write-out) twice, bitwise equal (a read of a slot that has not landed
rarely repeats), and the drained path (mu written out) once.

The panel sweep (``sweep=3``: mfmadots + acc kernels, R up to 16, fp64 and fp32 storage) gets the
same reference and bar over its dots forms, and the segmented sweep behind meta_PPLSi is run at the
wide split instantiations against the oracle.

Two cases of the plan need ncol(Y) >= r, which the library's theta check enforces as the reference
does (EM_W_multi.R:245): shape C at r = 8 and the wide panel shape at r = 10, 16 take q = r there
(sweep_bar.shape_pq, panel_pq); the split case keeps its padded width, hence its kernel body.

Worst err / bar on the MI355X when this file was written (each test prints its own; a later change
that eats the margin shows against these): split NSH 1 0.385 (shape A, where m = 16 and about 4 u of
it is the library's and the oracle's fp64 alpha..delta differing, see sweep_bar.sweep_problem;
shape B 0.0032), NSH 2 0.0069, NSH 4 0.0020; panel fp64 0.076, fp32 0.106 (both at p, q = 70, 37;
0.004 at p = 2100).
"""
import itertools
import zlib

import numpy as np
import pytest

import sweep_bar as sb
from conftest import make_problem
from oracle import ppls_oracle as o

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------- the expected kernels
# split<R,NSH,threads,RP,PIPE,SLOTS,CPW> by R: (rows_per_step 0 (auto), rows_per_step 1)
NSH1 = {
    1: ("split<1,1,512,2,true,4,2>", "split<1,1,512,1,true,4,2>"),
    2: ("split<2,1,512,2,true,4,2>", "split<2,1,512,1,true,4,2>"),
    3: ("split<3,1,512,2,true,4,2>", "split<3,1,512,1,true,4,2>"),
    4: ("split<4,1,512,2,true,4,2>", "split<4,1,512,1,true,4,2>"),
    5: ("split<5,1,512,2,true,4,2>", "split<5,1,512,1,true,4,2>"),
    6: ("split<6,1,512,2,true,4,2>", "split<6,1,512,1,true,4,2>"),
    7: ("split<7,1,512,2,true,4,2>", "split<7,1,512,1,true,4,2>"),
    8: ("split<8,1,512,2,true,4,2>", "split<8,1,512,1,true,4,2>"),
}
# R = 7, 8 have no two-row instantiation at NSH 2: rows_per_step 0 falls back to one row per step
NSH2 = {
    1: ("split<1,2,512,2,true,4,2>", "split<1,2,512,1,true,4,2>"),
    2: ("split<2,2,512,2,true,4,2>", "split<2,2,512,1,true,4,2>"),
    3: ("split<3,2,512,2,true,4,2>", "split<3,2,512,1,true,4,2>"),
    4: ("split<4,2,512,2,true,4,2>", "split<4,2,512,1,true,4,2>"),
    5: ("split<5,2,512,2,true,4,2>", "split<5,2,512,1,true,4,2>"),
    6: ("split<6,2,512,2,true,4,2>", "split<6,2,512,1,true,4,2>"),
    7: ("split<7,2,512,1,true,4,2>", "split<7,2,512,1,true,4,2>"),
    8: ("split<8,2,512,1,true,4,2>", "split<8,2,512,1,true,4,2>"),
}
# NSH 4 by R: (rows_per_step 0, rows_per_step 1 with pipe 1, rows_per_step 1 with pipe 0)
NSH4_CPW2 = {
    1: ("split<1,4,512,2,false,4,2>", "split<1,4,512,1,true,4,2>", "split<1,4,512,1,false,4,2>"),
    2: ("split<2,4,512,2,false,4,2>", "split<2,4,512,1,true,4,2>", "split<2,4,512,1,false,4,2>"),
    3: ("split<3,4,512,2,false,4,2>", "split<3,4,512,1,true,4,2>", "split<3,4,512,1,false,4,2>"),
    4: ("split<4,4,512,2,false,4,2>", "split<4,4,512,1,true,4,2>", "split<4,4,512,1,false,4,2>"),
    5: ("split<5,4,512,2,false,4,2>", "split<5,4,512,1,true,4,2>", "split<5,4,512,1,false,4,2>"),
}
NSH4_CPW4 = {
    1: ("split<1,4,512,2,false,4,4>", "split<1,4,512,1,true,4,4>", "split<1,4,512,1,false,4,4>"),
    2: ("split<2,4,512,2,false,4,4>", "split<2,4,512,1,true,4,4>", "split<2,4,512,1,false,4,4>"),
    3: ("split<3,4,512,2,false,4,4>", "split<3,4,512,1,true,4,4>", "split<3,4,512,1,false,4,4>"),
    4: ("split<4,4,512,2,false,4,4>", "split<4,4,512,1,true,4,4>", "split<4,4,512,1,false,4,4>"),
    5: ("split<5,4,512,2,false,4,4>", "split<5,4,512,1,true,4,4>", "split<5,4,512,1,false,4,4>"),
}
TABLE = {"A": NSH1, "B": NSH1, "C": NSH2, "D": NSH2, "E": NSH4_CPW2, "E'": NSH4_CPW2, "F": NSH4_CPW4,
         "G": NSH4_CPW4}
FAMILY = {"A": "split NSH 1", "B": "split NSH 1", "C": "split NSH 2", "D": "split NSH 2", "E": "split NSH 4",
          "E'": "split NSH 4", "F": "split NSH 4", "G": "split NSH 4"}
# whether the kernel's guard-free LDS reads are on at the shape (4 NSH <= nchx, nchy)
FULL = {"A": False, "B": True, "C": False, "D": True, "E": False, "E'": False, "F": False, "G": True}

SEEN = set()      # the split names the matrix ran
RAN = set()       # the (shape, r) cases of the matrix that ran to their end
WORST = {}        # family -> worst err / bar


def split_options(shape, r):
    """[(rows_per_step, pipe, expected name)]: the option settings that select distinct instantiations."""
    names = TABLE[shape][r]
    if len(names) == 2:
        return [(0, 1, names[0]), (1, 1, names[1])]
    return [(0, 1, names[0]), (1, 1, names[1]), (1, 0, names[2])]


# ---------------------------------------------------------------------------- the dispatcher's rules
def _nch(ldx, ldy):
    return ((ldx * 8 + 1023) >> 10) + ((ldy * 8 + 1023) >> 10)


def _split_lds(r, ldx, ldy, rp):
    v, nw = r * rp, 8
    return 4 * (_nch(ldx, ldy) << 10) + (2 * nw * v + nw * 2 * v + 4 * r) * 8


def dispatch_name(r, ldx, ldy, rp_opt, pipe_opt):
    """ppls_split_supported + launch_split_r + launch_split_cpw restated: the name, or None."""
    nsh = (max(ldx, ldy) // 2 + 255) // 256
    ns = 1 if nsh <= 1 else 2 if nsh <= 2 else 4 if nsh <= 4 else 0
    if not 1 <= r <= 8 or ns == 0 or (ns == 4 and r > 5) or _nch(ldx, ldy) > 32:
        return None
    if _split_lds(r, ldx, ldy, 2) > 160 * 1024:
        return None
    if ns == 1:
        rp, pipe = (2 if rp_opt != 1 else 1), True
    elif ns == 2:
        rp, pipe = (2 if r <= 6 and rp_opt != 1 else 1), True
    else:
        rp = 2 if rp_opt != 1 else 1
        pipe = False if rp == 2 else bool(pipe_opt)
    need = (_nch(ldx, ldy) + 7) // 8
    cpw = 2 if need <= 2 else 4 if need <= 4 else 0
    if not cpw:
        return None
    return f"split<{r},{ns},512,{rp},{'true' if pipe else 'false'},4,{cpw}>"


def dispatchable_names():
    """Every name the dispatcher can produce: all r, options and fp64 widths (even, <= 2048; the
    rules change only at multiples of 128 columns, so those and their neighbours stand for all)."""
    widths = sorted({2} | {w for k in range(1, 17) for w in (128 * k - 2, 128 * k, 128 * k + 2) if w <= 2048})
    names = set()
    for r, ldx, ldy, rp, pipe in itertools.product(range(1, 9), widths, widths, (0, 1, 2), (0, 1)):
        nm = dispatch_name(r, ldx, ldy, rp, pipe)
        if nm:
            names.add(nm)
    return names


# ---------------------------------------------------------------------------- fixtures and helpers
@pytest.fixture(scope="module")
def ctx():
    from ppls_amd import Context
    c = Context(0)
    yield c
    c.close()


DEFAULTS = dict(sweep=0, grid=0, rows_per_step=0, pipe=1, nt=-1, dtype=0, dots_rows=0, dots_pair=-1, acc_chunks=0)


def _restore(ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


def _check(ctx, th, ref, label):
    """One case: the counted-wait path twice (bitwise equal), the mu write-out path once; statistics
    of both and the moments of the second inside the bar.  Returns the worst err / bar."""
    s0 = ctx.sweep_stats(th, want_mu=False)
    s0b = ctx.sweep_stats(th, want_mu=False)
    for u, v in zip(s0[:3], s0b[:3]):
        assert np.array_equal(u, v), f"{label}: the counted-wait sweep does not repeat bitwise"
    s1 = ctx.sweep_stats(th, want_mu=True)
    worst = 0.0
    for path, s in (("counted waits", s0), ("mu write-out", s1)):
        assert np.array_equal(s[2], s[2].T), f"{label} ({path}): Gram not symmetric"
        rat = ref.ratios(*s)
        assert max(rat.values()) <= 1.0, f"{label} ({path}): err / bar {rat}"
        worst = max(worst, *rat.values())
    return worst


def _seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode())


# ---------------------------------------------------------------------------- split matrix
SPLIT_CASES = [(s, r) for s in sb.SHAPES for r in range(1, sb.RMAX_OF[s] + 1)]


@pytest.mark.parametrize("shape,r", SPLIT_CASES, ids=[f"{s}-r{r}" for s, r in SPLIT_CASES])
def test_split_matrix(ctx, shape, r):
    from ppls_amd import Theta
    p, q = sb.shape_pq(shape, r)
    ldx, ldy = sb.padded_width(p), sb.padded_width(q)
    nchx, nchy = (ldx * 8 + 1023) >> 10, (ldy * 8 + 1023) >> 10
    nsh = int(TABLE[shape][r][0].split(",")[1])
    assert (4 * nsh <= min(nchx, nchy)) == FULL[shape]
    worst = 0.0
    try:
        for n, grid in sb.ROWS:
            X, Y, thd = sb.sweep_problem(n, p, q, r, _seed(shape, r, n))
            ref = sb.Reference(X, Y, thd, ldx, ldy)
            th = Theta(**thd)
            ctx.set_option("grid", grid)
            ctx.set_data(X, Y)
            for (rp, pipe, name), nt in itertools.product(split_options(shape, r), (0, 1)):
                ctx.set_option("rows_per_step", rp)
                ctx.set_option("pipe", pipe)
                ctx.set_option("nt", nt)
                want = name + (" nt" if nt else "")
                assert ctx.sweep_kernel(r) == want
                assert dispatch_name(r, ldx, ldy, rp, pipe) == name
                worst = max(worst, _check(ctx, th, ref, f"{shape} r={r} n={n} grid={grid} {want}"))
                SEEN.add(name)
    finally:
        _restore(ctx)
    RAN.add((shape, r))
    WORST[FAMILY[shape]] = max(WORST.get(FAMILY[shape], 0.0), worst)
    print(f"split {shape} r={r}: worst err/bar {worst:.3g}")


def test_every_dispatchable_split_name_is_exercised():
    """The table covers every name the dispatcher can produce, and the matrix above ran them all
    (this test follows it in the file: run the module as a whole)."""
    can = dispatchable_names()
    table = {nm for s, r in SPLIT_CASES for _, _, nm in split_options(s, r)}
    assert table == can, (sorted(table - can), sorted(can - table))
    assert len(can) == 60
    if RAN == set(SPLIT_CASES):   # (a -k selection of the matrix leaves only the static check above)
        assert SEEN == can, sorted(can - SEEN)
    for fam in sorted(WORST):
        print(f"{fam}: worst err/bar {WORST[fam]:.3g}")


# ---------------------------------------------------------------------------- panel matrix
PANEL_CASES = [(dt, s, r) for s in sb.PANEL_SHAPES for dt in ("fp64", "fp32") for r in sb.PANEL_R[s]]


@pytest.mark.parametrize("dtype,shape,r", PANEL_CASES, ids=[f"{d}-{s}-r{r}" for d, s, r in PANEL_CASES])
def test_panel_matrix(ctx, dtype, shape, r):
    from ppls_amd import Theta
    f32 = dtype == "fp32"
    p, q = sb.panel_pq(shape, r)
    ldx, ldy = sb.padded_width(p, f32), sb.padded_width(q, f32)
    worst = 0.0
    try:
        ctx.set_option("sweep", 3)
        ctx.set_option("dtype", int(f32))
        for n in sb.PANEL_ROWS:
            X, Y, thd = sb.sweep_problem(n, p, q, r, _seed("panel", dtype, p, r, n))
            if f32:   # the data as stored
                X = X.astype(np.float32).astype(np.float64)
                Y = Y.astype(np.float32).astype(np.float64)
            ref = sb.Reference(X, Y, thd, ldx, ldy)
            th = Theta(**thd)
            ctx.set_data(X, Y)
            for rows, pair, nt, chunks in itertools.product((32, 64), (0, 1), (0, 1), (1, 3)):
                ctx.set_option("dots_rows", rows)
                ctx.set_option("dots_pair", pair)
                ctx.set_option("nt", nt)
                ctx.set_option("acc_chunks", chunks)
                want = (f"panel<{'float' if f32 else 'double'},{r}> (mfmadots {rows} rows/"
                        f"{'wave pair' if pair else 'wave'} + acc, {chunks} chunks)")
                assert ctx.sweep_kernel(r) == want
                worst = max(worst, _check(ctx, th, ref, f"{p}x{q} n={n} nt={nt} {want}"))
    finally:
        _restore(ctx)
        ctx.set_data(np.zeros((1, 2)), np.zeros((1, 2)))
    WORST["panel " + dtype] = max(WORST.get("panel " + dtype, 0.0), worst)
    print(f"panel {dtype} {p}x{q} r={r}: worst err/bar {worst:.3g}")


def test_panel_worst():
    for fam in sorted(f for f in WORST if f.startswith("panel")):
        print(f"{fam}: worst err/bar {WORST[fam]:.3g}")


# ---------------------------------------------------------------------------- segmented sweep, wide
def _relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("sizes", [[3, 500, 2, 495], [40] * 6], ids=["tiny_pops", "K6"])
@pytest.mark.parametrize("shape", ["E", "F", "G"])
def test_segmented_sweep_wide(ctx, shape, sizes):
    """meta_PPLSi's segmented sweep (one launch per EM step, a population per workgroup range) at the
    NSH 4 instantiations, 3 steps against the oracle at test_gpu_meta.py's tolerances."""
    p, q = sb.SHAPES[shape]
    n = int(sum(sizes))
    X, Y, _ = make_problem(n, p, q, 1, seed=_seed("meta", shape, n))
    init = o.initial_guess(p, q, "equal")
    _restore(ctx)
    ctx.set_data(X, Y)
    W, C, P, lg = ctx.meta_ppls(sizes, 3, -np.inf, init)
    assert ctx.meta_info() == "device_split"
    assert ctx.sweep_kernel(1) == {"E": "split<1,4,512,2,false,4,2>", "F": "split<1,4,512,2,false,4,4>",
                                   "G": "split<1,4,512,2,false,4,4>"}[shape]
    ref = o.meta_pplsi(X, Y, sizes, 3, -np.inf, init)
    assert lg.shape == ref["logvalue"].shape
    assert _relerr(lg, ref["logvalue"]) < 1e-10
    assert np.abs(W - ref["W"]).max() < 1e-8 and np.abs(C - ref["C"]).max() < 1e-8
    Pref = np.array([[pp[k] for k in ("B_T", "sigX", "sigY", "sigH", "sigT")] for pp in ref["params"]])
    assert _relerr(P, Pref) < 1e-8
