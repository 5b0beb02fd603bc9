"""meta_EMstep / meta_PPLSi from per-population cross-products on the GPU (ppls_xprod_meta.hip;
DESIGN §18): the statistics kernel against long-double statistics, the streamed fit against the
oracle, option meta_xprod on resident rows, both of them sharded, and the states the calls refuse.

Tolerances of the fits are those of tests/test_gpu_meta.py's golden test: log-likelihoods 1e-10
relative, loadings 1e-8 absolute, parameters 1e-8 relative, Cxt / Cyu 1e-9 relative, steps exact.
The kernel's bar is a priori (tests/meta_xprod_bar.py).
"""
import functools
import json
import os
import threading

import numpy as np
import pytest

from conftest import make_problem
from meta_xprod_bar import MetaReference, pop_params
from oracle import ppls_oracle as o
from sweep_bar import padded_width, sweep_problem

pytestmark = pytest.mark.gpu

E_ARG, E_NUMERIC, E_STATE = -1, -3, -4
GOLD = os.path.join(os.path.dirname(__file__), "golden")
META = sorted(f for f in os.listdir(GOLD) if f.startswith("meta_") and f.endswith(".npz"))
RWS = (0, 1, 2, 4, 8)


def _ctx():
    from ppls_amd import Context
    return Context(0)


def _relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _sizes(n, K):
    """K unequal populations over n rows, one of them of 2 rows."""
    head = [2, n // 4, n // 13, n // 3 + 1][:K - 1]
    return head + [n - sum(head)]


def _labels(sizes, seed):
    """Interleaved labels: a seeded shuffle of the populations' labels."""
    lab = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return np.random.default_rng(seed).permutation(lab)


def _chunks(n):
    """Three uneven chunks."""
    return [0, n // 5, n // 5 + n // 2 + 1, n]


def _stream(c, X, Y, labels, K, center, scale):
    c.stream_begin(X.shape[1], Y.shape[1], center, scale, nr_folds=K)
    b = _chunks(X.shape[0])
    for lo, hi in zip(b[:-1], b[1:]):
        c.stream_rows(X[lo:hi], Y[lo:hi], labels[lo:hi])
    return c.stream_end()


# ------------------------------------------------------------------------------ 1. the kernel
# p, q at the padding and tile boundaries: one column each; odd widths; P < 128; ldx exactly one
# 128-column step and ldy one step plus 2; more than two steps with a narrow Y; 600 columns
SHAPES = [(1, 1), (3, 2), (9, 12), (127, 130), (257, 5), (600, 7)]


def _kernel_case(p, q, K, n):
    from ppls_amd._lib import lib
    from ppls_amd.api import rank1_mu_coefficients
    X, Y, th = sweep_problem(n, p, q, 1, seed=1000 * p + 10 * q + K)
    sizes = _sizes(n, K)
    labels = _labels(sizes, seed=n + K)
    w, cc = th["W"][:, 0], th["C"][:, 0]
    params = pop_params(K)
    coef = rank1_mu_coefficients(params)
    with _ctx() as c, _ctx() as c2:
        out = _stream(c, X, Y, labels, K, False, False)
        assert list(out["fold_total"]) == sizes
        _stream(c2, X, Y, labels, K, False, False)
        S = [c.stream_fold_get(k)[0] for k in range(K)]      # what the device holds: the Gram's rounding
        ref = MetaReference(S, p, q, w, cc, coef)            # is not charged to this kernel
        P = padded_width(p) + padded_width(q)
        nt = lib().ppls_xprod_meta_nt(K, P)
        worst = dict(SX=0.0, SY=0.0, G=0.0)
        for rw in RWS:
            c.set_option("xprod_rw", rw)
            c2.set_option("xprod_rw", rw)
            SX, SY, G = c.xprod_meta_stats(w, cc, params)
            r = ref.ratios(SX, SY, G)
            print(f"({p},{q}) K={K} rw={rw} nt={nt}: err / bar {r}")
            assert max(r.values()) <= 1.0, (rw, r)
            worst = {k: max(worst[k], r[k]) for k in r}
            assert np.array_equal(G, np.transpose(G, (0, 2, 1)))               # exactly symmetric
            again = c.xprod_meta_stats(w, cc, params)
            other = c2.xprod_meta_stats(w, cc, params)
            for a, b, d in zip((SX, SY, G), again, other):
                assert np.array_equal(a, b) and np.array_equal(a, d)            # the same bits
    return nt, worst


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("p,q", SHAPES)
def test_kernel_inside_the_long_double_bar(p, q, K):
    nt, _ = _kernel_case(p, q, K, 150)
    assert nt == 0


def test_kernel_non_temporal_instantiation():
    """K = 5, (p, q) = (2000, 300), n = 60: P = 2300 and 5 x 8 x 2300^2 = 211.6 MB, just above the
    200 MiB (209.7 MB) the cache policy applies to the total -- one matrix alone (42 MB), which the
    single-matrix kernel's test looks at, would stay on the cached path, and so do K = 4."""
    from ppls_amd._lib import lib
    assert lib().ppls_xprod_meta_nt(4, 2300) == 0 and lib().ppls_xprod_meta_nt(1, 2300) == 0
    nt, _ = _kernel_case(2000, 300, 5, 60)
    assert nt == 1


# ------------------------------------------------------------------------------ 2. streamed fit
P37, Q29, N997 = 37, 29, 997
POPS = {"K4": [300, 250, 200, 247], "tiny_pops": [3, 500, 2, 492],
        # 16 populations as equal as 997 rows allow: five of 63 rows, eleven of 62
        "K16": [63] * 5 + [62] * 11}


@functools.lru_cache(maxsize=None)
def _fit_problem(name, seed=6):
    """Raw rows with interleaved labels, and the rows R's scale() gives (numpy, ddof = 1) stably
    sorted by label: what meta_PPLSi(scale(X), scale(Y), Ipopu) fits."""
    sizes = POPS[name]
    X, Y, _ = make_problem(N997, P37, Q29, 1, seed=seed)
    labels = _labels(sizes, seed=len(sizes))
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    Ys = (Y - Y.mean(0)) / Y.std(0, ddof=1)
    order = np.argsort(labels, kind="stable")
    out = (X, Y, labels, Xs[order], Ys[order])
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_fit(name, steps, atol):
    _, _, _, Xs, Ys = _fit_problem(name)
    return o.meta_pplsi(Xs, Ys, POPS[name], steps, atol, o.initial_guess(P37, Q29, "equal"))


def _check_fit(got, ref):
    W, C, P, lg = got
    assert lg.shape == ref["logvalue"].shape
    assert _relerr(lg, ref["logvalue"]) < 1e-10
    assert np.abs(W - ref["W"]).max() < 1e-8 and np.abs(C - ref["C"]).max() < 1e-8
    Pr = np.array([[pp[k] for k in ("B_T", "sigX", "sigY", "sigH", "sigT")] for pp in ref["params"]])
    assert _relerr(P, Pr) < 1e-8


@pytest.mark.parametrize("name", list(POPS))
def test_streamed_fit_matches_oracle(name):
    X, Y, labels, _, _ = _fit_problem(name)
    ref = _oracle_fit(name, 15, -np.inf)
    with _ctx() as c:
        _stream(c, X, Y, labels, len(POPS[name]), True, True)
        got = c.meta_ppls_stream(15, -np.inf, o.initial_guess(P37, Q29, "equal"))
        assert c.meta_info() == "device_stream"
    assert got[3].shape[0] == 16
    _check_fit(got, ref)


def test_streamed_fit_stops_where_the_oracle_stops():
    """A finite atol: the same step count.  Precondition, from the oracle's own trace: the increments
    at the stop step and at the step before are a factor >= 10 away from atol, so rounding cannot
    move the stop."""
    import ppls_amd
    atol = 1e5
    X, Y, labels, _, _ = _fit_problem("K4")
    ref = _oracle_fit("K4", 15, atol)
    inc = np.diff(ref["logvalue"].sum(axis=1))
    stop = len(inc)
    assert 2 <= stop < 15 and inc[stop - 1] <= atol / 10 and inc[stop - 2] >= 10 * atol, inc
    with _ctx() as c:
        ppls_amd.stream_data([(X[lo:hi], Y[lo:hi], labels[lo:hi]) for lo, hi in zip(_chunks(N997)[:-1], _chunks(N997)[1:])],
                             ctx=c, nr_folds=4)
        f = ppls_amd.meta_PPLSi(None, None, None, EMsteps=15, atol=atol, initialGuess="equal", ctx=c)
    assert f["logvalue"].shape[0] - 1 == stop and f["log"].shape == (stop, 4)
    _check_fit((f["W"], f["C"], np.array([[pp[k] for k in ("B_T", "sigX", "sigY", "sigH", "sigT")] for pp in f["params"]]),
                f["logvalue"]), ref)


def test_streamed_emstep_matches_oracle():
    import ppls_amd
    X, Y, labels, Xs, Ys = _fit_problem("K4")
    sizes = POPS["K4"]
    init = o.initial_guess(P37, Q29, "equal")
    params = [dict(B_T=1.0 + 0.1 * j, sigX=0.9 + 0.05 * j, sigY=0.8 + 0.02 * j, sigH=0.3 + 0.01 * j, sigT=1.1 - 0.05 * j)
              for j in range(4)]
    ref = o.meta_emstep(Xs, Ys, init["W"], init["C"], sizes, params)
    with _ctx() as c:
        _stream(c, X, Y, labels, 4, True, True)
        f = ppls_amd.meta_EMstep(None, None, init["W"], init["C"], None, params, ctx=c)
    assert np.abs(f["W."][:, 0] - ref["W"]).max() < 1e-8 and np.abs(f["C."][:, 0] - ref["C"]).max() < 1e-8
    for g, r in zip(f["pops"], ref["pops"]):
        assert _relerr(g["B"], r["B"]) < 1e-8
        assert _relerr(g["sighat"], r["sighat"]) < 1e-8 and _relerr(g["siglathat"], r["siglathat"]) < 1e-8
        assert _relerr(g["Cxt"], r["Cxt"]) < 1e-9 and _relerr(g["Cyu"], r["Cyu"]) < 1e-9


# ------------------------------------------------------------------------------ 3. resident meta_xprod = 1
def _init(g):
    s = g["init_s"]
    return dict(W=g["init_W"], C=g["init_C"], B=s[0], sigE=s[1], sigF=s[2], sigH=s[3], sigT=s[4])


@pytest.mark.parametrize("name", META)
def test_resident_option_matches_golden(name):
    g = np.load(os.path.join(GOLD, name))
    meta = json.loads(str(g["meta"]))
    with _ctx() as c:
        c.set_option("meta_xprod", 1)
        c.set_data(g["X"], g["Y"])
        W, C, P, lg = c.meta_ppls(meta["sizes"], meta["EMsteps"], meta["atol"], _init(g))
        assert c.meta_info() == "device_xprod"
        s = g["init_s"]
        K = len(meta["sizes"])
        W1, C1, P1, cxt, cyu = c.meta_emstep(g["init_W"], g["init_C"], meta["sizes"], np.tile(s[:5], (K, 1)))
        assert c.meta_xprod_info()["formations"] == 1
    assert lg.shape[0] - 1 == meta["steps"]
    assert _relerr(lg, g["logvalue"]) < 1e-10
    assert np.abs(W - g["W"]).max() < 1e-8 and np.abs(C - g["C"]).max() < 1e-8
    assert _relerr(P, g["params"]) < 1e-8
    assert np.abs(W1 - g["step1_W"]).max() < 1e-8 and np.abs(C1 - g["step1_C"]).max() < 1e-8
    assert _relerr(P1, g["step1_params"]) < 1e-8
    assert _relerr(cxt, g["step1_Cxt"]) < 1e-9 and _relerr(cyu, g["step1_Cyu"]) < 1e-9


@pytest.mark.parametrize("storage", ["f64", "f32", "wide"])
def test_resident_option_on_equals_off(storage):
    sizes = [300, 250, 200, 247]
    p, q = (4200, 29) if storage == "wide" else (37, 29)
    X, Y, _ = make_problem(sum(sizes), p, q, 1, seed=997)
    if storage == "f32":
        X = X.astype(np.float32).astype(np.float64)
        Y = Y.astype(np.float32).astype(np.float64)
    init = o.initial_guess(p, q, "equal")
    with _ctx() as c:
        c.set_option("dtype", 1 if storage == "f32" else 0)
        c.set_data(X, Y)
        off = c.meta_ppls(sizes, 40, 1e-6, init)
        assert c.meta_info() == ("device_split" if storage == "f64" else "device_panel")
        assert c.meta_xprod_info() == dict(npop=0, formations=0, form_ms=0.0)
        c.set_option("meta_xprod", 1)
        on = c.meta_ppls(sizes, 40, 1e-6, init)
        assert c.meta_info() == "device_xprod"
        info = c.meta_xprod_info()
        assert info["npop"] == 4 and info["formations"] == 1 and info["form_ms"] > 0.0
    assert on[3].shape == off[3].shape
    assert _relerr(on[3], off[3]) < 1e-10
    assert np.abs(on[0] - off[0]).max() < 1e-8 and np.abs(on[1] - off[1]).max() < 1e-8
    assert _relerr(on[2], off[2]) < 1e-8


def test_resident_cache_is_kept_and_dropped():
    sizes = [60, 25, 75]
    X, Y, th0 = make_problem(160, 13, 9, 1, seed=41)
    init = o.initial_guess(13, 9, "equal")
    other = dict(W=th0["W"][:, 0], C=th0["C"][:, 0], B=0.9, sigE=0.7, sigF=0.6, sigH=0.4, sigT=1.2)
    with _ctx() as c:
        c.set_option("meta_xprod", 1)
        c.set_data(X, Y)
        first = c.meta_ppls(sizes, 10, -np.inf, init)
        assert c.meta_xprod_info()["formations"] == 1
        c.meta_ppls(sizes, 12, 1e-3, other)                      # other starting values, steps, atol
        again = c.meta_ppls(sizes, 10, -np.inf, init)
        SX, SY, G = c.xprod_meta_stats(init["W"], init["C"], pop_params(3))     # the debug entry reads them too
        assert c.meta_xprod_info() == dict(npop=3, formations=1, form_ms=c.meta_xprod_info()["form_ms"])
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        assert SX.shape == (3, 13) and SY.shape == (3, 9) and np.array_equal(G, np.transpose(G, (0, 2, 1)))
        c.meta_ppls([85, 75], 5, -np.inf, init)                  # other populations: formed again
        assert c.meta_xprod_info()["formations"] == 2 and c.meta_xprod_info()["npop"] == 2
        c.scale_data(True, True)                                 # the data change: dropped
        assert c.meta_xprod_info()["npop"] == 0
        c.meta_ppls([85, 75], 5, -np.inf, init)
        assert c.meta_xprod_info()["formations"] == 3
        c.set_data(X, Y)
        assert c.meta_xprod_info()["npop"] == 0
        c.meta_ppls(sizes, 5, -np.inf, init)
        assert c.meta_xprod_info()["formations"] == 4 and c.meta_xprod_info()["npop"] == 3
        c.set_option("meta_xprod", 0)                            # the option goes to 0: dropped
        assert c.meta_xprod_info()["npop"] == 0
        c.meta_ppls(sizes, 5, -np.inf, init)
        assert c.meta_info() == "device_split" and c.meta_xprod_info()["formations"] == 4


def test_resident_single_population_equals_pplsi():
    import ppls_amd
    X, Y, _ = make_problem(160, 13, 9, 1, seed=41)
    init = o.initial_guess(13, 9, "equal")
    with _ctx() as c:
        c.set_option("meta_xprod", 1)
        m = ppls_amd.meta_PPLSi(X, Y, np.zeros(160), EMsteps=30, atol=1e-6, customGuess=init, ctx=c)
        assert c.meta_info() == "device_xprod"
        a = ppls_amd.PPLSi(X, Y, EMsteps=30, atol=1e-6, customGuess=init, ctx=c)
    assert m["logvalue"].shape[0] - 1 == a["Number_steps"]
    assert _relerr(m["logvalue"][:, 0], a["logvalue"]) < 1e-12
    assert np.abs(m["W"] - a["W"]).max() < 1e-10


# ------------------------------------------------------------------------------ 4. sharded
class ThreadAllReduce:
    """Sum over k host threads in rank order (tests/test_gpu_multirank.py's): every rank gets the
    bitwise-same result; a bounded barrier, so a missed collective fails instead of hanging."""

    def __init__(self, k):
        self.bar = threading.Barrier(k, timeout=60)
        self.bufs = [None] * k

    def fn(self, rank):
        def reduce(buf):
            self.bufs[rank] = buf.copy()
            self.bar.wait()
            tot = self.bufs[0].copy()
            for b in self.bufs[1:]:
                tot += b
            self.bar.wait()
            buf[:] = tot
        return reduce


def _run_ranks(k, work):
    """work(rank, ctx) on k threads, each with its own context on GPU 0 and the host reducer."""
    red = ThreadAllReduce(k)
    out, errs = [None] * k, []

    def body(rank):
        try:
            with _ctx() as c:
                c.set_reducer(red.fn(rank))
                out[rank] = work(rank, c)
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            red.bar.abort()

    ths = [threading.Thread(target=body, args=(i,)) for i in range(k)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ths), "a rank is stuck in a collective"
    if errs:
        raise errs[0]
    return out


@pytest.mark.parametrize("k", [2, 3])
def test_sharded_stream_every_rank_the_same_bits(k):
    n, p, q, sizes = 300, 12, 9, [120, 30, 150]
    X, Y, _ = make_problem(n, p, q, 1, seed=15)
    labels = _labels(sizes, seed=k)
    init = o.initial_guess(p, q, "equal")
    late = np.arange(150, n)
    # rank 0: two chunks, all populations; rank 1: no row of population 0; rank 2 (k = 3): no rows
    chunks = [[np.arange(0, 1), np.r_[np.arange(1, 150), late[labels[late] == 0]]], [late[labels[late] != 0]], []][:k]

    def work(rank, c):
        c.stream_begin(p, q, True, True, nr_folds=3)
        for idx in chunks[rank]:
            c.stream_rows(X[idx], Y[idx], labels[idx])
        c.stream_end()
        return c.meta_ppls_stream(20, 1e-6, init)

    res = _run_ranks(k, work)
    with _ctx() as one:
        one.stream_begin(p, q, True, True, nr_folds=3)
        for ch in chunks:
            for idx in ch:
                one.stream_rows(X[idx], Y[idx], labels[idx])
        one.stream_end()
        ref = one.meta_ppls_stream(20, 1e-6, init)
    for m in res:
        for a, b in zip(m, res[0]):
            assert np.array_equal(a, b)                                        # every rank: the same bits
    W, C, P, lg = res[0]
    assert lg.shape == ref[3].shape and _relerr(lg, ref[3]) < 1e-10
    assert np.abs(W - ref[0]).max() < 1e-8 and np.abs(C - ref[1]).max() < 1e-8
    assert _relerr(P, ref[2]) < 1e-8


@pytest.mark.parametrize("k", [2, 3])
def test_sharded_resident_option_equals_unsharded(k):
    """Populations [200, 100, 600] over k equal shards of 900 rows: populations 0 and 1 lie wholly on
    rank 0, and every other rank holds rows of population 2 alone."""
    from ppls_amd import Context
    n, p, q, sizes = 900, 60, 40, [200, 100, 600]
    X, Y, _ = make_problem(n, p, q, 1, seed=5)
    init = o.initial_guess(p, q, "equal")
    with _ctx() as c:
        c.set_option("meta_xprod", 1)
        c.set_data(X, Y)
        ref = c.meta_ppls(sizes, 30, 1e-6, init)

    def work(rank, c):
        r0, nl = Context.shard_range(n, k, rank)
        c.set_option("meta_xprod", 1)
        c.set_data(X[r0:r0 + nl], Y[r0:r0 + nl], n_total=n)
        c.row0 = r0
        loc, _ = c.pop_rows(sizes)
        return c.meta_ppls(sizes, 30, 1e-6, init), list(loc), c.meta_info()

    res = _run_ranks(k, work)
    assert res[0][1][:2] == [200, 100] and all(r[1][:2] == [0, 0] for r in res[1:])
    for m, _, path in res:
        assert path == "device_xprod"
        for a, b in zip(m, res[0][0]):
            assert np.array_equal(a, b)
    W, C, P, lg = res[0][0]
    assert lg.shape == ref[3].shape and _relerr(lg, ref[3]) < 1e-10
    assert np.abs(W - ref[0]).max() < 1e-8 and np.abs(C - ref[1]).max() < 1e-8
    assert _relerr(P, ref[2]) < 1e-8


# ------------------------------------------------------------------------------ 5. states and refusals
def _refused(fn):
    from ppls_amd import PplsError
    with pytest.raises(PplsError) as e:
        fn()
    return e.value.code


def test_states_and_refusals():
    import ppls_amd
    from ppls_amd import Theta
    n, p, q, K = 120, 12, 9, 3
    X, Y, th0 = make_problem(n, p, q, 2, seed=2)
    labels = _labels([50, 30, 40], seed=1)
    init = o.initial_guess(p, q, "equal")
    params = pop_params(K)

    def both(c):
        return (_refused(lambda: c.meta_ppls_stream(5, 1e-4, init)),
                _refused(lambda: c.meta_emstep_stream(init["W"], init["C"], params)))

    with _ctx() as c:
        c.p, c.q = p, q
        assert both(c) == (E_STATE, E_STATE)                                    # no data
        c.set_data(X, Y)
        assert both(c) == (E_STATE, E_STATE)                                    # resident rows
        assert _refused(lambda: c.xprod_meta_stats(init["W"], init["C"], params)) == E_STATE
        c.stream_begin(p, q, True, True)
        c.stream_rows(X, Y)
        assert both(c) == (E_STATE, E_STATE)                                    # an open stream
        c.stream_end()
        assert both(c) == (E_STATE, E_STATE)                                    # a plain stream
        c.stream_begin(p, q, True, True, nr_folds=K)
        c.stream_rows(X[:70], Y[:70], labels[:70])
        assert both(c) == (E_STATE, E_STATE)                                    # an open fold stream
        c.stream_rows(X[70:], Y[70:], labels[70:])
        c.stream_end()
        # the resident calls keep refusing a streamed context
        assert _refused(lambda: c.meta_ppls([50, 30, 40], 5, 1e-4, init)) == E_STATE
        assert _refused(lambda: c.meta_emstep(init["W"], init["C"], [50, 30, 40], params)) == E_STATE
        with pytest.raises(ValueError):
            ppls_amd.meta_PPLSi(None, None, labels, EMsteps=5, ctx=c)
        with pytest.raises(ValueError):
            ppls_amd.meta_EMstep(None, None, init["W"], init["C"], labels, [dict(B_T=1.0, sigX=1.0, sigY=1.0, sigH=1.0,
                                                                                sigT=1.0)] * K, ctx=c)
        with pytest.raises(NotImplementedError):
            ppls_amd.meta_PPLSi(None, None, None, EMsteps=5, initialGuess="o2m", ctx=c)
        # an active ppls_em_begin session
        c.em_begin(Theta(th0["W"], th0["C"], th0["B"], th0["sigE"], th0["sigF"], th0["sigH"], th0["sigT"]))
        assert both(c) == (E_STATE, E_STATE)
        c.ppls(1, 3, 1e-4, [init])                                              # ends the session
        # the selection is neither needed nor changed
        c.stream_select(2)
        rmsep0 = ppls_amd.cv_PPLS(None, None, 2, K, ctx=c, per_fold=True, EMsteps=10, atol=-1.0)[1]
        c.stream_select(2)
        sel = c.meta_ppls_stream(8, -np.inf, init)
        assert c.stream_fold_info()["selected"] == 2 and c.n_total == n - 40
        rmsep1 = ppls_amd.cv_PPLS(None, None, 2, K, ctx=c, per_fold=True, EMsteps=10, atol=-1.0)[1]
        assert np.array_equal(rmsep0, rmsep1, equal_nan=True) and np.isfinite(rmsep0).any()
        allf = c.meta_ppls_stream(8, -np.inf, init)                             # (cv_PPLS ends selected on -1)
        assert c.stream_fold_info()["selected"] == -1
        for a, b in zip(sel, allf):
            assert np.array_equal(a, b)                                         # whatever is selected
        # a NaN increment: coefficients that overflow (sigE = 1e-170: 1 / sigE^2 = Inf)
        bad = dict(init, sigE=1e-170)
        assert _refused(lambda: c.meta_ppls_stream(5, 1e-4, bad)) == E_NUMERIC
        ok = c.meta_ppls_stream(8, -np.inf, init)                               # and the context still fits
        for a, b in zip(ok, allf):
            assert np.array_equal(a, b)
