"""Time the pieces of the robust fit (robust_PPLS_simult) at the benchmark shapes.

    python tools/bench_robust.py [c3,c5] [--reps 5] [--scale 1.0] [--outer 10] [--outdir profiles]

One process per configuration (C3: n = 1e6, p = q = 2000, fp64; C5: n = 5e5, p = 1e4, q = 500, fp32 storage),
the synthetic data of bench.py, five repeats after a warm-up, one JSON file ``<outdir>/robust_<config>.json``:

gram_ms, gram_count_ms, gram_real_ms
                   kernel time (HIP events) of the joint Gram: unweighted, count-weighted (bootstrap counts) and
                   real-weighted (weights (nu + P) / (nu + chi2_P)), the same rows, alternating.
                   ``real_over_count`` = the medians' ratio (target: within 1 %), ``*_spread`` = (max - min) /
                   median of each, ``occupancy`` of the three instantiations
weight_kernel      the weights and t log-likelihood kernels alone (``robust_timing``) for one and 16 nu, with the
                   GB/s of the 24 B read + 16 B written per row
outer              one outer iteration at a = 5, wall clock per piece: ``robust_weights`` (distance pass, weight
                   kernel, reduction, copy-out of l_t), ``xprod_weighted`` (weighted Gram, finish, traces) and
                   five EM steps on the work context
fit                a whole ``PPLS_simult(., ., 5, 10, init = bench's theta0)`` and a whole
                   ``robust_PPLS_simult(., ., 5, outer = --outer, init = that fit)`` on the same context, wall
                   clock, with the steps taken
hbm                bytes in use: before, with the rows resident, after the robust fit (rows, the work context's
                   S and partials, the weights and distances)

--scale s multiplies n by s (a quick run on a smaller problem; the JSON records it).
"""
import argparse
import ctypes as ct
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ppls_amd import Context, PPLS_simult, bootstrap_counts, robust_PPLS_simult  # noqa: E402

SEED = 20261020
NU = 4.0
A = 5
_HIP = ct.CDLL("libamdhip64.so")


def hbm_used():
    free, total = ct.c_size_t(), ct.c_size_t()
    if _HIP.hipMemGetInfo(ct.byref(free), ct.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return total.value - free.value


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def run(name, reps, scale, outer):
    cfg = bench.CONFIGS[name]
    n, p, q = max(8, int(cfg["n"] * scale)), cfg["p"], cfg["q"]
    truth, th0 = bench.make_truth_and_theta0(p, q, A)
    rng = np.random.default_rng(SEED)
    f32 = cfg.get("storage") == "f32"
    out = dict(config=name, n=n, p=p, q=q, a=A, nu=NU, storage=cfg.get("storage", "f64"), scale=scale, reps=reps)
    hbm = dict(before=hbm_used())
    with Context(0) as ctx, Context(0) as work:
        if f32:
            ctx.set_option("dtype", 1)
        ctx.generate_synthetic(n, p, q, truth, seed=SEED)
        ctx.set_option("xprod", 1)
        hbm["data"] = hbm_used()
        # (a) the three instantiations of the Gram kernel on the same rows, alternating
        cnt = bootstrap_counts(n, 1, rng)[0]
        w = (NU + p + q) / (NU + rng.chisquare(p + q, n))
        g0, gc, gr = [], [], []
        for _ in range(reps + 1):          # the first round warms up (queue, clocks) and is dropped
            g0.append(ctx.gram(2, 0, want=False)[1])
            gc.append(ctx.gram(2, 0, want=False, count=cnt)[1])
            gr.append(ctx.gram(2, 0, want=False, weight=w)[1])
        g0, gc, gr = g0[1:], gc[1:], gr[1:]
        out.update(gram_ms=g0, gram_count_ms=gc, gram_real_ms=gr,
                   real_over_count=statistics.median(gr) / statistics.median(gc),
                   real_over_unweighted=statistics.median(gr) / statistics.median(g0),
                   gram_spread=spread(g0), gram_count_spread=spread(gc), gram_real_spread=spread(gr),
                   occupancy=dict(unweighted=ctx.gram_occupancy(f32), count=ctx.gram_occupancy(f32, weighted=True),
                                  real=ctx.gram_occupancy(f32, weighted="real")))
        # (b) the weight kernel alone
        tm = ctx.robust_timing(20)
        out["weight_kernel"] = dict(tm, gbps1=40.0 * n / tm["ms1"] / 1e6, gbps16=40.0 * n / tm["ms16"] / 1e6)
        # (c) the Gaussian fit, one outer iteration by pieces, the whole robust fit
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            gauss = PPLS_simult(None, None, A, 10, 1e-4, init=th0.as_dict(), ctx=ctx)
            ctx.synchronize()
            t_gauss = time.perf_counter() - t0
        from ppls_amd import Theta
        e = gauss["estimates"]
        th = Theta(e["W"], e["C"], e["B"], e["sigE"], e["sigF"], e["sigH"], e["sigT"])
        pieces = []
        for _ in range(reps + 1):          # the first allocates S, the partials and the weights
            t0 = time.perf_counter()
            ctx.robust_weights(th, NU)
            t1 = time.perf_counter()
            work.xprod_weighted(ctx)
            t2 = time.perf_counter()
            work.em_run(th, 5, -np.inf, want_eout=False, want_mu=False)
            work.synchronize()
            t3 = time.perf_counter()
            pieces.append(dict(weights_ms=1e3 * (t1 - t0), xprod_ms=1e3 * (t2 - t1), em5_ms=1e3 * (t3 - t2),
                               total_ms=1e3 * (t3 - t0)))
        out["outer_first"] = pieces[0]
        out["outer"] = pieces[1:]
        out["outer_median_ms"] = {k: statistics.median(x[k] for x in pieces[1:]) for k in pieces[0]}
        t0 = time.perf_counter()
        fit = robust_PPLS_simult(None, None, A, NU, outer=outer, init=e, ctx=ctx, work=work)
        t_rob = time.perf_counter() - t0
        out["fit"] = dict(gaussian_s=t_gauss, gaussian_steps=int(len(gauss["loglik"])), robust_s=t_rob,
                          robust_steps=int(fit["steps"]), converged=bool(fit["converged"]), outer_cap=outer,
                          loglik_first=float(fit["loglik"][0]), loglik_last=float(fit["loglik"][-1]),
                          sum_w_over_n=float(fit["weights"].sum() / n))
        hbm["after_robust_fit"] = hbm_used()
        out["hbm"] = hbm
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="?", default="c3,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--outer", type=int, default=10)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--one", action="store_true", help="run the single named configuration in this process")
    args = ap.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    if not args.one:                       # one fresh process per configuration
        for name in args.configs.split(","):
            subprocess.run([sys.executable, os.path.abspath(__file__), name, "--one", "--reps", str(args.reps), "--scale",
                            str(args.scale), "--outer", str(args.outer), "--outdir", args.outdir], check=True)
        return
    res = run(args.configs, args.reps, args.scale, args.outer)
    with open(os.path.join(args.outdir, f"robust_{args.configs}.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps({k: res.get(k) for k in ("config", "n", "real_over_count", "real_over_unweighted", "gram_count_spread",
                                               "gram_real_spread", "occupancy", "weight_kernel", "outer_median_ms", "fit",
                                               "hbm")}), flush=True)


if __name__ == "__main__":
    main()
