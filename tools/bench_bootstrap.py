"""Time one bootstrap replicate (ppls_xprod_resample) at the benchmark shapes.

    python tools/bench_bootstrap.py [c3,c5] [--reps 5] [--scale 1.0] [--outdir profiles]

Per configuration (C3: n = 1e6, p = q = 2000, r = 5, fp64; C5: n = 5e5, p = 1e4, q = 500, r = 10, fp32
storage) one context with the synthetic data of bench.py, and one JSON file
``<outdir>/bootstrap_<config>.json`` with, all from the same process and the same rows:

gram_ms            the unweighted joint Gram's kernel time, ``gram(2)`` (HIP events), every repeat
gram_weighted_ms   the weighted instantiation's, with counts from ``bootstrap_counts``, interleaved
                   with the unweighted launches
ratio              median weighted / median unweighted, beside ``gram_spread``, the unweighted
                   kernel's own (max - min) / median over the repeats: the yardstick for the ratio
replicate          whole replicates, wall clock: draw (``bootstrap_counts``), resample (upload of the
                   counts, weighted Gram, finish, traces) and a 100-step warm-started fit from S
hbm                bytes in use with the data resident, with S and the replicate context, and the peak
                   seen after a replicate

--scale s multiplies n by s (a quick run on a smaller problem; the JSON records it).
"""
import argparse
import ctypes as ct
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ppls_amd import Context, bootstrap_counts  # noqa: E402

SEED = 20261020
_HIP = ct.CDLL("libamdhip64.so")


def hbm_used():
    free, total = ct.c_size_t(), ct.c_size_t()
    if _HIP.hipMemGetInfo(ct.byref(free), ct.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return total.value - free.value


def run(name, reps, scale, fit_steps=100):
    cfg = bench.CONFIGS[name]
    n, p, q, r = max(8, int(cfg["n"] * scale)), cfg["p"], cfg["q"], cfg["r"]
    truth, th0 = bench.make_truth_and_theta0(p, q, r)
    rng = np.random.default_rng(SEED)
    out = dict(config=name, n=n, p=p, q=q, r=r, storage=cfg.get("storage", "f64"), scale=scale, reps=reps,
               fit_steps=fit_steps)
    base = hbm_used()
    with Context(0) as ctx, Context(0) as work:
        if cfg.get("storage") == "f32":
            ctx.set_option("dtype", 1)
        ctx.generate_synthetic(n, p, q, truth, seed=SEED)
        ctx.set_option("xprod", 1)
        hbm = dict(before=base, data=hbm_used())
        # the estimates a replicate is warm-started from: a fit of the data themselves
        est = ctx.em_run(th0, fit_steps, -np.inf, want_eout=False, want_mu=False)[0]
        counts = bootstrap_counts(n, reps + 1, rng)
        g, gw = [], []
        for b in range(reps + 1):          # the first pair warms up (queue, clocks) and is dropped
            g.append(ctx.gram(2, 0, want=False)[1])
            gw.append(ctx.gram(2, 0, want=False, count=counts[b])[1])
        g, gw = g[1:], gw[1:]
        med = statistics.median(g)
        out.update(gram_ms=g, gram_weighted_ms=gw, ratio=statistics.median(gw) / med,
                   gram_spread=(max(g) - min(g)) / med, gram_weighted_spread=(max(gw) - min(gw)) / statistics.median(gw),
                   occupancy=dict(unweighted=ctx.gram_occupancy(cfg.get("storage") == "f32"),
                                  weighted=ctx.gram_occupancy(cfg.get("storage") == "f32", weighted=True)))
        rep = []
        for b in range(reps + 1):          # the first replicate allocates S, the counts and the partials
            t0 = time.perf_counter()
            c = bootstrap_counts(n, 1, rng)[0]
            t1 = time.perf_counter()
            work.xprod_resample(ctx, c)
            t2 = time.perf_counter()
            ll = work.em_run(est, fit_steps, -np.inf, want_eout=False, want_mu=False)[1]
            work.synchronize()
            t3 = time.perf_counter()
            rep.append(dict(draw_ms=1e3 * (t1 - t0), resample_ms=1e3 * (t2 - t1), fit_ms=1e3 * (t3 - t2),
                            total_ms=1e3 * (t3 - t0), steps=int(len(ll))))
            hbm["peak_seen"] = max(hbm.get("peak_seen", 0), hbm_used())
        hbm["with_S_and_replicate_context"] = hbm_used()
        out["first_replicate"] = rep[0]
        out["replicate"] = rep[1:]
        out["replicate_median_ms"] = {k: statistics.median(x[k] for x in rep[1:])
                                      for k in ("draw_ms", "resample_ms", "fit_ms", "total_ms")}
        out["hbm"] = hbm
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="?", default="c3,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    for name in args.configs.split(","):
        res = run(name, args.reps, args.scale)
        path = os.path.join(args.outdir, f"bootstrap_{name}.json")
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({k: res[k] for k in ("config", "n", "ratio", "gram_spread", "replicate_median_ms", "hbm")}),
              flush=True)


if __name__ == "__main__":
    main()
