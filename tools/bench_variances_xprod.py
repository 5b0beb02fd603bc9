"""Time ppls_variances_xprod against ppls_variances at a benchmark shape.

    python tools/bench_variances_xprod.py c3|c5 [--reps 5] [--scale 1.0] [--outdir profiles]

One process per configuration (C3: p = q = 2000, a = 5; C5: p = 1e4, q = 500, a = 10, fp32 storage; "X"),
on bench.py's synthetic rows with S prepared, and one JSON file ``<outdir>/variances_xprod_<config>.json``:

xprod_ms, rows_ms    the whole ``variances_xprod`` call and the whole ``variances`` call (unchanged from
                     before; mu from ``estep``, S ready), wall clock around calls that end synchronised,
                     alternating, after one untimed pair; both return varMatrix and seLoad, neither
                     SSt_exp / SSt_star
ratio                median xprod / median rows, beside ``rows_spread`` = (max - min) / median of the rows
                     call over the repeats: the yardstick for the ratio
estep_ms             the ``estep`` that produces the rows call's mu (not part of either figure)
kernel_ms            the information kernel (all components, one launch) and the launches it replaces
                     (block copy out of S, a varmat kernels, batch copy, negate), HIP events, per repeat
hbm                  bytes in use with the data and S resident, and in use after each kind of call has returned
                     (its batch and scratch are freed by then: not a high-water mark; the largest over the repeats)

--scale s multiplies n by s (the p x p work does not depend on n; the JSON records it).
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
from ppls_amd import Context  # noqa: E402

SEED = 20261020
_HIP = ct.CDLL("libamdhip64.so")


def hbm_used():
    free, total = ct.c_size_t(), ct.c_size_t()
    if _HIP.hipMemGetInfo(ct.byref(free), ct.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return total.value - free.value


def run(name, reps, scale, em_steps=3):
    cfg = bench.CONFIGS[name]
    n, p, q, r = max(8, int(cfg["n"] * scale)), cfg["p"], cfg["q"], cfg["r"]
    truth, th0 = bench.make_truth_and_theta0(p, q, r)
    out = dict(config=name, n=n, p=p, q=q, r=r, storage=cfg.get("storage", "f64"), scale=scale, reps=reps)
    base = hbm_used()
    with Context(0) as ctx:
        if cfg.get("storage") == "f32":
            ctx.set_option("dtype", 1)
        ctx.generate_synthetic(n, p, q, truth, seed=SEED)
        ctx.xprod_prepare()
        hbm = dict(before=base, data_and_S=hbm_used())
        est = ctx.em_run(th0, em_steps, -np.inf, want_eout=False, want_mu=False)[0]
        t0 = time.perf_counter()
        e = ctx.estep(est, want_mu=True)
        out["estep_ms"] = 1e3 * (time.perf_counter() - t0)
        xp, rows = [], []
        for b in range(reps + 1):          # the first pair warms up (code objects, the rocBLAS handle) and is dropped
            t0 = time.perf_counter()
            W1, _, _, V1, se1, _, _ = ctx.variances_xprod(est, 0, full=False)
            t1 = time.perf_counter()
            hbm["in_use_after_xprod"] = max(hbm.get("in_use_after_xprod", 0), hbm_used())
            t2 = time.perf_counter()
            W0, _, V0, se0, _, _ = ctx.variances(e.mu_T, e.Ctt, est.sigE, 0, full=False)
            t3 = time.perf_counter()
            hbm["in_use_after_rows"] = max(hbm.get("in_use_after_rows", 0), hbm_used())
            xp.append(1e3 * (t1 - t0))
            rows.append(1e3 * (t3 - t2))
            print(f"pair {b}: xprod {xp[-1]:.1f} ms, rows {rows[-1]:.1f} ms", file=sys.stderr, flush=True)
        xp, rows = xp[1:], rows[1:]
        med = statistics.median(rows)
        out.update(xprod_ms=xp, rows_ms=rows, ratio=statistics.median(xp) / med, rows_spread=(max(rows) - min(rows)) / med,
                   xprod_spread=(max(xp) - min(xp)) / statistics.median(xp),
                   seLoad_rel_diff=float(np.abs(se1 - se0).max() / np.abs(se0).max()),
                   W_abs_diff=float(np.abs(W1 - W0).max()))
        del V0, V1
        k = [ctx.varinfo_timing(0, r, 5) for _ in range(reps)]
        out["kernel_ms"] = dict(varinfo=[a for a, _ in k], replaced=[b for _, b in k])
        # one launch: the block of S read once (p^2), J written (r p^2); the batch and the inverse's scratch
        out["bytes"] = dict(kernel_moved=8.0 * p * p * (1 + r), batch=8.0 * p * p * r)
        out["hbm"] = hbm
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(bench.CONFIGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    res = run(args.config, args.reps, args.scale)
    with open(os.path.join(args.outdir, f"variances_xprod_{args.config}.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
