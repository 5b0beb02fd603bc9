"""Time one permutation replicate (ppls_xprod_permute) at the benchmark shapes.

    python tools/bench_permute.py [c3,c5] [--reps 5] [--scale 1.0] [--outdir profiles] [--no-replicate]

Per configuration (C3: n = 1e6, p = q = 2000, r = 5, fp64; C5: n = 5e5, p = 1e4, q = 500, r = 10, fp32
storage) one context with the synthetic data of bench.py, and one JSON file
``<outdir>/permute_<config>.json`` with, all from the same process and the same rows:

gram_ms            the unweighted joint Gram's kernel time, ``gram(2)`` (HIP events), every repeat -- the
                   kernel ``xprod_prepare`` runs (``prepare_ms``: its own report, once), whose translation
                   unit this feature does not touch
perm_ms            the permuted cross block's kernel time, ``gram_permuted`` with permutations from
                   ``permutation_indices``, interleaved with the Gram launches
identity_ms        the same kernel with the identity permutation: what the gather itself costs
items              work items per row split: the block's 64 x 64 quadrants, and the joint Gram's live
                   lower-triangle quadrants; ``work_ratio`` their quotient, beside ``time_ratio``
                   (median perm / median Gram) and ``per_item_ratio`` = time_ratio / work_ratio
replicate          whole replicates, wall clock: draw (``permutation_indices``), permute (split by
                   ``xperm_timing`` into the host check, the index upload, kernel + finish) and
                   ``PPLS(., a, 100, 1e-4, "o2m_xprod")`` from S (C3 only by default)

--scale s multiplies n by s (a quick run on a smaller problem; the JSON records it).
"""
import argparse
import ctypes as ct
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ppls_amd import PPLS, Context, permutation_indices  # noqa: E402

SEED = 20261020
GT, GQ = 128, 64   # the joint Gram's tile and quadrant edges (ppls_variances.hip)


def joint_live_quadrants(p, q, ldx, P):
    """The joint Gram's work items per split: ppls_gram_quad_live over the lower tiles."""
    def live(a):   # whether the 16 columns [a, a + 16) hold any that can be non-zero
        return a < P and (a < p or (a + 16 > ldx and a < ldx + q))

    def side(t, w):
        return any(live(t * GT + w * GQ + a) for a in range(0, GQ, 16))
    nb = (P + GT - 1) // GT
    return sum(1 for I in range(nb) for J in range(I + 1) for wi in (0, 1) for wj in (0, 1)
               if not (I == J and wi == 0 and wj == 1) and side(I, wi) and side(J, wj))


def run(name, reps, scale, replicate, fit_steps=100):
    cfg = bench.CONFIGS[name]
    n, p, q, r = max(8, int(cfg["n"] * scale)), cfg["p"], cfg["q"], cfg["r"]
    truth, _ = bench.make_truth_and_theta0(p, q, r)
    rng = np.random.default_rng(SEED)
    f32 = cfg.get("storage") == "f32"
    out = dict(config=name, n=n, p=p, q=q, r=r, storage=cfg.get("storage", "f64"), scale=scale, reps=reps,
               fit_steps=fit_steps)
    with Context(0) as ctx, Context(0) as work:
        if f32:
            ctx.set_option("dtype", 1)
        ctx.generate_synthetic(n, p, q, truth, seed=SEED)
        ctx.set_option("xprod", 1)
        out["prepare_ms"] = ctx.xprod_prepare()[0]
        P, ldx = ct.c_int(), ct.c_int()
        ctx._chk(ctx._L.ppls_xprod_get(ctx.h, None, ct.byref(P), ct.byref(ldx)))
        perms = permutation_indices(n, reps + 1, rng)
        ident = np.arange(n, dtype=np.int64)
        g, gp, gi = [], [], []
        for b in range(reps + 1):          # the first round warms up (queue, clocks) and is dropped
            g.append(ctx.gram(2, 0, want=False)[1])
            gp.append(ctx.gram_permuted(perms[b], 0, want=False)[1])
            gi.append(ctx.gram_permuted(ident, 0, want=False)[1])
        g, gp, gi = g[1:], gp[1:], gi[1:]
        med, medp = statistics.median(g), statistics.median(gp)
        items = dict(block=((p + GQ - 1) // GQ) * ((q + GQ - 1) // GQ), joint=joint_live_quadrants(p, q, ldx.value, P.value))
        work_ratio = items["block"] / items["joint"]
        out.update(gram_ms=g, perm_ms=gp, identity_ms=gi, items=items, work_ratio=work_ratio, time_ratio=medp / med,
                   per_item_ratio=medp / med / work_ratio, identity_per_item_ratio=statistics.median(gi) / med / work_ratio,
                   gram_spread=(max(g) - min(g)) / med, perm_spread=(max(gp) - min(gp)) / medp,
                   occupancy=dict(unweighted=ctx.gram_occupancy(f32), weighted=ctx.gram_occupancy(f32, weighted=True),
                                  permuted=ctx.xperm_occupancy(f32)))
        if replicate:
            rep = []
            for b in range(reps + 1):      # the first replicate allocates S, the index array and the partials
                t0 = time.perf_counter()
                pm = permutation_indices(n, 1, rng)[0]
                t1 = time.perf_counter()
                work.xprod_permute(ctx, pm)
                t2 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    f = PPLS(None, None, r, fit_steps, 1e-4, "o2m_xprod", ctx=work)
                work.synchronize()
                t3 = time.perf_counter()
                tm = work.xperm_timing()
                rep.append(dict(draw_ms=1e3 * (t1 - t0), permute_ms=1e3 * (t2 - t1), check_ms=tm["check"],
                                upload_ms=tm["upload"], kernel_finish_ms=tm["kernel"], fit_ms=1e3 * (t3 - t2),
                                total_ms=1e3 * (t3 - t0), steps=[int(s) for s in f["Other_output"]["Number_steps"]]))
            out["first_replicate"] = rep[0]
            out["replicate"] = rep[1:]
            out["replicate_median_ms"] = {k: statistics.median(x[k] for x in rep[1:])
                                          for k in ("draw_ms", "permute_ms", "check_ms", "upload_ms", "kernel_finish_ms",
                                                    "fit_ms", "total_ms")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="?", default="c3,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-replicate", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    for name in args.configs.split(","):
        res = run(name, args.reps, args.scale, replicate=not args.no_replicate and name == "c3")
        path = os.path.join(args.outdir, f"permute_{name}.json")
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({k: res.get(k) for k in ("config", "n", "items", "work_ratio", "time_ratio", "per_item_ratio",
                                                   "identity_per_item_ratio", "gram_spread", "replicate_median_ms")}),
              flush=True)


if __name__ == "__main__":
    main()
