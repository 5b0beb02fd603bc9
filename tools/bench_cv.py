"""Time crossval_PPLS (crossval_PPLS.R:78-114) on the device against the same folds through the
fitting API alone (what a caller had before the device CV loop: slice on the host, upload, fit,
score in numpy).

    python tools/bench_cv.py [c4s,c3] [--repeats 3] [--no-parent] [--parent-max-gb 40] [--out FILE]

Per shape (c4s: the 8-GPU share of C4, n = 125k; c3: n = 1e6; p = q = 2000, fp64): 5 folds, a = 1..5
from one loop of 5-component fits (shared_folds=True), 'equal' starts, EMsteps = 100, atol = 1e-4, on
both statistics paths (xprod 0: streaming sweeps, xprod 1: cross-products by downdating).  Reported
per path: the wall time of every repeat, the split of the best repeat into gather / held-out Gram +
downdate / fits / scoring (ppls_cv_timing: HIP events for the two kernels, wall clock for the
host-driven phases), the gather's and the scoring kernel's GB/s, and -- unless --no-parent or the
host copy of X, Y would exceed --parent-max-gb -- the host loop's times and new / parent ratio.
Prints one JSON line (all shapes); --out also appends each shape's entry as soon as it is measured.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CONFIGS, make_truth_and_theta0  # noqa: E402
from ppls_amd import PPLS, Context, crossval_PPLS, cv_blocks  # noqa: E402

K, A, STEPS, ATOL = 5, [1, 2, 3, 4, 5], 100, 1e-4


def parent_loop(ctx, X, Y, perm):
    """The same folds with the fitting API only: per fold slice the training rows on the host, fit
    PPLS on a context (which uploads them), score Y - X W B C' in numpy for every prefix."""
    n = X.shape[0]
    blocks = cv_blocks(n, K)
    err = np.zeros((K, len(A)))
    for i in range(K):
        out = perm[blocks == i + 1]
        keep = np.ones(n, dtype=bool)
        keep[out] = False
        fit = PPLS(X[keep], Y[keep], max(A), STEPS, ATOL, "equal", ctx=ctx)
        T = X[out] @ fit["W"] * fit["B"]
        for j, e in enumerate(A):
            k = min(e, fit["W"].shape[1])
            err[i, j] = np.sqrt(np.mean((Y[out] - T[:, :k] @ fit["C"][:, :k].T) ** 2))
    return err.mean(axis=0)


def spread(ts):
    return dict(seconds=[round(t, 4) for t in ts], best=min(ts), spread=max(ts) - min(ts))


def measure(cfgname, repeats, parent, parent_max_gb):
    cfg = CONFIGS[cfgname]
    n, p, q = cfg["n"], cfg["p"], cfg["q"]
    truth, _ = make_truth_and_theta0(p, q, max(A))
    perm = np.random.default_rng(20261019).permutation(n)
    res = dict(workload=cfg["name"], n=n, p=p, q=q, folds=K, a=A, EMsteps=STEPS, atol=ATOL, repeats=repeats)
    host_gb = 8.0 * n * (p + q) / 1e9
    X = Y = None
    for xprod in (0, 1):
        ctx = Context(0)
        ctx.set_option("xprod", xprod)
        ctx.generate_synthetic(n, p, q, truth, seed=20261019)
        kw = dict(shared_folds=True, ctx=ctx, folds=perm, EMsteps=STEPS, atol=ATOL)
        crossval_PPLS(None, None, A, K, **kw)          # warm-up: allocations, the training context, S of all rows
        ts, splits = [], []
        for _ in range(repeats):
            ctx.cv_timing(reset=True)
            ctx.synchronize()
            t0 = time.perf_counter()
            cv = crossval_PPLS(None, None, A, K, **kw)
            ts.append(time.perf_counter() - t0)
            splits.append(ctx.cv_timing(reset=True))
        best = splits[int(np.argmin(ts))]
        entry = dict(new=spread(ts), errors=[float(e) for e in cv["errors"]], which_error=cv["which_error"],
                     split_ms={k: best[k] for k in ("gather_ms", "downdate_ms", "fit_ms", "score_ms")},
                     gather_GBps=best["gather_bytes"] / best["gather_ms"] / 1e6 if best["gather_ms"] > 0 else None,
                     score_GBps=best["score_bytes"] / best["score_ms"] / 1e6 if best["score_ms"] > 0 else None,
                     note="split of the best repeat; S of all rows is formed in the warm-up and reused "
                          "(xprod 1), as it is across crossval_PPLS calls on resident data")
        if parent and host_gb <= parent_max_gb:
            if X is None:
                X, Y = ctx.get_data_rows()
            pctx = Context(0)
            pctx.set_option("xprod", xprod)
            pe = parent_loop(pctx, X, Y, perm)         # warm-up
            tp = []
            for _ in range(repeats):
                pctx.synchronize()
                t0 = time.perf_counter()
                pe = parent_loop(pctx, X, Y, perm)
                tp.append(time.perf_counter() - t0)
            pctx.close()
            entry["parent"] = spread(tp)
            entry["parent_errors"] = [float(e) for e in pe]
            entry["new_over_parent"] = min(ts) / min(tp)
            entry["errors_rel_diff"] = float(np.max(np.abs(pe - cv["errors"]) / pe))
        elif parent:
            entry["parent"] = None
            entry["parent_skipped"] = f"host copy of X, Y is {host_gb:.0f} GB (> --parent-max-gb {parent_max_gb:g})"
        res[f"xprod{xprod}"] = entry
        ctx.close()
    return res


def main():
    argv = sys.argv[1:]
    names = argv[0].split(",") if argv and not argv[0].startswith("-") else ["c4s", "c3"]
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    pmax = float(argv[argv.index("--parent-max-gb") + 1]) if "--parent-max-gb" in argv else 40.0
    outfile = argv[argv.index("--out") + 1] if "--out" in argv else None
    out = dict(tool="tools/bench_cv.py", shapes={})
    for name in names:
        out["shapes"][name] = measure(name, repeats, "--no-parent" not in argv, pmax)
        if outfile:
            with open(outfile, "a") as f:
                f.write(json.dumps({name: out["shapes"][name]}) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
