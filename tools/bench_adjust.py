"""Time the covariate adjustment (ppls_adjust_data, ppls_xprod_adjust) pass by pass against the scale passes.

    python tools/bench_adjust.py [c3,c5] [--k1 3,9,16] [--repeats 3] [--outdir profiles]
    python tools/bench_adjust.py c5 --k1 9 --coef-only      # one coefficient pass, for a counters-only profile

Per config (bench.py's: c3 n = 1e6, p = q = 2000, fp64; c5 n = 5e5, p = 10000, q = 500, fp32 storage) the
data are generated on the device.  In the same process and on the same context:

  scale_data(center=True, scale=False)   its statistics pass (column sums: one read of the rows) and its
                                         apply pass (one read, one write) are the yardsticks;
  adjust_data(Z, intercept=True)         for each k1: Z = k1 - 1 standard normal columns; the coefficient
                                         pass (one read, k1 fp64 FMAs per element) and the apply pass
                                         (one read, one write, k1 FMAs per element).  The data are
                                         generated again before each call: adjusted data refuse another.
  xprod_adjust(src, k, scale=True)       the Schur pass on the context's S (its last k Y columns as the
                                         covariates) against the stream's standardise pass that follows
                                         it on the result -- the same 64 x 64 tile pass with one vector
                                         instead of k.

Every time is the ms between two HIP events around the pass's kernels (X and Y together); the best of
``repeats`` calls is reported, all of them kept.  The expectation on record: each row pass <= 1.25 x its scale
pass at k1 <= 9 (at C3 with k1 = 9 the arithmetic is 3.6e10 FMAs, about 0.9 ms at the fp64 vector peak,
beside a 4.7 ms read); k1 = 16 as measured.  Writes profiles/adjust_<config>.json.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CONFIGS, make_truth_and_theta0  # noqa: E402
from ppls_amd import Context  # noqa: E402

SEED = 20261021


def measure(name, k1s, repeats):
    cfg = CONFIGS[name]
    n, p, q = cfg["n"], cfg["p"], cfg["q"]
    f32 = cfg.get("storage") == "f32"
    truth, _ = make_truth_and_theta0(p, q, cfg["r"])
    es = 4 if f32 else 8
    res = dict(tool="tools/bench_adjust.py", config=name, workload=cfg["name"], n=n, p=p, q=q,
               storage="f32" if f32 else "f64", repeats=repeats, row_bytes=n * es * (p + q))
    rng = np.random.default_rng(SEED)
    Zall = rng.standard_normal((n, max(k1s) - 1))
    with Context(0) as ctx, Context(0) as dst:
        ctx.set_option("dtype", 1 if f32 else 0)
        ctx.generate_synthetic(n, p, q, truth, seed=SEED)
        ctx.scale_data(True, False)                   # warm-up
        runs = []
        for _ in range(repeats):
            ctx.scale_data(True, False)
            runs.append(ctx.scale_timing()["ms"].copy())
        stat = min(float(t[0]) for t in runs)
        appl = min(float(t[2]) for t in runs)
        res["scale"] = dict(stats_ms=round(stat, 4), apply_ms=round(appl, 4),
                            stats_ms_all=[round(float(t[0]), 4) for t in runs],
                            apply_ms_all=[round(float(t[2]), 4) for t in runs])
        res["adjust"] = {}
        for k1 in k1s:
            Z = np.ascontiguousarray(Zall[:, : k1 - 1])
            info = None
            coef, app = [], []
            for _ in range(repeats + 1):              # the first call is the warm-up
                ctx.generate_synthetic(n, p, q, truth, seed=SEED)
                info = ctx.adjust_info(k1)
                ctx.adjust_data(Z, True)
                t = ctx.adjust_timing()
                coef.append(float(t["coef"]))
                app.append(float(t["apply"]))
            coef, app = coef[1:], app[1:]
            res["adjust"][f"k1={k1}"] = dict(
                kt=info["kt"], plan_x=info["X"], coef_ms=round(min(coef), 4), apply_ms=round(min(app), 4),
                coef_ms_all=[round(v, 4) for v in coef], apply_ms_all=[round(v, 4) for v in app],
                coef_vs_scale_stats=round(min(coef) / stat, 3), apply_vs_scale_apply=round(min(app) / appl, 3),
                fma=float(n) * (p + q) * k1)
        # the Schur pass on S of the same size: the last k Y columns of fresh data as the covariates
        ctx.generate_synthetic(n, p, q, truth, seed=SEED)
        ctx.scale_data(True, False)
        res["schur"] = {}
        for k1 in k1s:
            k = min(k1, q - 1)
            sch, std = [], []
            for _ in range(repeats + 1):
                dst.xprod_adjust(ctx, k, True)
                t = dst.adjust_timing()
                sch.append(float(t["schur"]))
                std.append(float(t["standardise"]))
            sch, std = sch[1:], std[1:]
            res["schur"][f"k={k}"] = dict(schur_ms=round(min(sch), 4), standardise_ms=round(min(std), 4),
                                          schur_ms_all=[round(v, 4) for v in sch],
                                          standardise_ms_all=[round(v, 4) for v in std],
                                          schur_vs_standardise=round(min(sch) / min(std), 3))
    return res


def coef_once(name, k1):
    """One coefficient pass at k1 on the config's data, for a counters-only profiler run around it
    (rocprofv3 --pmc FETCH_SIZE with no tracing; the kernel's row of the CSV is the pass's fetch)."""
    cfg = CONFIGS[name]
    n, p, q = cfg["n"], cfg["p"], cfg["q"]
    truth, _ = make_truth_and_theta0(p, q, cfg["r"])
    Q = np.random.default_rng(SEED).standard_normal((n, k1)) / np.sqrt(n)
    with Context(0) as ctx:
        ctx.set_option("dtype", 1 if cfg.get("storage") == "f32" else 0)
        ctx.generate_synthetic(n, p, q, truth, seed=SEED)
        ctx.adjust_coef(Q)
        print(json.dumps(dict(config=name, k1=k1, coef_ms=float(ctx.adjust_timing()["coef"]))))


def main():
    argv = sys.argv[1:]
    if "--coef-only" in argv:
        return coef_once(argv[0], int(argv[argv.index("--k1") + 1]))
    names = argv[0].split(",") if argv and not argv[0].startswith("-") else ["c3", "c5"]
    k1s = [int(v) for v in argv[argv.index("--k1") + 1].split(",")] if "--k1" in argv else [3, 9, 16]
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    outdir = argv[argv.index("--outdir") + 1] if "--outdir" in argv else os.path.join(ROOT, "profiles")
    for name in names:
        line = json.dumps(measure(name, k1s, repeats))
        print(line, flush=True)
        with open(os.path.join(outdir, f"adjust_{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
