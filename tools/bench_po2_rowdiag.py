"""The PO2PLS row diagnostics kernel at a bench config on resident synthetic data, beside the kernel it is
measured against, by the method of tools/rowdiag_timing.py:

* ppls_po2_rowdiag_kernel over all local rows at the config's (r, rx, ry), without and with the posterior means
  (ppls_po2_rowdiag_timing: HIP events around --reps launches after one untimed launch);
* ppls_rowdiag_kernel at r = max(kx, ky) on the same rows (ppls_rowdiag_timing), the same way: both read every
  row of X and of Y twice, so the target is the project's bar for a same-read kernel, 1.10 x;
* three rounds, the two kernels alternated in one process; medians;
* one outer iteration of robust_PO2PLS (wall clock, synchronised): po2_robust_weights, xprod_weighted from the
  kept weights, five forced ECM steps of po2_em_run on S_u.

    python3 tools/bench_po2_rowdiag.py [c3|c5] [--reps N] [--out FILE]   (default profiles/po2_rowdiag_<config>.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from ppls_amd import Context, Po2Theta  # noqa: E402

SIZES = {"c3": (5, 3, 2), "c5": (10, 4, 2)}
TARGET = 1.10


def po2_theta(p, q, r, rx, ry, seed=7):
    rng = np.random.default_rng(seed)
    Gx = np.linalg.qr(rng.standard_normal((p, r + rx)))[0]
    Gy = np.linalg.qr(rng.standard_normal((q, r + ry)))[0]
    return Po2Theta(Gx[:, :r], Gx[:, r:], Gy[:, :r], Gy[:, r:], 1.2 - 0.05 * np.arange(r), 1.5 - 0.05 * np.arange(r),
                    1.1 - 0.1 * np.arange(rx), 0.9 - 0.1 * np.arange(ry), 0.7, 0.8, 0.5)


def main():
    argv = sys.argv[1:]
    opt = {}
    for key in ("--out", "--reps"):
        if key in argv:
            i = argv.index(key)
            opt[key] = argv[i + 1]
            del argv[i:i + 2]
    name = argv[0] if argv else "c3"
    reps = int(opt.get("--reps", 20))
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", f"po2_rowdiag_{name}.json"))
    cfg = bench.CONFIGS[name]
    n, p, q = cfg["n"], cfg["p"], cfg["q"]
    r, rx, ry = SIZES[name]
    kx, ky = r + rx, r + ry
    f32 = cfg.get("storage") == "f32"
    row_bytes = float(n) * (4 if f32 else 8) * (p + q)
    rec = dict(config=name, n=n, p=p, q=q, r=r, rx=rx, ry=ry, comparator_r=max(kx, ky), storage="f32" if f32 else "f64",
               reps=reps, row_bytes=row_bytes, target=TARGET)
    th = po2_theta(p, q, r, rx, ry)
    with Context(0) as ctx:
        if f32:
            ctx.set_option("dtype", 1)
        truth, _ = bench.make_truth_and_theta0(p, q, cfg["r"])
        ctx.generate_synthetic(n, p, q, truth, seed=20261021)
        rec["instantiation"] = ctx.po2_rowdiag_info(r, rx, ry, f32)
        ctx.po2_rowdiag_timing(th, 1)                          # untimed: loads the code
        ctx.rowdiag_timing(max(kx, ky), 1)
        new, old = [], []
        for _ in range(3):                                     # alternate the two kernels: the machine is shared
            old.append(ctx.rowdiag_timing(max(kx, ky), reps))
            new.append(ctx.po2_rowdiag_timing(th, reps))
        with Context(0) as work:                               # an error here ends the run: no profile is written
            for it in range(2):                                # the first iteration allocates and loads code
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.po2_robust_weights(th, 4.0)
                ctx.synchronize()
                t1 = time.perf_counter()
                work.xprod_weighted(ctx)
                work.synchronize()
                t2 = time.perf_counter()
                work.po2_em_run(th, 5, -np.inf, want_eout=False)
                work.synchronize()
                t3 = time.perf_counter()
                wall = dict(weights_ms=(t1 - t0) * 1e3, xprod_weighted_ms=(t2 - t1) * 1e3, em_run_5_ms=(t3 - t2) * 1e3,
                            total_ms=(t3 - t0) * 1e3)
            rec["robust_outer_iteration_wall"] = wall
    rec["po2_rowdiag_ms"] = [float(x["ms"]) for x in new]
    rec["po2_rowdiag_mu_ms"] = [float(x["ms_mu"]) for x in new]
    rec["rowdiag_ms"] = [float(x["ms"]) for x in old]
    rec["rowdiag_mu_ms"] = [float(x["ms_mu"]) for x in old]
    med = statistics.median
    rec["median"] = {key: med(rec[key]) for key in ("po2_rowdiag_ms", "po2_rowdiag_mu_ms", "rowdiag_ms", "rowdiag_mu_ms")}
    rec["ratio"] = rec["median"]["po2_rowdiag_ms"] / rec["median"]["rowdiag_ms"]
    rec["ratio_mu"] = rec["median"]["po2_rowdiag_mu_ms"] / rec["median"]["rowdiag_mu_ms"]
    rec["meets_target"] = bool(rec["ratio"] <= TARGET)
    rec["meets_target_mu"] = bool(rec["ratio_mu"] <= TARGET)
    rec["po2_rowdiag_tb_per_s_of_one_read"] = row_bytes / (rec["median"]["po2_rowdiag_ms"] * 1e-3) / 1e12
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
