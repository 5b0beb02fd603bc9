"""The row diagnostics kernel at a bench config on resident synthetic data, beside the two existing
row passes it is measured against:

* the kernel over all local rows without and with the posterior means (ppls_rowdiag_timing: HIP events
  around the launches only, averaged over --reps launches after one untimed launch);
* ppls_heldout_sse over all rows with the config's k (its scoring kernel and reduce between HIP events,
  ppls_cv_timing's score_ms): phase 1 on X and phase 2 on Y, where the diagnostics kernel does both on both;
* ppls_scores (wall clock of the call, which includes the copy of T and U to the host).

    python3 tools/rowdiag_timing.py [c3|c5] [--reps N] [--out FILE]     (default profiles/diagnostics_<config>.json)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from ppls_amd import Context  # noqa: E402


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
    out_path = opt.get("--out", os.path.join(ROOT, "profiles", f"diagnostics_{name}.json"))
    cfg = bench.CONFIGS[name]
    n, p, q, r = cfg["n"], cfg["p"], cfg["q"], cfg["r"]
    f32 = cfg.get("storage") == "f32"
    row_bytes = float(n) * (4 if f32 else 8) * (p + q)
    rec = dict(config=name, n=n, p=p, q=q, k=r, storage="f32" if f32 else "f64", reps=reps, row_bytes=row_bytes)
    with Context(0) as ctx:
        if f32:
            ctx.set_option("dtype", 1)
        truth, _ = bench.make_truth_and_theta0(p, q, r)
        ctx.generate_synthetic(n, p, q, truth, seed=20261020)
        rows = np.arange(n, dtype=np.int64)
        B = np.diag(truth.B) if np.ndim(truth.B) == 2 else np.asarray(truth.B)
        held, rounds = [], []
        ctx.heldout_sse(truth.W, truth.C, B, rows)            # untimed: loads the code
        for _ in range(3):                                     # alternate the two kernels: the machine is shared
            ctx.cv_timing(reset=True)
            for _ in range(5):
                ctx.heldout_sse(truth.W, truth.C, B, rows)
            held.append(ctx.cv_timing(reset=True)["score_ms"] / 5)
            rounds.append(ctx.rowdiag_timing(r, reps))
        ctx.scores(truth.W, truth.C)
        wall = []
        for _ in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.scores(truth.W, truth.C)
            wall.append((time.perf_counter() - t0) * 1e3)
    rec["heldout_sse_ms"] = held
    rec["rowdiag_ms"] = [x["ms"] for x in rounds]
    rec["rowdiag_mu_ms"] = [x["ms_mu"] for x in rounds]
    rec["scores_call_wall_ms"] = wall
    med = statistics.median
    rec["median"] = dict(heldout_sse_ms=med(held), rowdiag_ms=med(rec["rowdiag_ms"]), rowdiag_mu_ms=med(rec["rowdiag_mu_ms"]),
                         scores_call_wall_ms=med(wall))
    rec["ratio_to_heldout_sse"] = rec["median"]["rowdiag_ms"] / rec["median"]["heldout_sse_ms"]
    rec["ratio_mu_to_heldout_sse"] = rec["median"]["rowdiag_mu_ms"] / rec["median"]["heldout_sse_ms"]
    rec["rowdiag_tb_per_s_of_one_read"] = row_bytes / (rec["median"]["rowdiag_ms"] * 1e-3) / 1e12
    rec["heldout_sse_tb_per_s"] = row_bytes / (rec["median"]["heldout_sse_ms"] * 1e-3) / 1e12
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
