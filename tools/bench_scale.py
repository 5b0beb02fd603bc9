"""Time ppls_scale_data (R's scale() on the resident data) pass by pass.

    python tools/bench_scale.py [c3,c5] [--repeats 3] [--out profiles/scale_bench.json]

Per config (bench.py's: c3 n = 1e6, p = q = 2000, fp64; c5 n = 5e5, p = 10000, q = 500, fp32 storage)
the data are generated on the device, then ``scale_data(True, True)`` and ``scale_data(True, False)``
run ``repeats`` times each after one warm-up call (every call rescales the already scaled data: the
same bytes move).  Reported per call kind, from the repeat with the smallest total: ms per pass
(HIP events around the pass's kernels, X and Y together), bytes per pass (the statistics passes read
the real columns' 16-byte units; the apply pass reads and writes the real columns) and TB/s, and the
statistics passes' rate relative to the C3 split sweep's read rate of the README's results table.
Writes one JSON line per config to --out (replacing the file) and prints them.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CONFIGS, make_truth_and_theta0  # noqa: E402
from ppls_amd import Context  # noqa: E402

SWEEP_READ_TBPS = 6.74      # the C3 split sweep (README results table): the yardstick for pure reads
PASSES = ("sums", "centred_squares", "apply")


def measure(name, repeats):
    cfg = CONFIGS[name]
    n, p, q = cfg["n"], cfg["p"], cfg["q"]
    f32 = cfg.get("storage") == "f32"
    truth, _ = make_truth_and_theta0(p, q, cfg["r"])
    res = dict(tool="tools/bench_scale.py", config=name, workload=cfg["name"], n=n, p=p, q=q,
               storage="f32" if f32 else "f64", repeats=repeats, sweep_read_TBps=SWEEP_READ_TBPS)
    with Context(0) as ctx:
        ctx.set_option("dtype", 1 if f32 else 0)
        ctx.generate_synthetic(n, p, q, truth, seed=20261019)
        ctx.scale_data(True, True)                    # warm-up
        for key, (center, scale) in (("center_scale", (True, True)), ("center", (True, False))):
            runs = []
            for _ in range(repeats):
                ctx.scale_data(center, scale)
                runs.append(ctx.scale_timing())
            best = min(runs, key=lambda t: float(t["ms"].sum()))
            entry = dict(total_ms_all=[round(float(t["ms"].sum()), 4) for t in runs])
            for i, pname in enumerate(PASSES):
                ms, by = float(best["ms"][i]), float(best["bytes"][i])
                if by == 0.0:
                    continue
                tbps = by / ms / 1e9 if ms > 0 else None
                entry[pname] = dict(ms=round(ms, 4), bytes=by, TBps=None if tbps is None else round(tbps, 3))
                if i < 2 and tbps is not None:
                    entry[pname]["vs_sweep_read"] = round(tbps / SWEEP_READ_TBPS, 3)
            res[key] = entry
        ssq = ctx.ssq()
        res["ssq_after"] = [ssq[0], ssq[1]]           # (n - 1) p and (n - 1) q for standardised columns
    return res


def main():
    argv = sys.argv[1:]
    names = argv[0].split(",") if argv and not argv[0].startswith("-") else ["c3", "c5"]
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    outfile = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "scale_bench.json")
    lines = []
    for name in names:
        lines.append(json.dumps(measure(name, repeats)))
        print(lines[-1], flush=True)
        with open(outfile, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
