"""PO2PLS from the cross-products at a bench shape: the statistics pass (both panels of M = S G)
against the PPLS_simult tile kernel at r = max(kx, ky) on the same S in the same process (HIP events,
reps launches back to back, three rounds alternating the two, medians), the Gram, the small kernel, the
loading update (polar type, and QR type: the same without the Jacobi polar factor) and one whole ECM
iteration, and that iteration against the cross-product iteration of PPLS_simult at the same joint r
(wall clock around ppls_em_iterate, synchronised).

The pass and both iterations read S only, so the row count enters through the formation of S, which
is outside every timed window: --n takes fewer rows than the config's to shorten the run.
    python3 tools/bench_po2.py [c3|c5] [--n ROWS] [--reps K] [--out FILE]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
from ppls_amd import Context, Po2Theta  # noqa: E402

SHAPES = {"c3": (5, 3, 2), "c5": (10, 4, 2)}   # (r, rx, ry)


def _opt(argv, flag, default, cast):
    if flag in argv:
        i = argv.index(flag)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def main():
    argv = sys.argv[1:]
    out_path = _opt(argv, "--out", None, str)
    reps = _opt(argv, "--reps", 200, int)
    name = argv[0] if argv and not argv[0].startswith("--") else "c3"
    cfg = bench.CONFIGS[name]
    n = _opt(argv, "--n", cfg["n"], int)
    p, q = cfg["p"], cfg["q"]
    r, rx, ry = SHAPES[name]
    kx, ky, wmax = r + rx, r + ry, max(r + rx, r + ry)
    rec = dict(config=name, n=n, p=p, q=q, r=r, rx=rx, ry=ry, reps=reps, rounds=3)
    with Context(0) as ctx:
        if cfg.get("storage") == "f32":
            ctx.set_option("dtype", 1)
        truth, _ = bench.make_truth_and_theta0(p, q, r)
        ctx.generate_synthetic(n, p, q, truth, seed=20261021)
        ctx.set_option("xprod", 1)
        ctx.xprod_prepare()
        info = ctx.xprod_info(wmax)
        rec.update(bytes_per_pass=info["bytes_per_pass"], rows_per_wave=info["rows_per_wave"])
        rng = np.random.default_rng(7)
        Gx, Gy = np.linalg.qr(rng.standard_normal((p, kx)))[0], np.linalg.qr(rng.standard_normal((q, ky)))[0]
        th = Po2Theta(Gx[:, :r], Gx[:, r:], Gy[:, :r], Gy[:, r:], np.ones(r), np.ones(r), np.ones(rx), np.ones(ry), 1.0, 1.0, 1.0)
        _, th_wide = bench.make_truth_and_theta0(p, q, wmax)
        _, th_joint = bench.make_truth_and_theta0(p, q, r)
        # warm both code paths
        ctx.po2_timing(th, 3)
        ctx.em_begin(th_wide)
        ctx.em_iterate(2)
        ctx.xprod_tile_timing(3)
        po2, tile = [], []
        for _ in range(3):   # alternating, same process, same S
            po2.append(ctx.po2_timing(th, reps))
            ctx.em_begin(th_wide)
            ctx.em_iterate(1)
            tile.append(ctx.xprod_tile_timing(reps))
        med = lambda key: statistics.median(t[key] for t in po2)   # noqa: E731
        tile_ms = statistics.median(tile)
        rec["po2_ms"] = {k: med(k) for k in ("pass", "gram", "small", "update", "iteration", "update_qr")}
        rec["po2_all"] = po2
        rec["tile_ms"] = dict(r=wmax, ms=tile_ms, all_ms=tile)
        rec["pass_over_tile"] = med("pass") / tile_ms
        rec["pass_gbytes_per_s"] = info["bytes_per_pass"] / med("pass") / 1e6
        # the whole xprod iteration of PPLS_simult at the joint r
        steps = 100
        its = []
        for _ in range(3):
            ctx.em_begin(th_joint)
            ctx.em_iterate(3)
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.em_iterate(steps)
            ctx.synchronize()
            its.append((time.perf_counter() - t0) * 1e3 / steps)
        rec["simult_iteration_ms"] = dict(r=r, ms=statistics.median(its), all_ms=its, steps=steps)
        rec["iteration_over_simult"] = med("iteration") / statistics.median(its)
    print(json.dumps(rec), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
