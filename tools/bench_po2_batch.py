"""Batched PO2PLS fits at a bench shape: 16 candidate sizes around the config's (r, rx, ry) on
one S, 50 forced EM steps,

  * ppls_po2_em_run_batch against the same 16 models one after another by ppls_po2_em_run, in the same process
    on the same S: wall clock around the calls (both return synchronised and include their uploads and
    read-backs), alternating rounds, medians;
  * the device time alone (ppls_po2_timing_batch, HIP events): one batched iteration against the 16 single
    iterations, and the batched pass (shared panels + one Gram launch) against the 16 single passes;
  * the parts of one model's iteration (ppls_po2_timing) for the centre candidate, to read the ratio against;
  * with --cv K: a whole crossval_PO2PLS call on the same grid from a K-fold stream of --cv-rows rows, and the
    share of it spent in the starts (the ppls_po2_start calls timed alone on the same selections).

S is formed once outside every timed window; --n takes fewer rows than the config's to shorten the run.
    python3 tools/bench_po2_batch.py [c3|c5] [--n ROWS] [--steps K] [--rounds R] [--cv K] [--cv-rows N] [--out FILE]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
from ppls_amd import Context, Po2Theta, crossval_PO2PLS  # noqa: E402

CENTRE = {"c3": (5, 3, 2), "c5": (10, 4, 2)}   # (r, rx, ry)


def _opt(argv, flag, default, cast):
    if flag in argv:
        i = argv.index(flag)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def candidates(r, rx, ry):
    """16 sizes around the centre: r - 2 .. r + 1 times rx - 1, rx + 1 times ry - 1, ry + 1 (r + rx <= 16 at C5)."""
    return [(a, b, c) for a in (r - 2, r - 1, r, r + 1) for b in (rx - 1, rx + 1) for c in (ry - 1, ry + 1)]


def start(rng, p, q, r, rx, ry):
    Gx, Gy = np.linalg.qr(rng.standard_normal((p, r + rx)))[0], np.linalg.qr(rng.standard_normal((q, r + ry)))[0]
    return Po2Theta(Gx[:, :r], Gx[:, r:], Gy[:, :r], Gy[:, r:], np.ones(r), np.ones(r), np.ones(rx), np.ones(ry), 1.0, 1.0, 1.0)


def main():
    argv = sys.argv[1:]
    out_path = _opt(argv, "--out", None, str)
    steps = _opt(argv, "--steps", 50, int)
    rounds = _opt(argv, "--rounds", 3, int)
    cv = _opt(argv, "--cv", 0, int)
    cv_rows = _opt(argv, "--cv-rows", 4000, int)
    name = argv[0] if argv and not argv[0].startswith("--") else "c3"
    cfg = bench.CONFIGS[name]
    n = _opt(argv, "--n", cfg["n"], int)
    p, q = cfg["p"], cfg["q"]
    r, rx, ry = CENTRE[name]
    cands = candidates(r, rx, ry)
    rec = dict(config=name, n=n, p=p, q=q, centre=[r, rx, ry], candidates=cands, steps=steps, rounds=rounds,
               sum_kx=sum(a + b for a, b, _ in cands), sum_ky=sum(a + c for a, _, c in cands))
    rec["panel_launches_per_pass"] = dict(batch=-(-rec["sum_kx"] // 16) - (-rec["sum_ky"] // 16), sequential=2 * len(cands))
    with Context(0) as ctx:
        if cfg.get("storage") == "f32":
            ctx.set_option("dtype", 1)
        truth, _ = bench.make_truth_and_theta0(p, q, r)
        ctx.generate_synthetic(n, p, q, truth, seed=20261021)
        ctx.set_option("xprod", 1)
        ctx.xprod_prepare()
        rng = np.random.default_rng(7)
        ths = [start(rng, p, q, *c) for c in cands]
        centre = start(rng, p, q, r, rx, ry)
        # warm every code path
        ctx.po2_em_run_batch(ths, 2, -np.inf)
        for t in ths:
            ctx.po2_em_run(t, 2, -np.inf, want_eout=False)
        wall_b, wall_s, dev = [], [], []
        for _ in range(rounds):   # alternating, same process, same S
            t0 = time.perf_counter()
            ctx.po2_em_run_batch(ths, steps, -np.inf)
            wall_b.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for t in ths:
                ctx.po2_em_run(t, steps, -np.inf, want_eout=False)
            wall_s.append((time.perf_counter() - t0) * 1e3)
            dev.append(ctx.po2_timing_batch(ths, steps, 1))
        med = lambda key: statistics.median(d[key] for d in dev)   # noqa: E731
        rec["wall_ms"] = dict(batch=statistics.median(wall_b), sequential=statistics.median(wall_s), batch_all=wall_b,
                              sequential_all=wall_s)
        rec["wall_ratio"] = rec["wall_ms"]["sequential"] / rec["wall_ms"]["batch"]
        rec["device_ms_per_iteration"] = {k: med(k) for k in ("batch", "sequential", "batch_pass", "sequential_pass")}
        rec["device_all"] = dev
        rec["device_ratio"] = med("sequential") / med("batch")
        rec["pass_ratio"] = med("sequential_pass") / med("batch_pass")
        rec["one_model_ms"] = ctx.po2_timing(centre, 50)
    if cv:
        rng = np.random.default_rng(11)
        X, Y = rng.standard_normal((cv_rows, p)), rng.standard_normal((cv_rows, q))
        labels = (np.arange(cv_rows) % cv).astype(np.int32)
        rs, rxs, rys = sorted({c[0] for c in cands}), sorted({c[1] for c in cands}), sorted({c[2] for c in cands})
        with Context(0) as c:
            c.stream_begin(p, q, False, False, nr_folds=cv)
            c.stream_rows(X, Y, labels)
            c.stream_end()
            crossval_PO2PLS(None, None, rs[:1], rxs[:1], rys[:1], cv, ctx=c, EMsteps=2, rng=np.random.default_rng(1))   # warm
            t0 = time.perf_counter()
            res = crossval_PO2PLS(None, None, rs, rxs, rys, cv, ctx=c, EMsteps=steps, atol=-np.inf, rng=np.random.default_rng(1))
            total = time.perf_counter() - t0
            V0x, V0y = rng.standard_normal((p, max(rxs))), rng.standard_normal((q, max(rys)))
            t0 = time.perf_counter()
            for f in range(cv):
                c.stream_select(f)
                for a, b, d in cands:
                    c.po2_start(a, b, d, V0x[:, :b], V0y[:, :d], 10)
            starts = time.perf_counter() - t0
            c.stream_select(-1)
        rec["crossval"] = dict(folds=cv, rows=cv_rows, cells=len(cands), steps=steps, total_s=total, starts_s=starts,
                               starts_share=starts / total, failed=int(res["failed"].sum()))
    rec["method"] = ("wall_ms: perf_counter around ppls_po2_em_run_batch and around the 16 ppls_po2_em_run calls (both "
                     "synchronous, uploads and read-backs included), alternating rounds in one process on one S, medians. "
                     "device_ms_per_iteration: HIP events around `steps` forced iterations (ppls_po2_timing_batch), one round per "
                     "alternation, medians. S is formed once outside every timed window. Produced by tools/bench_po2_batch.py.")
    rec["device"] = "MI355X (gfx950), one GPU"
    print(json.dumps(rec), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
