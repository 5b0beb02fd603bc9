"""PPLS(X, Y, a, 20, 1e-4, initialGuess) at a bench config on resident synthetic data: wall seconds of
the whole sequential fit with 'o2m_xprod' starting values (the cross-products S, one device pass over
its off-diagonal block per Lanczos step, every component fitted once) and with 'o2m' (joint Gram + host
singular pairs + the device refits of earlier components) beside 'equal' and 'random'.  Three settings,
because only 'o2m_xprod' needs S when the fits sweep the rows (option xprod = 0, the context's default):

* cold -- xprod = 0 and no S on the context: the call forms S itself (what a plain first call costs);
* kept -- xprod = 0 with the S an earlier call left: the start's own cost beside a row-sweeping fit;
* xprod = 1 -- every kind's fits read S, so S is shared work and outside every timed call.

Then the 'o2m_xprod' pass alone against one r = 1 pass of the tile kernel over the same S (HIP events,
back to back, after a warm-up), and the Lanczos passes and milliseconds of one start.
    python3 tools/bench_o2m.py [c3|c5] [--out FILE] [--skip-o2m]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
from ppls_amd import PPLS, Context, Theta, initial_guess  # noqa: E402


def main():
    argv = sys.argv[1:]
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    names = [a for a in argv if not a.startswith("--")]
    name = names[0] if names else "c3"
    cfg = bench.CONFIGS[name]
    n, p, q, r = cfg["n"], cfg["p"], cfg["q"], cfg["r"]
    rec = dict(config=name, n=n, p=p, q=q, a=r, fits=[])
    with Context(0) as ctx:
        if cfg.get("storage") == "f32":
            ctx.set_option("dtype", 1)
        truth, _ = bench.make_truth_and_theta0(p, q, r)
        ctx.generate_synthetic(n, p, q, truth, seed=20261015)
        fit = None

        def timed(kind, setting):
            nonlocal fit
            ready = ctx.xprod_info()["ready"]
            ctx.synchronize()
            t0 = time.perf_counter()
            f = PPLS(None, None, r, 20, 1e-4, kind, rng=np.random.default_rng(1), ctx=ctx)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            row = dict(initialGuess=kind, setting=setting, s_ready_before=ready, seconds=dt,
                       steps=[int(v) for v in f["Other_output"]["Number_steps"]],
                       loglik_last=float(f["Other_output"]["Loglikelihoods"][-1]))
            if kind == "o2m_xprod":
                row.update(o2m_info=ctx.o2m_info())
                fit = f
            rec["fits"].append(row)
            print(json.dumps(dict(config=name, **row)), flush=True)
            return dt

        def med(kind, setting):
            return statistics.median(x["seconds"] for x in rec["fits"] if x["initialGuess"] == kind and x["setting"] == setting)

        # xprod = 0: the fits sweep the rows.  'equal' first (loads the sweep's code), then per round a
        # 'random' fit, a cold 'o2m_xprod' (no S: the call forms it; the first round also loads the
        # Gram's code) and a kept one (S left by the cold call), S released again at the round's end
        timed("equal", "xprod0")
        for _ in range(3):
            timed("random", "xprod0")
            assert not ctx.xprod_info()["ready"]
            timed("o2m_xprod", "cold")
            rec.setdefault("cold_setup_ms", []).append(ctx.xprod_setup_times()[2])
            timed("o2m_xprod", "kept")
            ctx.xprod_release()
        if "--skip-o2m" not in sys.argv:
            timed("o2m", "xprod0")
        # xprod = 1: every kind reads S, formed once outside the timed calls
        ctx.set_option("xprod", 1)
        ctx.xprod_prepare()
        timed("equal", "xprod1")
        for _ in range(3):
            timed("random", "xprod1")
            timed("o2m_xprod", "xprod1")
        ctx.set_option("xprod", 0)   # (S came from xprod_prepare: it stays)
        rnd0, rnd1 = med("random", "xprod0"), med("random", "xprod1")
        rec["seconds"] = dict(
            xprod0=dict(random=rnd0, equal=med("equal", "xprod0"), o2m_xprod_cold=med("o2m_xprod", "cold"),
                        o2m_xprod_cold_all=[x["seconds"] for x in rec["fits"] if x["setting"] == "cold"],
                        o2m_xprod_kept=med("o2m_xprod", "kept"),
                        **({} if "--skip-o2m" in sys.argv else dict(o2m=med("o2m", "xprod0")))),
            xprod1=dict(random=rnd1, equal=med("equal", "xprod1"), o2m_xprod=med("o2m_xprod", "xprod1")))
        rec["o2m_xprod_over_random"] = dict(cold=med("o2m_xprod", "cold") / rnd0, kept=med("o2m_xprod", "kept") / rnd0,
                                            xprod1=med("o2m_xprod", "xprod1") / rnd1)
        # the pass alone, and the r = 1 tile pass of the same S
        reps = 50
        pt = [ctx.o2m_pass_timing(reps) for _ in range(3)]
        ms = statistics.median(t["ms"] for t in pt)
        rec["pass"] = dict(ms=ms, all_ms=[t["ms"] for t in pt], path=pt[0]["path"], bytes=pt[0]["bytes"],
                           gbytes_per_s=pt[0]["bytes"] / ms / 1e6, reps=reps)
        ctx.set_option("xprod", 1)
        g = initial_guess(p, q, "equal")
        ctx.em_begin(Theta(g["W"].reshape(p, 1), g["C"].reshape(q, 1), g["B"], g["sigE"], g["sigF"], g["sigH"], g["sigT"]))
        tt = [ctx.xprod_tile_timing(reps) for _ in range(3)]
        tile_ms = statistics.median(tt)
        info = ctx.xprod_info(1)
        rec["tile_r1"] = dict(ms=tile_ms, all_ms=tt, bytes=info["bytes_per_pass"],
                              gbytes_per_s=info["bytes_per_pass"] / tile_ms / 1e6, reps=reps)
        rec["pass_over_tile"] = ms / tile_ms
        ctx.set_option("xprod", 0)
        # one start: undeflated, and deflated by the fitted components but the last
        starts = {}
        for label, k in (("k0", 0), (f"k{r - 1}", r - 1)):
            Wp, Cp = (fit["W"][:, :k], fit["C"][:, :k]) if k else (None, None)
            ts = []
            for _ in range(5):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.o2m_start(Wp, Cp)
                ts.append((time.perf_counter() - t0) * 1e3)
            starts[label] = dict(ms=statistics.median(ts), all_ms=ts, passes=ctx.o2m_info()["passes"])
        rec["start"] = starts
    print(json.dumps(rec), flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
