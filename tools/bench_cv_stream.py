"""Time cross-validation on streamed data (ppls_stream_begin_folds .. ppls_cv_ppls_stream).

    python tools/bench_cv_stream.py [--out profiles/cv_stream_bench.json] [--scale 1.0] [--repeats 3]

Shape C3 (p = q = 2000, n = 1e6) fed as ten device chunks from source contexts (as
tools/bench_stream.py builds them), K = 5 folds from a seeded permutation, center = scale = 1.  One
JSON line:

formation  begin .. end with folds against the plain stream's begin .. end, in the same process on
           the same chunks, interleaved; one warm-up repeat and --repeats (default 3) timed ones,
           every call's wall time kept.  The plain stream is the yardstick.  Beside it the cost model of what the
           folds add, at the rates DESIGN §15 measured: one gather of every chunk (read + write),
           K merges per chunk instead of one (each a read + write of S_k plus its Gram partials), and
           at the end one recentre-and-standardise pass over K matrices (read + write) and one
           selection (K reads, one write) in place of the plain stream's standardise pass.  The K
           short Grams of a chunk run the flops of the one long Gram, so the model predicts
           plain + extra; the file records the prediction, the measurement and their difference,
           and the plain stream's run-to-run spread to judge it by.
cv         crossval_PPLS(a = 1..5, shared_folds=True, EMsteps=100, atol=1e-4, 'equal') on the streamed
           context, --repeats timed runs after a warm-up, and one pass with the phases timed apart
           (select, fit, held-out error per fold).  profiles/cv_bench.json's C3 ``xprod 1`` row
           (resident rows, the same K, a and stop rule) is quoted beside it; the two come from
           different runs.

--scale s multiplies n by s (a quick run on a smaller problem; the JSON records it).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_truth_and_theta0  # noqa: E402
from ppls_amd import Context, crossval_PPLS, fold_labels, initial_guess  # noqa: E402

P = Q = 2000
K = 5
NCH = 10
SEED = 20261019
READ_TBPS = 6.75        # the column-sum passes at C3
RW_TBPS = 5.2           # the in-place apply pass (bytes read + written)


def cost_model(n, nsplit=8):
    """Milliseconds the folds add to the plain stream's formation, pass by pass."""
    data = n * 8.0 * (P + Q)
    s_bytes = 8.0 * (P + Q) ** 2
    quads = ((P + Q + 127) // 128) * (((P + Q + 127) // 128) + 1) // 2 * 4
    part = nsplit * quads * 64 * 64 * 8.0           # (a segment's Gram is taken to split as a chunk's does)
    ms = lambda b, rate: b / rate / 1e9             # noqa: E731
    extra = dict(gather=ms(2 * data, RW_TBPS),
                 merges=ms(NCH * (K - 1) * (2 * s_bytes + part), RW_TBPS),
                 end_finish=ms(K * 2 * s_bytes, RW_TBPS),
                 end_select=ms((K + 1) * s_bytes, RW_TBPS),
                 minus_plain_standardise=-ms(2 * s_bytes, RW_TBPS))
    return dict(extra_ms={k: round(v, 3) for k, v in extra.items()}, extra_total_ms=round(sum(extra.values()), 3),
                note="the K Grams of n_c / K rows run the flops of the chunk's one Gram; launches and the "
                     "upload of every segment's Gram queue are not in the model")


def timed_stream(c, srcs, labels, bounds):
    c.synchronize()
    t0 = time.perf_counter()
    c.stream_begin(P, Q, True, True, nr_folds=None if labels is None else K)
    stamps = [time.perf_counter()]
    for k, s in enumerate(srcs):
        c.stream_rows_from(s, None if labels is None else labels[bounds[k]:bounds[k + 1]])
        stamps.append(time.perf_counter())
    c.stream_end()
    t2 = time.perf_counter()
    calls = [round((b - a) * 1e3, 2) for a, b in zip([t0] + stamps, stamps + [t2])]
    return round((t2 - t0) * 1e3, 3), calls


def main():
    argv = sys.argv[1:]
    outfile = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "cv_stream_bench.json")
    scale = float(argv[argv.index("--scale") + 1]) if "--scale" in argv else 1.0
    reps = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    n = int(1_000_000 * scale)
    truth, _ = make_truth_and_theta0(P, Q, 5)
    bounds = [n * k // NCH for k in range(NCH + 1)]
    labels = fold_labels(n, K, rng=np.random.default_rng(SEED))
    res = dict(tool="tools/bench_cv_stream.py", p=P, q=Q, n=n, chunks=NCH, nr_folds=K, repeats=reps, scale=scale)
    srcs = []
    for k in range(NCH):
        s = Context(0)
        s.generate_synthetic(n, P, Q, truth, SEED, row0=bounds[k], n_local=bounds[k + 1] - bounds[k])
        srcs.append(s)
    with Context(0) as c, Context(0) as plain:
        tf, tp, cf, cp = [], [], [], []
        for rep in range(reps + 1):                # the first repeat is the warm-up (allocations)
            a, ca = timed_stream(plain, srcs, None, bounds)
            b, cb = timed_stream(c, srcs, labels, bounds)
            if rep:
                tp.append(a), cp.append(ca), tf.append(b), cf.append(cb)
        model = cost_model(n)
        med_p, med_f = float(np.median(tp)), float(np.median(tf))
        predicted = med_p + model["extra_total_ms"]
        S, Sp = c.xprod_matrix(), plain.xprod_matrix()
        d = np.sqrt(np.diag(Sp))
        res["formation"] = dict(
            folds_ms=tf, plain_ms=tp, folds_calls_ms=cf, plain_calls_ms=cp,
            plain_spread_ms=round(max(tp) - min(tp), 3), folds_spread_ms=round(max(tf) - min(tf), 3),
            ratio_measured=round(med_f / med_p, 4), ratio_model=round(predicted / med_p, 4),
            cost_model=model, predicted_folds_ms=round(predicted, 3),
            measured_minus_model_ms=round(med_f - predicted, 3),
            fold_total=[int(v) for v in c.stream_fold_info()["fold_total"]],
            max_S_diff_over_sqrt_diag=float(np.max(np.abs(S - Sp) / np.outer(d, d))))
        print(json.dumps(dict(formation=res["formation"])), flush=True)
        for s in srcs:
            s.close()
        # cross-validation on the streamed context
        a_list = [1, 2, 3, 4, 5]
        args = dict(EMsteps=100, atol=1e-4, initialGuess="equal")
        times, cv = [], None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            cv = crossval_PPLS(None, None, a_list, K, shared_folds=True, ctx=c, **args)
            if rep:
                times.append(round(time.perf_counter() - t0, 4))
        inits = [initial_guess(P, Q, "equal") for _ in range(max(a_list))]
        phases = dict(select_ms=[], fit_ms=[], heldout_ms=[], steps=[], cond_max=[])
        for f in range(K):
            t0 = time.perf_counter()
            c.stream_select(f)
            t1 = time.perf_counter()
            fit = c.ppls(max(a_list), args["EMsteps"], args["atol"], inits)
            t2 = time.perf_counter()
            sse, mag = c.heldout_sse_fold(fit["W"], fit["C"], fit["B"], f)
            t3 = time.perf_counter()
            phases["select_ms"].append(round((t1 - t0) * 1e3, 3))
            phases["fit_ms"].append(round((t2 - t1) * 1e3, 3))
            phases["heldout_ms"].append(round((t3 - t2) * 1e3, 3))
            phases["steps"].append([int(v) for v in fit["Other_output"]["Number_steps"]])
            phases["cond_max"].append(float(np.max(mag / sse)))
        c.stream_select(-1)
        res["cv"] = dict(a=a_list, shared_folds=True, EMsteps=100, atol=1e-4, initialGuess="equal", crossval_s=times,
                         crossval_spread_s=round(max(times) - min(times), 4), errors=[float(e) for e in cv["errors"]],
                         a_min=int(cv["a_min"]), phases=phases)
        ref = os.path.join(ROOT, "profiles", "cv_bench.json")
        if os.path.exists(ref):
            with open(ref) as f:
                res["cv"]["resident_reference"] = dict(
                    file="profiles/cv_bench.json", note="C3, xprod 1, resident rows, the same K, a and stop rule: "
                    "5.76 s; a different run, so no ratio is claimed")
    with open(outfile, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(dict(cv=res["cv"])), flush=True)


if __name__ == "__main__":
    main()
