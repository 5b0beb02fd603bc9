"""Time the streamed-data path (ppls_stream_*).

    python tools/bench_stream.py [c3,overlap,big] [--out profiles/stream_bench.json] [--scale 1.0]

Three measurements at p = q = 2000, each a key of the one JSON line written to --out (keys of an
existing file that are not measured again are kept, so the parts may run one by one; a part that is
measured again keeps its earlier figures under ``<part>_previous_run``):

c3       n = 1e6 fed as ten device chunks (``generate_synthetic`` into ten source contexts, then
         ``stream_rows_from``) with center = scale = 1, five repeats of begin .. end (wall clock).
         Yardstick, in the same process: the resident path on the same rows, ``scale_data()`` +
         ``xprod_prepare()``, five repeats.  Beside them the cost model of the extra passes: per
         chunk one mean pass (a read), one centring pass (read + write) and the stage copy (read +
         write) at the rates DESIGN §15 measured, and one merge pass over S (read + write of 128 MB
         plus the Gram partials).
overlap  n = 2.5e5 rows on the host (8 GB, row-major) in chunks of 25,000: wall time of the streamed
         load against upload-only (the same chunks copied to the device, nothing else) and
         device-work-only (the same chunks already resident in a source context) runs; the ratio to
         max(upload, device work) is 1.0 for perfect overlap.
big      n = 1e7 (320 GB of rows, more than HBM) in chunks of 1e5 rows generated on the device and fed
         through ``stream_rows_from``; then ``PPLS_simult(None, None, 5)``.  Formation time, fit time
         and the smallest free HBM seen.

--scale s multiplies every n by s (a quick run on a smaller problem; the JSON records it).
"""
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_truth_and_theta0  # noqa: E402
from ppls_amd import Context, PPLS_simult  # noqa: E402

P = Q = 2000
SEED = 20261019
READ_TBPS = 6.75        # the column-sum passes at C3
RW_TBPS = 5.2           # the in-place apply pass (bytes read + written)
PARENT_MS = dict(scale_data=22.0, xprod_prepare=230.0)   # README: the resident path at C3


_HIP = ct.CDLL("libamdhip64.so")
_HIP.hipMalloc.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t]
_HIP.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
_HIP.hipFree.argtypes = [ct.c_void_p]


def _hip(rc):
    if rc != 0:
        raise RuntimeError(f"HIP runtime call failed with error {rc}")


def free_hbm():
    free, total = ct.c_size_t(), ct.c_size_t()
    _hip(_HIP.hipMemGetInfo(ct.byref(free), ct.byref(total)))
    return free.value


def cost_model(n, nchunks, nsplit_per_chunk=8):
    """Extra milliseconds of the streamed formation over the resident scale_data + xprod_prepare."""
    row_bytes = 8.0 * (P + Q)
    data = n * row_bytes
    s_bytes = 8.0 * (P + Q) ** 2
    quads = ((P + Q + 127) // 128) * (((P + Q + 127) // 128) + 1) // 2 * 4
    part = nsplit_per_chunk * quads * 64 * 64 * 8.0
    stream = dict(mean_pass=data / READ_TBPS / 1e9, centring_pass=2 * data / RW_TBPS / 1e9,
                  stage_copy=2 * data / RW_TBPS / 1e9,
                  merge_passes=nchunks * (2 * s_bytes + part) / RW_TBPS / 1e9)
    resident = dict(two_stat_passes=2 * data / READ_TBPS / 1e9, apply_pass=2 * data / RW_TBPS / 1e9,
                    gram_finish=(s_bytes + part) / RW_TBPS / 1e9)
    return dict(streamed_ms=stream, resident_ms=resident,
                extra_ms=round(sum(stream.values()) - sum(resident.values()), 3),
                note="both paths run the same MFMA Gram flops; chunked Grams have shorter row splits")


def bench_c3(scale):
    n = int(1_000_000 * scale)
    nch = 10
    truth, _ = make_truth_and_theta0(P, Q, 5)
    bounds = [n * k // nch for k in range(nch + 1)]
    out = dict(n=n, chunks=nch, repeats=5)
    srcs = []
    for k in range(nch):
        s = Context(0)
        s.generate_synthetic(n, P, Q, truth, SEED, row0=bounds[k], n_local=bounds[k + 1] - bounds[k])
        srcs.append(s)
    with Context(0) as c:
        times, ends, calls = [], [], []
        for rep in range(6):                       # one warm-up (allocations), five timed
            c.synchronize()
            t0 = time.perf_counter()
            c.stream_begin(P, Q, True, True)
            stamps = [time.perf_counter()]
            for s in srcs:
                c.stream_rows_from(s)
                stamps.append(time.perf_counter())
            t1 = time.perf_counter()
            res = c.stream_end()
            t2 = time.perf_counter()
            if rep:
                times.append(round((t2 - t0) * 1e3, 3))
                ends.append(round((t2 - t1) * 1e3, 3))
                # wall time of every call: [begin, the ten stream_rows_from calls ..., end]
                calls.append([round((b - a) * 1e3, 2) for a, b in zip([t0] + stamps, stamps + [t2])])
        out["calls_ms"] = calls
        ssq = c.ssq()
        S = c.xprod_matrix()
        out.update(streamed_ms=times, of_which_stream_end_ms=ends, ssq=[ssq[0], ssq[1]], n_streamed=res["n"],
                   free_hbm_gb=round(free_hbm() / 1e9, 2))
    for s in srcs:
        s.close()
    with Context(0) as r:
        r.generate_synthetic(n, P, Q, truth, SEED)
        par, parts = [], []
        for rep in range(6):
            r.synchronize()
            t0 = time.perf_counter()
            r.scale_data(True, True)
            t1 = time.perf_counter()
            r.xprod_prepare()
            t2 = time.perf_counter()
            if rep:
                par.append(round((t2 - t0) * 1e3, 3))
                parts.append([round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3)])
        Sr = r.xprod_matrix()
        out.update(resident_ms=par, resident_scale_prepare_ms=parts)
    d = np.sqrt(np.diag(Sr))
    out["max_S_diff_over_sqrt_diag"] = float(np.max(np.abs(S - Sr) / np.outer(d, d)))
    out["cost_model"] = cost_model(n, nch)
    out["readme_parent_ms"] = PARENT_MS
    out["streamed_min_over_resident_max"] = round(min(times) / max(par), 4)
    out["excess_over_slowest_resident_ms"] = round(min(times) - max(par), 3)
    return out


def bench_overlap(scale):
    n = int(250_000 * scale)
    rows = int(25_000 * scale)
    truth, _ = make_truth_and_theta0(P, Q, 5)
    with Context(0) as g:
        g.generate_synthetic(n, P, Q, truth, SEED)
        X, Y = g.get_data_rows()                   # the host array: n x 4000 doubles
    chunks = [(X[i:i + rows], Y[i:i + rows]) for i in range(0, n, rows)]
    out = dict(n=n, chunk_rows=rows, chunks=len(chunks), host_gb=round((X.nbytes + Y.nbytes) / 1e9, 2))
    with Context(0) as c:
        def streamed():
            c.stream_begin(P, Q, True, True)
            for Xc, Yc in chunks:
                c.stream_rows(Xc, Yc)
            c.stream_end()

        dbuf = ct.c_void_p()
        _hip(_HIP.hipMalloc(ct.byref(dbuf), chunks[0][0].nbytes))

        def upload_only():                         # plain hipMemcpy of every chunk, host to device
            for Xc, Yc in chunks:
                _hip(_HIP.hipMemcpy(dbuf, Xc.ctypes.data, Xc.nbytes, 1))
                _hip(_HIP.hipMemcpy(dbuf, Yc.ctypes.data, Yc.nbytes, 1))

        with Context(0) as src:
            def device_only():
                c.stream_begin(P, Q, True, True)
                for _ in chunks:
                    c.stream_rows_from(src)
                c.stream_end()

            src.set_data(*chunks[0])
            for name, fn in (("streamed_ms", streamed), ("upload_only_ms", upload_only), ("device_only_ms", device_only)):
                ts = []
                for rep in range(3):               # the first is the warm-up
                    t0 = time.perf_counter()
                    fn()
                    ts.append(round((time.perf_counter() - t0) * 1e3, 2))
                out[name] = ts[1:]
        _hip(_HIP.hipFree(dbuf))
    best = {k: min(out[k]) for k in ("streamed_ms", "upload_only_ms", "device_only_ms")}
    out["ratio_to_max_upload_device"] = round(best["streamed_ms"] / max(best["upload_only_ms"], best["device_only_ms"]), 4)
    out["ratio_to_sum_upload_device"] = round(best["streamed_ms"] / (best["upload_only_ms"] + best["device_only_ms"]), 4)
    return out


def bench_big(scale):
    n = int(10_000_000 * scale)
    rows = int(100_000 * scale) or 1
    truth, _ = make_truth_and_theta0(P, Q, 5)
    out = dict(n=n, chunk_rows=rows, rows_gb=round(n * 8.0 * (P + Q) / 1e9, 1), free_hbm_before_gb=round(free_hbm() / 1e9, 2))
    low = free_hbm()
    with Context(0) as c, Context(0) as src:
        t_gen = t_stream = 0.0
        t0 = time.perf_counter()
        c.stream_begin(P, Q, True, True)
        for lo in range(0, n, rows):
            ta = time.perf_counter()
            src.generate_synthetic(n, P, Q, truth, SEED, row0=lo, n_local=min(rows, n - lo))
            tb = time.perf_counter()
            c.stream_rows_from(src)
            t_stream += time.perf_counter() - tb
            t_gen += tb - ta
            low = min(low, free_hbm())
        ta = time.perf_counter()
        res = c.stream_end()
        t_stream += time.perf_counter() - ta
        out.update(n_streamed=res["n"], chunks=c.stream_info()["chunks"], total_s=round(time.perf_counter() - t0, 3),
                   generate_s=round(t_gen, 3), stream_calls_s=round(t_stream, 3))
        src.close()
        t0 = time.perf_counter()
        fit = PPLS_simult(None, None, 5, ctx=c, seed=1)
        out.update(fit_s=round(time.perf_counter() - t0, 3), fit_steps=int(len(fit["loglik"])),
                   loglik_last=float(fit["loglik"][-1]), sigE=float(fit["estimates"]["sigE"]),
                   mu_T_is_None=fit["Expectations"]["mu_T"] is None)
        low = min(low, free_hbm())
    out.update(free_hbm_min_gb=round(low / 1e9, 2),
               peak_hbm_used_gb=round((out["free_hbm_before_gb"] * 1e9 - low) / 1e9, 2))
    return out


def main():
    argv = sys.argv[1:]
    parts = argv[0].split(",") if argv and not argv[0].startswith("-") else ["c3", "overlap", "big"]
    outfile = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "stream_bench.json")
    scale = float(argv[argv.index("--scale") + 1]) if "--scale" in argv else 1.0
    res = dict(tool="tools/bench_stream.py", p=P, q=Q)
    if os.path.exists(outfile):
        with open(outfile) as f:
            res.update(json.loads(f.readline() or "{}"))
    for name in parts:
        r = dict(c3=bench_c3, overlap=bench_overlap, big=bench_big)[name](scale)
        if scale != 1.0:
            r["scale"] = scale
        if name in res:                            # a part measured again: the earlier figures stay beside the new
            res[name + "_previous_run"] = res[name]
        res[name] = r
        print(json.dumps({name: r}), flush=True)
        with open(outfile, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
