"""What the exact 1-D Matern GP in state-space form costs on the device: svgp_ss_fit and svgp_ss_predict (1e5 test times) at N = 1e6 and
1e7, Matern-3/2 and -5/2, fp64 data, and beside them one svgp_cg_fit at N = 1e5, d = 1 (tol 1e-6, 16 probes), the only other exact
route in the library.  Device time from the library's HIP events (svgp_last_timing), median [min, max] of --reps after one warm-up; the
CG fit once, by the host clock.  --samples S adds to every row the device time of one svgp_ss_sample of S joint paths at --sample-n-test
times (the kernels of every group of samples; the draws' uploads lie between the groups and are not counted) and of one svgp_ss_predict
at the same times.  Neither number is a pass / fail condition.

    python tools/ss_time.py [--reps 3] [--sizes 1000000 10000000] [--samples 64] [--append] [--no-cg] [--out profiles/statespace/ss_time.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))


def stat(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--n-test", type=int, default=100_000)
    ap.add_argument("--cg-n", type=int, default=100_000)
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--sample-n-test", type=int, default=1000)
    ap.add_argument("--append", action="store_true", help="append the rows to --out instead of replacing it")
    ap.add_argument("--no-cg", action="store_true", help="leave the svgp_cg_fit row out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statespace", "ss_time.jsonl"))
    a = ap.parse_args()
    import approxgp
    from approxgp import _ffi
    from approxgp.statespace import DeviceStateSpace

    ctx = _ffi.Context(0)
    rng = np.random.default_rng(0)
    rows = []
    for N in a.sizes:
        t = np.sort(rng.uniform(0.0, N / 100.0, N))
        y = np.sin(t) + 0.3 * rng.standard_normal(N)
        ts = np.sort(rng.uniform(t[0], t[-1], a.n_test))
        dev = DeviceStateSpace(ctx, t, y, np.float64)
        for name, base in (("matern32", approxgp.Matern32Kernel()), ("matern52", approxgp.Matern52Kernel())):
            desc = dev.desc(1.0 * approxgp.with_lengthscale(base, 1.0), 0.09)
            fit, pred = [], []
            for r in range(a.reps + 1):
                lml, info = dev.fit(desc)
                fit.append(info.ms_total)
                dev.predict(ts)
                pred.append(ctx.timing().ms_total)
            rows.append({"call": "svgp_ss_fit + svgp_ss_predict", "kernel": name, "N": N, "n_test": a.n_test, "dtype": "float64",
                         "fit_ms": stat(fit[1:]), "predict_ms": stat(pred[1:]), "levels": info.levels, "lml": lml})
            if a.samples > 0:   # the times are sorted: the library's draw layout is the caller's, no reordering copy of z
                tq = np.ascontiguousarray(ts[np.linspace(0, ts.shape[0] - 1, a.sample_n_test).astype(int)])
                z = rng.standard_normal((a.samples, N + tq.shape[0], info.state_dim))
                eps, out = rng.standard_normal((a.samples, N)), np.zeros((a.samples, tq.shape[0]))
                smp, prs = [], []
                for r in range(a.reps + 1):
                    dev._check(ctx.lib.svgp_ss_sample(ctx.h, dev.h, tq.shape[0], _ffi._ptr(tq), a.samples, _ffi._ptr(z), _ffi._ptr(eps), _ffi._ptr(out)))
                    smp.append(ctx.timing().ms_total)
                    dev.predict(tq)
                    prs.append(ctx.timing().ms_total)
                rows[-1].update({"samples": a.samples, "sample_n_test": int(tq.shape[0]), "sample_ms": stat(smp[1:]), "predict_same_n_ms": stat(prs[1:])})
                del z, eps
            print(json.dumps(rows[-1]), flush=True)
        dev.free()
    if not a.no_cg:
        rows.append(cg_row(ctx, rng, a.cg_n))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


def cg_row(ctx, rng, N):
    import approxgp
    from approxgp.statespace import DeviceStateSpace

    t = np.sort(rng.uniform(0.0, N / 100.0, N))
    y = np.sin(t) + 0.3 * rng.standard_normal(N)
    cg = approxgp.DeviceConjugateGradients(ctx, t, y, np.float64)
    desc, keep = cg.desc(1.0 * approxgp.with_lengthscale(approxgp.Matern32Kernel(), 1.0), 0.09, tol=1e-6, maxiter=1000)
    t0 = time.perf_counter()
    lml, info = cg.fit(desc, approxgp.draw_probes(N, 16, 0))
    wall = (time.perf_counter() - t0) * 1e3
    cg.free()
    dev = DeviceStateSpace(ctx, t, y, np.float64)
    lml_ss, info_ss = dev.fit(dev.desc(1.0 * approxgp.with_lengthscale(approxgp.Matern32Kernel(), 1.0), 0.09))
    dev.free()
    return {"call": "svgp_cg_fit", "kernel": "matern32", "N": N, "d": 1, "dtype": "float64", "wall_ms": round(wall, 1),
            "iterations": info.iterations, "converged": info.converged, "lml_cg": lml, "lml_ss": lml_ss, "ss_fit_ms": round(info_ss.ms_total, 3)}


if __name__ == "__main__":
    main()
