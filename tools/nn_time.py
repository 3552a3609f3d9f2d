"""NearestNeighbors (Vecchia) timings (csrc/nn.hip): approx_lml, value-and-gradient, fit and predict (n* = 1024, mean + var) for
SE-ARD, d = 8, at N in {1e4, 1e5, 1e6}, k in {16, 32, 64}, fp64 and fp32.  Wall times by the host clock around calls that end in a
device synchronise, after a warm-up of every shape; the median of --reps repeats, with the spread.  Beside each k the numpy
restatement (tests/nn_ref.py lml_joint: one Cholesky per point, no N x N matrix) at --host-n points, the largest size it
finishes well under a minute at.

    python tools/nn_time.py [--sizes 10000 100000 1000000] [--ks 16 32 64] [--reps 5] [--host-n 10000] [--out profiles/nn/nn_time.jsonl]

Rate: k^3 / 3 + 2 k^2 + k^2 (3 d + 20) / 2 flops per point (factorisation, the two carried rows, block generation) over the
approx_lml wall time, against the FP64 / FP32 vector peaks 78.6 / 157.3 TFLOP/s (MI355X_MICROARCH.md, AMD's published FP64 figure).
The device clock torch reports is noted per row when available.

    python tools/nn_time.py --local [--local-n 200000] [--local-nq 4096] [--ks 16 64] [--local-ds 2 8] [--out ...]

times the local predictions (svgp_nn_predict_local, mean + var) beside svgp_nn_predict (window, and with the nearest table unless
--local-no-table) at the same N, n*, k and dtype, and writes their ratio; --out appends in this mode.  Cost model: global n* N
kernel evaluations (n* N (kb + 1) with a table), local n* N distances of 3 d flops plus n* (k^2 (3 d + 20) / 2 + k^3 / 3)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402,F401  (its HIP runtime first)

import nn_ref as nr  # noqa: E402
from approxgp import DeviceNearestNeighbors, _ffi  # noqa: E402
from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel  # noqa: E402

PEAK_TF = {"float64": 78.6, "float32": 157.3}


def flops_per_point(k, d):
    return k ** 3 / 3 + 2 * k ** 2 + k ** 2 * (3 * d + 20) / 2


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def local_rows(a, emit):
    """predict_local beside predict at one N, n*: a row per (d, dtype, k)"""
    ctx = _ffi.Context(0)
    var, diag, n, nq = 1.2, 1e-2, a.local_n, a.local_nq
    for d in a.local_ds:
        il = np.linspace(0.8, 1.1, d)
        kern = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(il)), var)
        x, y = nr.synth(n, d, seed=1)
        xs = np.random.default_rng(2).uniform(-2, 2, size=(d, nq))
        for dt in (np.float64, np.float32):
            dev = DeviceNearestNeighbors(ctx, x.astype(dt), y.astype(dt), dt)
            xq = xs.astype(dt)
            for k in a.ks:
                desc, keep = dev.desc(kern, k, diag)
                dev.fit(desc)
                dev.predict(xq, cov=False)      # warm-up of every shape
                dev.predict_local(xq, k)
                t_glob = timed(lambda: dev.predict(xq, cov=False), a.reps)
                t_loc = timed(lambda: dev.predict_local(xq, k), a.reps)
                row = {"local": True, "n": n, "nq": nq, "k": k, "d": d, "dtype": np.dtype(dt).name, "clock_mhz": clock_mhz(), "reps": a.reps,
                       "predict_window_ms": [round(v, 3) for v in t_glob], "predict_local_ms": [round(v, 3) for v in t_loc],
                       "window_over_local": round(t_glob[0] / t_loc[0], 3),
                       "local_gdist_per_s": round(n * nq / (t_loc[0] * 1e-3) / 1e9, 2)}
                if not a.local_no_table:
                    dev.build_neighbors(k, il)
                    dev.fit(desc)
                    dev.predict(xq, cov=False)
                    t_tab = timed(lambda: dev.predict(xq, cov=False), a.reps)
                    row["predict_table_ms"] = [round(v, 3) for v in t_tab]
                    row["table_over_local"] = round(t_tab[0] / t_loc[0], 3)
                    dev.clear_neighbors()
                emit(row)
            dev.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--local", action="store_true", help="only the predict_local rows")
    ap.add_argument("--local-n", type=int, default=200_000)
    ap.add_argument("--local-nq", type=int, default=4096)
    ap.add_argument("--local-ds", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--local-no-table", action="store_true", help="skip the table-mode svgp_nn_predict (its search is N^2 / 2 distances)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=10_000)
    ap.add_argument("--table-max-n", type=int, default=100_000, help="largest N that also gets the neighbour-table rows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a" if a.local else "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if a.local:
        local_rows(a, emit)
        return
    ctx = _ffi.Context(0)
    d, var, diag = 8, 1.2, 1e-2
    il = np.linspace(0.8, 1.1, d)
    kern = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(il)), var)
    host = {}
    for k in a.ks:
        x, y = nr.synth(a.host_n, d, seed=1)
        t0 = time.perf_counter()
        ref = nr.lml_joint(nr.kernel_of(0, var, il), x, y, k, diag)
        host[k] = (1e3 * (time.perf_counter() - t0), ref)
        emit({"host_numpy": True, "n": a.host_n, "k": k, "approx_lml_ms": round(host[k][0], 1), "lml": ref})
    for n in a.sizes:
        x, y = nr.synth(n, d, seed=1)
        xs = np.random.default_rng(2).uniform(-2, 2, size=(d, 1024))
        for dt in (np.float64, np.float32):
            dev = DeviceNearestNeighbors(ctx, x.astype(dt), y.astype(dt), dt)
            for k in a.ks:
                desc, keep = dev.desc(kern, k, diag)
                lml = dev.lml(desc)[0]      # warm-up of every shape
                dev.lml_grad(desc)
                dev.fit(desc)
                dev.predict(xs.astype(dt))
                t_lml = timed(lambda: dev.lml(desc), a.reps)
                t_grad = timed(lambda: dev.lml_grad(desc), a.reps)
                t_fit = timed(lambda: dev.fit(desc), a.reps)
                t_pred = timed(lambda: dev.predict(xs.astype(dt)), a.reps)
                name = np.dtype(dt).name
                tf = n * flops_per_point(k, d) / (t_lml[0] * 1e-3) / 1e12
                row = {"n": n, "k": k, "dtype": name, "lml": lml, "clock_mhz": clock_mhz(), "reps": a.reps,
                       "approx_lml_ms": [round(v, 3) for v in t_lml], "value_and_grad_ms": [round(v, 3) for v in t_grad],
                       "fit_ms": [round(v, 3) for v in t_fit], "predict_1024_mean_var_ms": [round(v, 3) for v in t_pred],
                       "lml_tflops": round(tf, 3), "share_of_vector_peak": round(tf / PEAK_TF[name], 4)}
                if n == a.host_n and dt == np.float64:
                    row["host_numpy_approx_lml_ms"] = round(host[k][0], 1)
                    row["host_rel_diff"] = abs(lml - host[k][1]) / abs(host[k][1])
                emit(row)
                if n > a.table_max_n:   # the brute-force search is N^2 / 2 distances
                    continue
                # the same N, k and dtype with the k nearest predecessors as a table; the window row above is the yardstick
                dev.build_neighbors(k, il)
                t_build = timed(lambda: dev.build_neighbors(k, il), a.reps)
                lml_t = dev.lml(desc)[0]
                dev.lml_grad(desc)
                dev.fit(desc)
                dev.predict(xs.astype(dt))
                tt = {"approx_lml_ms": timed(lambda: dev.lml(desc), a.reps), "value_and_grad_ms": timed(lambda: dev.lml_grad(desc), a.reps),
                      "fit_ms": timed(lambda: dev.fit(desc), a.reps), "predict_1024_mean_var_ms": timed(lambda: dev.predict(xs.astype(dt)), a.reps)}
                rowt = {"n": n, "k": k, "dtype": name, "neighbors": "nearest", "lml": lml_t, "reps": a.reps,
                        "build_ms": [round(v, 3) for v in t_build], "build_gdist_per_s": round(n * n / 2 / (t_build[0] * 1e-3) / 1e9, 2)}
                for key, v in tt.items():
                    rowt[key] = [round(u, 3) for u in v]
                    rowt[key.replace("_ms", "_over_window")] = round(v[0] / row[key][0], 3)
                emit(rowt)
                dev.clear_neighbors()
            dev.free()
    ctx.close()


if __name__ == "__main__":
    main()
