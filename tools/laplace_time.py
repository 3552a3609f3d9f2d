"""Laplace approximation timings (csrc/laplace.hip): per Newton step the device time of the point kernels (+ B assembly), the
factorisation cholesky(B), L^-1 and the GEMVs (svgp_laplace_info, HIP events), iterations to convergence, approx_lml and value-and-
gradient wall times (host clock around calls that end in a device synchronise), and the same approx_lml in numpy on the host
(tests/laplace_ref.py).  Bernoulli-logistic, SE with ARD, d = 8, jitter 1e-6.

    python tools/laplace_time.py [--sizes 2048 4096 8192] [--host-max 4096] [--reps 3]
    python tools/laplace_time.py --xgrad [--sizes 4096 8192] [--reps 3]     # after tools/build_prev.sh; -> profiles/laplace/laplace_xgrad_time.jsonl

--xgrad: what the input gradient costs.  svgp_laplace_lml_grad_inputs of this tree (x_bar into device memory) beside svgp_laplace_lml_grad
of the parent commit's library (--prev-lib), cold starts, one process per leg, interleaved, medians of --reps rounds of wall times (each
call ends in a device synchronise); and the device time of the one N x N pass of csrc/laplace_xgrad.hip with its finish kernel from
HIP events around the two (svgp_last_timing).  That pass reads R once: N^2 elements over the pass's own time is its rate.

Rates: N^3 / 3 flops for cholesky(B) and for L^-1 each, over their device times; the GEMVs stream K twice and the two triangles of
L^-1 once each (3 N^2 elements per step).  Peaks: FP32 matrix 157.3 TFLOP/s and HBM 8 TB/s (MI355X_MICROARCH.md); FP64 matrix
78.6 TFLOP/s (AMD's published figure)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import laplace_ref as lr  # noqa: E402
from approxgp import BernoulliLikelihood, DeviceLaplace, _ffi  # noqa: E402
from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel  # noqa: E402

PEAK_TF = {np.float64: 78.6, np.float32: 157.3}
PEAK_TBS = 8.0


def xgrad_child(leg, sizes, inner):
    """One process of --xgrad: per (N, dtype) one warm-up call, then the median wall time of `inner` cold-start calls, one JSON line each.
    leg `new`: svgp_laplace_lml_grad_inputs of this tree into device memory, and the device time of its pass alone (svgp_last_timing:
    HIP events around lp_xgrad_kernel and its finish kernel).  leg `prev`: svgp_laplace_lml_grad of a library without the new symbol."""
    import torch

    if leg == "prev":
        _ffi.SYMBOLS.pop("svgp_laplace_lml_grad_inputs", None)
    ctx = _ffi.Context(0)
    d = 8
    kern = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.full(d, 0.5))), 1.0)
    for n in sizes:
        x, y = lr.synth(1, n, d, seed=n)
        for dt in (np.float64, np.float32):
            dev = DeviceLaplace(ctx, x.astype(dt), y.astype(dt), dt)
            desc, keep = dev.desc(kern, BernoulliLikelihood(), 1e-6)
            xbar = torch.empty((d, n), dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda")
            torch.cuda.synchronize()
            call = (lambda: dev.lml_grad(desc, wrt_inputs=True, x_grad_out=xbar)) if leg == "new" else (lambda: dev.lml_grad(desc))
            call()
            wall, dev_ms = [], []
            for _ in range(inner):
                t0 = time.perf_counter()
                r = call()
                wall.append(1e3 * (time.perf_counter() - t0))
                dev_ms.append(ctx.timing().ms_strip if leg == "new" else 0.0)
            dev.free()
            print(json.dumps({"n": n, "dtype": np.dtype(dt).name, "iterations": r[-1].iterations, "ms_wall": float(np.median(wall)),
                              "ms_pass": float(np.median(dev_ms)), "finite": bool(torch.isfinite(xbar).all()) if leg == "new" else True,
                              "lml_grad_hex": [float(v).hex() for v in (r[0], r[1], *r[2])]}), flush=True)
    ctx.close()


def xgrad(a):
    """--xgrad: this tree's svgp_laplace_lml_grad_inputs against svgp_laplace_lml_grad of the library --prev-lib (the parent commit's:
    tools/build_prev.sh), one process per leg, interleaved new / prev, medians over --reps rounds."""
    import statistics
    import subprocess

    if not os.path.exists(a.prev_lib):
        raise SystemExit(f"{a.prev_lib} is missing: tools/build_prev.sh builds the parent commit's library")
    sizes = a.sizes or [4096, 8192]
    runs = {"new": [], "prev": []}
    for _ in range(a.reps):
        for leg in ("new", "prev"):
            env = dict(os.environ)
            if leg == "prev":
                env["SVGP_MI355X_LIB"] = os.path.abspath(a.prev_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--xgrad-child", leg, "--inner", str(a.inner), "--sizes", *map(str, sizes)]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit(f"leg {leg} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            runs[leg].append([json.loads(ln) for ln in res.stdout.splitlines() if ln.startswith("{")])
    with open(a.xgrad_out, "w") as out:
        for i in range(len(runs["new"][0])):
            new, prev = [r[i] for r in runs["new"]], [r[i] for r in runs["prev"]]
            mn, mp = statistics.median(r["ms_wall"] for r in new), statistics.median(r["ms_wall"] for r in prev)
            es = 8 if new[0]["dtype"] == "float64" else 4
            ps = statistics.median(r["ms_pass"] for r in new)
            row = {"n": new[0]["n"], "d": 8, "dtype": new[0]["dtype"], "iterations": new[0]["iterations"], "rounds": a.reps, "calls_per_round": a.inner,
                   "lml_grad_inputs_ms": round(mn, 3), "lml_grad_inputs_ms_rounds": [round(r["ms_wall"], 3) for r in new],
                   "parent_lml_grad_ms": round(mp, 3), "parent_lml_grad_ms_rounds": [round(r["ms_wall"], 3) for r in prev],
                   "ratio": round(mn / mp, 4), "xgrad_pass_device_ms": round(ps, 4), "pass_share_of_call": round(ps / mn, 5),
                   "r_read_tbs_over_pass": round(new[0]["n"] ** 2 * es / (ps * 1e-3) / 1e12, 3) if ps > 0 else None, "peak_tbs": PEAK_TBS,
                   "lml_grad_bitwise_parent": all(r["lml_grad_hex"] == prev[0]["lml_grad_hex"] for r in new + prev),
                   "finite": all(r["finite"] for r in new)}
            print(json.dumps(row), flush=True)
            out.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--xgrad", action="store_true", help="svgp_laplace_lml_grad_inputs beside the parent commit's svgp_laplace_lml_grad")
    ap.add_argument("--xgrad-child", choices=("new", "prev"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--inner", type=int, default=5, help="--xgrad: timed calls per process (their median is the process's figure)")
    ap.add_argument("--prev-lib", default=os.path.join(ROOT, "approximategps.jl_amd", "csrc", "ablate", "libsvgp_prev.so"))
    ap.add_argument("--xgrad-out", default=os.path.join(ROOT, "profiles", "laplace", "laplace_xgrad_time.jsonl"))
    ap.add_argument("--sizes", type=int, nargs="+", default=None)
    ap.add_argument("--host-max", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.xgrad_child:
        return xgrad_child(a.xgrad_child, a.sizes, a.inner)
    if a.xgrad:
        return xgrad(a)
    ctx = _ffi.Context(0)
    a.sizes = a.sizes or [2048, 4096, 8192]
    d = 8
    il = np.full(d, 0.5)
    kern = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(il)), 1.0)
    for n in a.sizes:
        x, y = lr.synth(1, n, d, seed=n)
        for dt in (np.float64, np.float32):
            dev = DeviceLaplace(ctx, x.astype(dt), y.astype(dt), dt)
            desc, keep = dev.desc(kern, BernoulliLikelihood(), 1e-6)
            dev.fit(desc)
            dev.lml_grad(desc)   # warm-up of every shape
            t_fit, t_grad = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                lml, info = dev.fit(desc)
                t_fit.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                dev.lml_grad(desc)
                t_grad.append(time.perf_counter() - t0)
            dev.free()
            steps = info.iterations + (0 if info.converged else 1)
            per = {k: getattr(info, k) / steps for k in ("ms_point", "ms_chol", "ms_linv", "ms_gemv")}
            es = np.dtype(dt).itemsize
            row = {"n": n, "dtype": np.dtype(dt).name, "iterations": info.iterations, "converged": info.converged, "lml": lml,
                   "step_ms": {k: round(v, 4) for k, v in per.items()},
                   "solves_plus_gemv_ms": round(per["ms_linv"] + per["ms_gemv"], 4),
                   "chol_tflops": round(n ** 3 / 3 / (per["ms_chol"] * 1e-3) / 1e12, 2),
                   "linv_tflops": round(n ** 3 / 3 / (per["ms_linv"] * 1e-3) / 1e12, 2),
                   "gemv_tbs": round(3 * n * n * es / (per["ms_gemv"] * 1e-3) / 1e12, 2),
                   "approx_lml_ms": round(1e3 * min(t_fit), 2), "value_and_grad_ms": round(1e3 * min(t_grad), 2),
                   "peak_tflops": PEAK_TF[dt], "peak_tbs": PEAK_TBS}
            if dt == np.float64 and n <= a.host_max:
                t0 = time.perf_counter()
                ref = lr.fit(lr.kernel_of(0, 1.0, il), x, y, 1, jitter=1e-6)[0]
                row["host_numpy_approx_lml_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                row["host_rel_diff"] = abs(lml - ref) / abs(ref)
            print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
