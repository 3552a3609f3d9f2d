"""Laplace approximation timings (csrc/laplace.hip): per Newton step the device time of the point kernels (+ B assembly), the
factorisation cholesky(B), L^-1 and the GEMVs (svgp_laplace_info, HIP events), iterations to convergence, approx_lml and value-and-
gradient wall times (host clock around calls that end in a device synchronise), and the same approx_lml in numpy on the host
(tests/laplace_ref.py).  Bernoulli-logistic, SE with ARD, d = 8, jitter 1e-6.

    python tools/laplace_time.py [--sizes 2048 4096 8192] [--host-max 4096] [--reps 3]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096, 8192])
    ap.add_argument("--host-max", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
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
