"""Timings of the collapsed bound (svgp_collapsed_bound / _q / _grad) beside svgp_elbo and svgp_elbo_grad in the same process, on the
benchmark's synthetic problems: H (N = 1e6, M = 1024, d = 8, fp64) and C5 (N = 1e5, M = 512, d = 4, fp32) by default.  Wall times by
the host clock around calls that block until their results are on the host, after a warm-up of every call; the median of --reps
repeats with min and max.  svgp_elbo / svgp_elbo_grad are timed behind a model update each (their M-sized prep is part of an
evaluation); the collapsed calls re-prepare after svgp_collapsed_q by themselves.

    python tools/collapsed_time.py [--configs H C5] [--reps 5] [--out profiles/collapsed/collapsed_time.jsonl]

The bound has the forward ELBO's flop count (2 M^2 per point: a triangular solve and a SYRK), so the figure to watch is
bound_over_elbo."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import torch  # noqa: E402,F401  (its HIP runtime first)

from approxgp import _ffi  # noqa: E402
from approxgp.synthetic import synth_arrays  # noqa: E402

CONFIGS = {"H": (0, 1_000_000, 1024, 8, np.float64), "C5": (5, 100_000, 512, 4, np.float32),
           "small": (2, 20_000, 256, 4, np.float64)}


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [round(1e3 * statistics.median(ts), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["H", "C5"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    out = open(a.out, "w") if a.out else None
    for name in a.configs:
        cid, n, M, d, dt = CONFIGS[name]
        p = synth_arrays(cid, n, M, d, dtype=dt)
        mk = lambda: _ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"], p["jitter"],
                                    lik_sigma2=p["sigma2"])
        desc, keep = mk()
        model = _ffi.DeviceModel(ctx, desc, keep)
        data = _ffi.DeviceData(ctx, p["x"], p["y"], dt)

        def upd(fn):
            def run():
                dsc, kp = mk()
                model.update(dsc, kp)
                fn()
            return run

        calls = {"elbo_ms": upd(lambda: model.elbo(data, 0, n, float(n))),
                 "elbo_grad_ms": upd(lambda: model.elbo_grad(data, 0, n, float(n))),
                 "collapsed_bound_ms": upd(lambda: model.collapsed_bound(data, 0, n)),
                 "collapsed_q_ms": upd(lambda: model.collapsed_q(data, 0, n, fetch=False)),
                 "collapsed_grad_ms": upd(lambda: model.collapsed_grad(data, 0, n))}
        row = {"config": name, "n": n, "M": M, "d": d, "dtype": np.dtype(dt).name, "reps": a.reps}
        for k, fn in calls.items():
            fn()                      # warm-up: workspaces, first launches
            row[k] = timed(fn, a.reps)
        row["update_ms"] = timed(lambda: model.update(*mk()), a.reps)
        row["bound"] = model.collapsed_bound(data, 0, n)[0]
        row["bound_over_elbo"] = round(row["collapsed_bound_ms"][0] / row["elbo_ms"][0], 3)
        row["grad_over_elbo_grad"] = round(row["collapsed_grad_ms"][0] / row["elbo_grad_ms"][0], 3)
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        model.free()
        data.free()
    ctx.close()


if __name__ == "__main__":
    main()
