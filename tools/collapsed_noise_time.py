"""Timings of the collapsed bound with per-point noise variances and prior mean offsets (svgp_collapsed_bound_with_noise /
_grad_with_noise, device-resident mux, s and s_bar / mux_bar) beside the plain svgp_collapsed_bound / _grad and svgp_elbo in the same
process, on the benchmark's synthetic problems: H (N = 1e6, M = 1024, d = 8, fp64) and C5 (N = 1e5, M = 512, d = 4, fp32) by default.
Wall times by the host clock around calls that block until their results are on the host, behind a model update each, after a warm-up
of every call; the median of --reps repeats with min and max.

    python tools/collapsed_noise_time.py [--configs H C5] [--reps 3] [--out profiles/collapsed/collapsed_noise_time.jsonl]
    SVGP_MI355X_LIB=approximategps.jl_amd/csrc/ablate/libsvgp_prev.so python tools/collapsed_noise_time.py --plain-only ...

--plain-only times the calls an earlier library has as well (tools/build_prev.sh builds the parent commit's): run the two interleaved
on one box for the A/B of the NULL path; every row carries the bound and the ELBO so that the outputs can be compared bitwise."""
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

import torch  # noqa: E402  (its HIP runtime first)

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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default="tree")
    a = ap.parse_args()
    if a.plain_only:   # an earlier library does not export the newest symbols: do not ask it for them
        for k in [k for k in _ffi.SYMBOLS if k.endswith("_with_noise")]:
            del _ffi.SYMBOLS[k]
    ctx = _ffi.Context(0)
    out = open(a.out, "a") if a.out else None
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
                return fn()
            return run

        calls = {"elbo_ms": upd(lambda: model.elbo(data, 0, n, float(n))),
                 "collapsed_bound_ms": upd(lambda: model.collapsed_bound(data, 0, n)),
                 "collapsed_grad_ms": upd(lambda: model.collapsed_grad(data, 0, n))}
        if not a.plain_only:
            rng = np.random.default_rng(7)
            tdt = torch.float64 if dt == np.float64 else torch.float32
            # noise over two orders of magnitude above lik_sigma2, offsets of the size of y: device-resident, as a training loop holds them
            s = torch.tensor((p["sigma2"] * (10.0 ** (2.0 * rng.random(n)) - 1.0)).astype(dt), device="cuda")
            mux = torch.tensor((0.3 * np.cos(np.arange(n) * 1e-3)).astype(dt), device="cuda")
            sbar, mbar = torch.zeros(n, dtype=tdt, device="cuda"), torch.zeros(n, dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            calls["noise_bound_ms"] = upd(lambda: model.collapsed_bound(data, 0, n, prior_mean=mux, noise=s))
            calls["mean_only_bound_ms"] = upd(lambda: model.collapsed_bound(data, 0, n, prior_mean=mux))
            calls["noise_grad_ms"] = upd(lambda: model.collapsed_grad(data, 0, n, prior_mean=mux, noise=s, want_mean_grad=mbar,
                                                                      want_noise_grad=sbar))
        row = {"config": name, "lib": a.tag, "n": n, "M": M, "d": d, "dtype": np.dtype(dt).name, "reps": a.reps}
        for k, fn in calls.items():
            fn()                      # warm-up: workspaces, first launches
            row[k] = timed(fn, a.reps)
        row["bound"] = calls["collapsed_bound_ms"]()[0]
        row["elbo"] = calls["elbo_ms"]()[0]
        if not a.plain_only:
            row["noise_bound"] = calls["noise_bound_ms"]()[0]
            row["noise_over_plain_bound"] = round(row["noise_bound_ms"][0] / row["collapsed_bound_ms"][0], 3)
            row["noise_over_plain_grad"] = round(row["noise_grad_ms"][0] / row["collapsed_grad_ms"][0], 3)
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
