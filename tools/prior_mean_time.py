"""Cost of prior mean offsets: each call without offsets against the same call with them, on one context, interleaved per repetition;
min and median wall time of each.  Forward: svgp_elbo vs svgp_elbo_with_mean (device mux, host mux).  Value and gradient: svgp_elbo_grad
vs svgp_elbo_grad_with_mean (device mux and device mux_bar; host mux and host mux_bar).  The model carries muz in every "+mean" call.
usage: tools/prior_mean_time.py [bench.py config names, default H C5] [--reps R]"""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(R, ".."))
sys.path.insert(0, os.path.join(R, "..", "approximategps.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

import bench  # noqa: E402
from approxgp import _ffi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["H", "C5"])
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
print(f"# python tools/prior_mean_time.py {' '.join(args.configs)} --reps {args.reps}  (interleaved per repetition; median and min of "
      f"{args.reps})", flush=True)

ctx = _ffi.Context(0)
for cfg in args.configs:
    n, M, d, family, lik, dtype, cid = bench.CONFIGS[cfg]
    nd = bench.C5_NUM_DATA if cfg == "C5" else float(n)
    p = bench.synth(cid, n, M, d, family, lik, dtype)
    desc, keep = _ffi.make_desc(p["np_dt"], family, p["variance"], p["inv_l"], p["z"], p["m"], p["Lq"], p["jitter"], likelihood=lik,
                                lik_sigma2=p["sigma2"], neg_var_policy=_ffi.NEGVAR_CLAMP)
    base = _ffi.DeviceModel(ctx, desc, keep)
    desc, keep = _ffi.make_desc(p["np_dt"], family, p["variance"], p["inv_l"], p["z"], p["m"], p["Lq"], p["jitter"], likelihood=lik,
                                lik_sigma2=p["sigma2"], neg_var_policy=_ffi.NEGVAR_CLAMP)
    withm = _ffi.DeviceModel(ctx, desc, keep)
    withm.set_mean_z(0.01 * np.ones(M))
    data = _ffi.DeviceData(ctx, p["x"], p["y"], p["np_dt"])
    tdt = torch.float64 if p["np_dt"] == np.float64 else torch.float32
    mux_h = (0.01 * np.sin(np.arange(n))).astype(p["np_dt"])
    mux_d = torch.tensor(mux_h, device="cuda")
    mub_d = torch.empty(n, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    calls = {"elbo": lambda: base.elbo(data, 0, n, nd),
             "elbo+mean(dev)": lambda: withm.elbo(data, 0, n, nd, prior_mean=mux_d),
             "elbo+mean(host)": lambda: withm.elbo(data, 0, n, nd, prior_mean=mux_h),
             "grad": lambda: base.elbo_grad(data, 0, n, nd),
             "grad+mean(dev)": lambda: withm.elbo_grad(data, 0, n, nd, prior_mean=mux_d, mean_grad=mub_d),
             "grad+mean(host)": lambda: withm.elbo_grad(data, 0, n, nd, prior_mean=mux_h, mean_grad=True)}
    for fn in calls.values():   # warm-up (workspace, staging)
        fn()
    ts = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    for k, v in ts.items():
        ref = float(np.median(ts["elbo" if k.startswith("elbo") else "grad"]))
        med = float(np.median(v))
        print(f"{cfg} n={n} M={M} d={d} {np.dtype(p['np_dt']).name} {k:16s} min {min(v) * 1e3:8.3f} ms  median {med * 1e3:8.3f} ms"
              f"  ratio {med / ref:.4f}", flush=True)
    base.free()
    withm.free()
    data.free()
    del mux_d, mub_d
ctx.close()
