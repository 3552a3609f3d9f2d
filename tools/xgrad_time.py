"""Cost of d elbo / d x: svgp_elbo_grad against svgp_elbo_grad_inputs (device output, and host output) on one context,
interleaved A / B / C per repetition; min and median wall time of each.
usage: tools/xgrad_time.py [bench.py config names, default H Hd64 C5] [--reps R]"""
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
ap.add_argument("configs", nargs="*", default=["H", "Hd64", "C5"])
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()

ctx = _ffi.Context(0)
for cfg in args.configs:
    n, M, d, family, lik, dtype, cid = bench.CONFIGS[cfg]
    nd = bench.C5_NUM_DATA if cfg == "C5" else float(n)
    p = bench.synth(cid, n, M, d, family, lik, dtype)
    desc, keep = _ffi.make_desc(p["np_dt"], family, p["variance"], p["inv_l"], p["z"], p["m"], p["Lq"], p["jitter"], likelihood=lik,
                                lik_sigma2=p["sigma2"], neg_var_policy=_ffi.NEGVAR_CLAMP)
    model = _ffi.DeviceModel(ctx, desc, keep)
    data = _ffi.DeviceData(ctx, p["x"], p["y"], p["np_dt"])
    gx = torch.empty((d, n), dtype=torch.float64 if p["np_dt"] == np.float64 else torch.float32, device="cuda")
    torch.cuda.synchronize()
    calls = {"grad": lambda: model.elbo_grad(data, 0, n, nd),
             "grad+x(device)": lambda: model.elbo_grad(data, 0, n, nd, inputs=(gx.data_ptr(), n)),
             "grad+x(host)": lambda: model.elbo_grad(data, 0, n, nd, inputs=True)}
    for fn in calls.values():   # warm-up (workspace, staging)
        fn()
    ts = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    base = float(np.median(ts["grad"]))
    for k, v in ts.items():
        med = float(np.median(v))
        print(f"{cfg} n={n} M={M} d={d} {np.dtype(p['np_dt']).name} {k:16s} min {min(v) * 1e3:8.3f} ms  median {med * 1e3:8.3f} ms"
              f"  ratio {med / base:.4f}", flush=True)
    model.free()
    data.free()
    del gx
ctx.close()
