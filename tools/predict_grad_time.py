"""What the predictive gradients cost: svgp_predictor_eval (mean, variance and both gradients, device output) at n* = 1e6 and 4096,
d = 8, M = 1024, fp64 and fp32, against (a) the 2 d + 1 calls of svgp_marginals a caller paid before for a central-difference gradient -
with --parent-lib from a library built from the parent commit, otherwise this tree's, whose svgp_marginals is compiled from the same
text - and (b) svgp_sampler_eval_grad at S = 16, L = 0 in the same run, per generated kernel entry.  No ratio is fixed in advance.

    python tools/predict_grad_time.py [--rounds 3] [--parent-lib PATH] [--out profiles/predict_grad/predict_grad_time.jsonl]

Times: the wall time by the host clock around the blocking calls after a warm-up of every shape, the legs interleaved inside each
round; median [min, max] of --rounds rounds.  The parent library is loaded in a child process of its own."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def stat(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def marginals_leg(a):
    """The child: 2 d + 1 svgp_marginals calls per round with the library of SVGP_MI355X_LIB, one JSON line."""
    from approxgp import _ffi
    from approxgp.synthetic import synth_arrays

    ctx = _ffi.Context(0)
    res = {}
    for dt in (np.float64, np.float32):
        for n in a.n:
            p = synth_arrays(0, n, a.M, a.d, dtype=dt)
            model = _ffi.DeviceModel(ctx, *_ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"],
                                                          p["jitter"], lik_sigma2=p["sigma2"]))
            data = _ffi.DeviceData(ctx, p["x"], None, dt)
            model.marginals(data)
            res[f"{np.dtype(dt).name}_{n}"] = [wall(lambda: [model.marginals(data) for _ in range(2 * a.d + 1)]) for _ in range(a.rounds)]
            model.free()
            data.free()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 4096])
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--marginals-leg", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.marginals_leg:
        return marginals_leg(a)
    import torch

    from approxgp import _ffi
    from approxgp.pathwise import draw_basis
    from approxgp.synthetic import synth_arrays

    parent = None
    if a.parent_lib:
        env = dict(os.environ, SVGP_MI355X_LIB=os.path.abspath(a.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--marginals-leg", "--rounds", str(a.rounds), "--M", str(a.M), "--d", str(a.d), "--n", *map(str, a.n)]
        parent = json.loads(subprocess.run(cmd, env=env, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])
    ctx = _ffi.Context(0)
    rows = []
    for dt in (np.float64, np.float32):
        tdt = torch.float64 if dt == np.float64 else torch.float32
        for n in a.n:
            p = synth_arrays(0, n, a.M, a.d, dtype=dt)
            model = _ffi.DeviceModel(ctx, *_ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"],
                                                          p["jitter"], lik_sigma2=p["sigma2"]))
            data = _ffi.DeviceData(ctx, p["x"], None, dt)
            t0 = time.perf_counter()
            pred = model.predictor()
            create_ms = (time.perf_counter() - t0) * 1e3
            smp = model.sampler(draw_basis(_ffi.KERNEL_SE, a.M, 0, a.samples, np.random.default_rng(0), dt, d=a.d))
            outs = [torch.empty(s, dtype=tdt, device="cuda") for s in ((n,), (n,), (a.d, n), (a.d, n))]
            gout = torch.empty((a.samples, a.d, n), dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            legs = {"predictor_eval": lambda: pred.eval(data, out=outs),
                    "marginals_2d+1": lambda: [model.marginals(data) for _ in range(2 * a.d + 1)],
                    "sampler_eval_grad": lambda: smp.eval_grad(data, values=False, grad_out=gout)}
            for fn in legs.values():
                fn()
            ts = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    ts[k].append(wall(fn))
            row = {"dtype": np.dtype(dt).name, "n": n, "M": a.M, "d": a.d, "create_ms": round(create_ms, 2)}
            row.update({k + "_ms": stat(v) for k, v in ts.items()})
            if parent:
                row["parent_marginals_2d+1_ms"] = stat(parent[f"{np.dtype(dt).name}_{n}"])
            base = row.get("parent_marginals_2d+1_ms", row["marginals_2d+1_ms"])[0]
            row["ratio_to_marginals"] = round(row["predictor_eval_ms"][0] / base, 4)
            # generated kernel entries: the predictor regenerates each tile per row block of G; per Mp x n* entry of the contraction
            row["ps_per_entry_predictor"] = round(row["predictor_eval_ms"][0] * 1e9 / (a.M * n), 3)
            row["ps_per_entry_sampler_grad"] = round(row["sampler_eval_grad_ms"][0] * 1e9 / (a.M * n), 3)
            rows.append(row)
            print(json.dumps(row))
            for h in (pred, smp, model, data):
                h.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
