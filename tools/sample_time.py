"""What pathwise function samples cost: svgp_sampler_create at M = 1024, L = 2048, S = 16 and svgp_sampler_eval at H's shape
(n* = 1e6 points, d = 8; fp64 and fp32, device output), against svgp_kuf over the same window on the same box in the same run.
svgp_kuf generates the same M x n* kernel tiles and WRITES them; the sampler's kernel generates them plus L x n* cosines and multiplies
where svgp_kuf writes.  No ratio is fixed in advance: the run reports it.

    python tools/sample_time.py [--reps 7] [--n 1000000] [--out profiles/sample/sample_time.jsonl]

Times: the device time of the call's kernels from the library's own events (svgp_last_timing: ms_strip of svgp_sampler_eval, ms_kuf of
svgp_kuf) and the wall time by the host clock around the blocking call, after a warm-up of every shape; eval and kuf alternate inside
the timed loop; median [min, max] of --reps repeats.  generated_per_s = (L + M) n* / device time: kernel and feature entries a second."""
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


def stat(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from approxgp import _ffi
    from approxgp.pathwise import draw_basis
    from approxgp.synthetic import synth_arrays

    ctx = _ffi.Context(0)
    rows = []
    n, M, d, L, S = a.n, a.M, a.d, a.features, a.samples
    for dt in (np.float64, np.float32):
        p = synth_arrays(0, n, M, d, dtype=dt)
        model = _ffi.DeviceModel(ctx, *_ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"],
                                                      p["jitter"], lik_sigma2=p["sigma2"]))
        data = _ffi.DeviceData(ctx, p["x"], None, dt)
        basis = draw_basis(_ffi.KERNEL_SE, M, L, S, np.random.default_rng(0), dt, d=d)
        out = torch.empty((S, n), dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        smp = model.sampler(basis)            # warm-up of every shape the timed windows use
        smp.eval(data, out=out)
        model.kuf(data, fetch=False)
        smp.free()
        t_create = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            s = model.sampler(basis)
            t_create.append(1e3 * (time.perf_counter() - t0))
            s.free()
        smp = model.sampler(basis)
        ev_dev, ev_wall, kuf_dev, kuf_wall = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            smp.eval(data, out=out)
            ev_wall.append(1e3 * (time.perf_counter() - t0))
            ev_dev.append(ctx.timing().ms_strip)
            t0 = time.perf_counter()
            model.kuf(data, fetch=False)
            kuf_wall.append(1e3 * (time.perf_counter() - t0))
            kuf_dev.append(ctx.timing().ms_kuf)
        chk = out[:, :: max(n // 1000, 1)].double().cpu().numpy()
        row = {"dtype": np.dtype(dt).name, "n": n, "M": M, "d": d, "L": L, "S": S, "reps": a.reps,
               "ms_create_wall": stat(t_create), "ms_eval": stat(ev_dev), "ms_eval_wall": stat(ev_wall), "ms_kuf": stat(kuf_dev),
               "ms_kuf_wall": stat(kuf_wall), "eval_over_kuf": round(statistics.median(ev_dev) / statistics.median(kuf_dev), 3),
               "generated_per_s": float(f"{(L + M) * n / (1e-3 * statistics.median(ev_dev)):.4g}"),
               "kuf_entries_per_s": float(f"{M * n / (1e-3 * statistics.median(kuf_dev)):.4g}"),
               "finite": bool(np.all(np.isfinite(chk))), "sample_abs_max": float(np.abs(chk).max())}
        print(json.dumps(row), flush=True)
        rows.append(row)
        smp.free()
        model.free()
        data.free()
        del out
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
