"""What pathwise function samples cost: svgp_sampler_create at M = 1024, L = 2048, S = 16 and svgp_sampler_eval at H's shape
(n* = 1e6 points, d = 8; fp64 and fp32, device output), against svgp_kuf over the same window on the same box in the same run.
svgp_kuf generates the same M x n* kernel tiles and WRITES them; the sampler's kernel generates them plus L x n* cosines and multiplies
where svgp_kuf writes.  No ratio is fixed in advance: the run reports it.

    python tools/sample_time.py [--reps 7] [--n 1000000] [--out profiles/sample/sample_time.jsonl]
    python tools/sample_time.py --grad [--reps 7] [--out profiles/sample/sample_grad_time.jsonl]

--grad: svgp_sampler_eval_grad (values and gradient; gradient only) at the same shape, with L features and with L = 0, against the
unchanged svgp_sampler_eval in the same run, alternating inside the timed loop.  The yardstick is what a caller paid before the call
existed: 2 d central-difference calls of svgp_sampler_eval per gradient; the run reports the ratio to that and to one svgp_sampler_eval.

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


def grad_main(a):
    import torch

    from approxgp import _ffi
    from approxgp.pathwise import draw_basis
    from approxgp.synthetic import synth_arrays

    ctx = _ffi.Context(0)
    rows = []
    n, M, d, S = a.n, a.M, a.d, a.samples
    for dt in (np.float64, np.float32):
        tdt = torch.float64 if dt == np.float64 else torch.float32
        p = synth_arrays(0, n, M, d, dtype=dt)
        model = _ffi.DeviceModel(ctx, *_ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"],
                                                      p["jitter"], lik_sigma2=p["sigma2"]))
        data = _ffi.DeviceData(ctx, p["x"], None, dt)
        out = torch.empty((S, n), dtype=tdt, device="cuda")
        ref = torch.empty((S, n), dtype=tdt, device="cuda")
        gout = torch.empty((S, d, n), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        for L in (a.features, 0):
            smp = model.sampler(draw_basis(_ffi.KERNEL_SE, M, L, S, np.random.default_rng(0), dt, d=d))
            smp.eval(data, out=ref)           # warm-up of every call the timed loop makes
            smp.eval_grad(data, out=out, grad_out=gout)
            smp.eval_grad(data, values=False, grad_out=gout)
            both, only, ev = [], [], []
            for _ in range(a.reps):
                smp.eval_grad(data, out=out, grad_out=gout)
                both.append(ctx.timing().ms_strip)
                smp.eval(data, out=ref)
                ev.append(ctx.timing().ms_strip)
                smp.eval_grad(data, values=False, grad_out=gout)
                only.append(ctx.timing().ms_strip)
            chk = gout[:, :, :: max(n // 1000, 1)].double().cpu().numpy()
            mb, mo, me = (statistics.median(t) for t in (both, only, ev))
            row = {"dtype": np.dtype(dt).name, "n": n, "M": M, "d": d, "L": L, "S": S, "reps": a.reps,
                   "ms_eval_grad": stat(both), "ms_grad_only": stat(only), "ms_eval": stat(ev),
                   "ms_finite_differences": round(2 * d * me, 3),   # 2 d calls of svgp_sampler_eval: what a caller paid before
                   "eval_grad_over_eval": round(mb / me, 3), "grad_only_over_eval": round(mo / me, 3),
                   "eval_grad_over_finite_differences": round(mb / (2 * d * me), 4),
                   "grad_only_over_finite_differences": round(mo / (2 * d * me), 4),
                   "values_bitwise_eval": bool(torch.equal(out, ref)), "finite": bool(np.all(np.isfinite(chk))),
                   "grad_abs_max": float(np.abs(chk).max())}
            print(json.dumps(row), flush=True)
            rows.append(row)
            smp.free()
        model.free()
        data.free()
        del out, ref, gout
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grad", action="store_true", help="time svgp_sampler_eval_grad against svgp_sampler_eval")
    a = ap.parse_args()
    if a.grad:
        return grad_main(a)
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
