"""What the exact GP by conjugate gradients costs: svgp_cg_matvec at N = 1e5, d = 8, S = 16 (fp64 and fp32, device memory) and one
svgp_cg_fit at tol 1e-6 with 16 Rademacher probes, beside svgp_sampler_eval at n_features = 0 with the same S and d on the same box in
the same run.  The sampler's kernel is the one kmv_kernel was modelled on (same tile generation, resident panel), so its generated
entries a second are the yardstick; no ratio is fixed in advance: the run reports it.

    python tools/cg_time.py [--reps 7] [--n 100000] [--out profiles/cg/cg_time.jsonl]
    python tools/cg_time.py --precond 256 512 1024 --precond-out profiles/cg/cg_precond_time.jsonl

--precond K ...: after the unpreconditioned fit, the same fit (17 columns, same tol and maxiter) with the Nystrom preconditioner of K
data points (default_rng([0, 2]).choice, jitter 1e-4): iterations, final residual, wall time, the preconditioner's setup time and
the device time of one svgp_cg_precond_apply (16 columns) beside one matvec of the same run.

Times: the device time of the call's kernels from the library's own events (svgp_last_timing's ms_strip for matvec and the sampler,
svgp_cg_info's ms_matvec / ms_vector summed over the iterations of the fit) and the wall time by the host clock around the blocking
call, after a warm-up of every shape; matvec and the sampler alternate inside the timed loop; median [min, max] of --reps repeats.
generated_per_s = N^2 / device time of one matvec (M n* / device time for the sampler)."""
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
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--M", type=int, default=1024, help="inducing points of the sampler the rate is compared with")
    ap.add_argument("--n-sampler", type=int, default=1_000_000)
    ap.add_argument("--maxiter", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--precond", type=int, nargs="*", default=[], help="preconditioner sizes for the preconditioned leg")
    ap.add_argument("--precond-out", default=None)
    a = ap.parse_args()
    import torch

    from approxgp import DeviceConjugateGradients, _ffi, draw_probes
    from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel
    from approxgp.pathwise import draw_basis
    from approxgp.synthetic import synth_arrays

    ctx = _ffi.Context(0)
    rows, prows = [], []
    N, d, S, M, ns = a.n, a.d, a.cols, a.M, a.n_sampler
    for dt in (np.float64, np.float32):
        tdt = torch.float64 if dt == np.float64 else torch.float32
        p = synth_arrays(0, max(N, ns), M, d, dtype=dt)
        kernel = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.asarray(p["inv_lengthscale"], dtype=np.float64))), p["variance"])
        dev = DeviceConjugateGradients(ctx, p["x"][:, :N], p["y"][:N], dt)
        desc, keep = dev.desc(kernel, p["sigma2"], tol=1e-6, maxiter=a.maxiter)
        V = torch.randn((S, N), dtype=tdt, device="cuda")
        out = torch.empty_like(V)
        model = _ffi.DeviceModel(ctx, *_ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"],
                                                      p["jitter"], lik_sigma2=p["sigma2"]))
        data = _ffi.DeviceData(ctx, p["x"][:, :ns], None, dt)
        smp = model.sampler(draw_basis(_ffi.KERNEL_SE, M, 0, S, np.random.default_rng(0), dt, d=d))
        sout = torch.empty((S, ns), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        dev.matvec(desc, V, out=out)   # warm-up of every shape the timed loop uses
        smp.eval(data, out=sout)
        mv_dev, mv_wall, sm_dev = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dev.matvec(desc, V, out=out)
            mv_wall.append(1e3 * (time.perf_counter() - t0))
            mv_dev.append(ctx.timing().ms_strip)
            smp.eval(data, out=sout)
            sm_dev.append(ctx.timing().ms_strip)
        z = draw_probes(N, 16, 0)
        t0 = time.perf_counter()
        lml, info = dev.fit(desc, z)
        fit_wall = 1e3 * (time.perf_counter() - t0)
        mv, sm = statistics.median(mv_dev), statistics.median(sm_dev)
        row = {"dtype": np.dtype(dt).name, "N": N, "d": d, "S": S, "reps": a.reps, "ms_matvec": stat(mv_dev), "ms_matvec_wall": stat(mv_wall),
               "generated_per_s": float(f"{N * N / (1e-3 * mv):.4g}") if mv > 0 else None,
               "sampler": {"M": M, "n": ns, "ms_eval": stat(sm_dev), "generated_per_s": float(f"{M * ns / (1e-3 * sm):.4g}") if sm > 0 else None},
               "rate_over_sampler": round((N * N / mv) / (M * ns / sm), 3) if mv > 0 and sm > 0 else None,
               "fit": {"tol": 1e-6, "probes": 16, "iterations": info.iterations, "converged": info.converged,
                       "max_rel_residual": info.max_rel_residual, "lml": lml, "ms_wall": round(fit_wall, 1),
                       "ms_matvec": round(info.ms_matvec, 1), "ms_vector": round(info.ms_vector, 1)},
               "finite": bool(torch.isfinite(out).all().item())}
        print(json.dumps(row), flush=True)
        rows.append(row)
        for k in a.precond:
            idx = np.random.default_rng([0, 2]).choice(N, size=k, replace=False)
            dev.set_preconditioner(np.asarray(p["x"])[:, idx], 1e-4)
            pout = torch.empty_like(V)
            dev.precond_apply(desc, V, out=pout)   # warm-up
            ap_dev, setup = [], []
            for _ in range(a.reps):
                dev.precond_apply(desc, V, out=pout)
                tm = ctx.timing()
                ap_dev.append(tm.ms_strip)
                setup.append(tm.ms_prep)
            t0 = time.perf_counter()
            try:
                lml_k, info_k = dev.fit(desc, z, probes_k=draw_probes(k, 16, np.random.default_rng([0, 1])))
            except _ffi.PosDefException as e:   # r' P^-1 r of a column not > 0: the applied preconditioner lost positive definiteness
                wall_k = 1e3 * (time.perf_counter() - t0)
                prow = {"dtype": np.dtype(dt).name, "N": N, "d": d, "k": k, "columns": 17, "tol": 1e-6, "maxiter": a.maxiter,
                        "status": "SVGP_NOT_POSDEF", "message": str(e), "ms_wall": round(wall_k, 1), "ms_setup": stat(setup), "ms_apply_16": stat(ap_dev)}
                print(json.dumps(prow), flush=True)
                prows.append(prow)
                dev.set_preconditioner(None)
                del pout
                continue
            wall_k = 1e3 * (time.perf_counter() - t0)
            prow = {"dtype": np.dtype(dt).name, "N": N, "d": d, "k": k, "columns": 17, "tol": 1e-6, "maxiter": a.maxiter,
                    "iterations": info_k.iterations, "converged": info_k.converged, "n_unconverged": info_k.n_unconverged,
                    "max_rel_residual": info_k.max_rel_residual, "lml": lml_k, "ms_wall": round(wall_k, 1),
                    "ms_matvec": round(info_k.ms_matvec, 1), "ms_vector": round(info_k.ms_vector, 1), "ms_setup": stat(setup),
                    "ms_apply_16": stat(ap_dev), "ms_matvec_16": stat(mv_dev),
                    "unpreconditioned": {"iterations": info.iterations, "converged": info.converged,
                                         "max_rel_residual": info.max_rel_residual, "ms_wall": round(fit_wall, 1), "lml": lml}}
            if not info_k.converged:   # the end of the residual curve: the same deterministic iteration stopped earlier
                tail = {}
                for it in (a.maxiter - 100, a.maxiter - 50, a.maxiter - 10):
                    if it < 1:
                        continue
                    dk, keep_k = dev.desc(kernel, p["sigma2"], tol=1e-6, maxiter=it)
                    try:
                        tail[str(it)] = dev.fit(dk, z, probes_k=draw_probes(k, 16, np.random.default_rng([0, 1])))[1].max_rel_residual
                    except _ffi.PosDefException as e:
                        tail[str(it)] = "not positive definite"
                tail[str(a.maxiter)] = info_k.max_rel_residual
                prow["residual_tail"] = tail
            print(json.dumps(prow), flush=True)
            prows.append(prow)
            dev.set_preconditioner(None)
            del pout
        smp.free()
        model.free()
        data.free()
        dev.free()
        del V, out, sout
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if a.precond_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.precond_out)), exist_ok=True)
        with open(a.precond_out, "w") as f:
            for r in prows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
