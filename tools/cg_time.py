"""What the exact GP by conjugate gradients costs: svgp_cg_matvec at N = 1e5, d = 8, S = 16 (fp64 and fp32, device memory) and one
svgp_cg_fit at tol 1e-6 with 16 Rademacher probes, beside svgp_sampler_eval at n_features = 0 with the same S and d on the same box in
the same run.  The sampler's kernel is the one kmv_kernel was modelled on (same tile generation, resident panel), so its generated
entries a second are the yardstick; no ratio is fixed in advance: the run reports it.

    python tools/cg_time.py [--reps 7] [--n 100000] [--out profiles/cg/cg_time.jsonl]
    python tools/cg_time.py --precond 256 512 1024 --precond-out profiles/cg/cg_precond_time.jsonl
    python tools/cg_time.py --sample --sample-out profiles/cg/cg_sample_time.jsonl      (sample_leg below)
    python tools/cg_time.py --xgrad --xgrad-out profiles/cg/cg_xgrad_time.jsonl         (xgrad_leg below; after tools/build_prev.sh)
    python tools/cg_time.py --noise --noise-out profiles/cg/cg_noise_time.jsonl         (noise_leg below; after tools/build_prev.sh)

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


def sample_leg(a):
    """--sample: what the pathwise function samples of the exact GP cost at N = --n, d = --d, S = --cols, L = --features, both dtypes,
    median [min, max] of --sample-reps: svgp_cg_sampler_eval over n* = N points (the data themselves) beside svgp_cg_matvec at the same N
    and S (generated kernel entries a second: (N + L) n* and N^2 per device time); eval and eval_grad over n* = 256 points beside
    kmv_kernel over the same points (svgp_cg_predict, mean only; wall time of the blocking calls, upload of the 256 points included in
    both); svgp_cg_sampler_create beside one svgp_cg_solve of the same number of columns at the same tol and --sample-maxiter."""
    import torch

    from approxgp import DeviceConjugateGradients, _ffi, cg_sample_plan
    from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel
    from approxgp.pathwise import draw_basis
    from approxgp.synthetic import synth_arrays

    ctx = _ffi.Context(0)
    N, d, S, L, reps = a.n, a.d, a.cols, a.features, a.sample_reps
    rows = []
    for dt in (np.float64, np.float32):
        tdt = torch.float64 if dt == np.float64 else torch.float32
        p = synth_arrays(0, N, 64, d, dtype=dt)
        kernel = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.asarray(p["inv_lengthscale"], dtype=np.float64))), p["variance"])
        x = np.asarray(p["x"])[:, :N]
        dev = DeviceConjugateGradients(ctx, x, p["y"][:N], dt)
        desc, keep = dev.desc(kernel, p["sigma2"], tol=1e-6, maxiter=a.sample_maxiter)
        basis = draw_basis(_ffi.KERNEL_SE, N, L, S, np.random.default_rng(0), dt, d=d)
        V = torch.randn((S, N), dtype=tdt, device="cuda")
        out = torch.empty_like(V)
        X = torch.empty_like(V)
        x256 = np.ascontiguousarray(x[:, :256] + 0.01)
        big = torch.empty((S, N), dtype=tdt, device="cuda")
        f256 = torch.empty((S, 256), dtype=tdt, device="cuda")
        g256 = torch.empty((S, d, 256), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        wall = lambda fn: (lambda t0: (fn(), 1e3 * (time.perf_counter() - t0))[1])(time.perf_counter())
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            smp = dev.sampler(desc, basis)   # warm-up of every shape
            dev.fit(desc)
            dev.matvec(desc, V, out=out)
            smp.eval(dev.data, out=big)
            smp.eval(x256, out=f256)
            smp.eval_grad(x256, out=f256, grad_out=g256)
            dev.predict(x256, var=False)
            smp.free()
            cr_wall, so_wall, so_mv, cr_mv, iters = [], [], [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                smp = dev.sampler(desc, basis)
                cr_wall.append(1e3 * (time.perf_counter() - t0))
                cr_mv.append(smp.info.ms_matvec)
                iters.append(smp.info.iterations)
                t0 = time.perf_counter()
                info = dev.solve(desc, V, out=X)[3]
                so_wall.append(1e3 * (time.perf_counter() - t0))
                so_mv.append(info.ms_matvec)
                if _ < reps - 1:
                    smp.free()
        mv, ev, e256, g256t, e256w, g256w, p256w = [], [], [], [], [], [], []
        for _ in range(reps):
            dev.matvec(desc, V, out=out)
            mv.append(ctx.timing().ms_strip)
            smp.eval(dev.data, out=big)
            ev.append(ctx.timing().ms_strip)
            e256w.append(wall(lambda: smp.eval(x256, out=f256)))
            e256.append(ctx.timing().ms_strip)
            g256w.append(wall(lambda: smp.eval_grad(x256, out=f256, grad_out=g256)))
            g256t.append(ctx.timing().ms_strip)
            p256w.append(wall(lambda: dev.predict(x256, var=False)))
        m_mv, m_ev = statistics.median(mv), statistics.median(ev)
        seg_rows, nseg, rnd = cg_sample_plan(N)
        row = {"dtype": np.dtype(dt).name, "N": N, "d": d, "S": S, "L": L, "reps": reps, "plan": {"seg_rows": seg_rows, "segments": nseg, "round": rnd},
               "eval_all": {"n": N, "ms": stat(ev), "generated_per_s": float(f"{(N + L) * N / (1e-3 * m_ev):.4g}") if m_ev > 0 else None},
               "matvec": {"ms": stat(mv), "generated_per_s": float(f"{N * N / (1e-3 * m_mv):.4g}") if m_mv > 0 else None},
               "rate_over_matvec": round(((N + L) * N / m_ev) / (N * N / m_mv), 3) if m_mv > 0 and m_ev > 0 else None,
               "n256": {"ms_eval": stat(e256), "ms_eval_grad": stat(g256t), "ms_eval_wall": stat(e256w), "ms_eval_grad_wall": stat(g256w),
                        "ms_predict_mean_wall": stat(p256w),
                        "predict_over_eval_wall": round(statistics.median(p256w) / statistics.median(e256w), 2),
                        "predict_over_eval_grad_wall": round(statistics.median(p256w) / statistics.median(g256w), 2)},
               "create": {"tol": 1e-6, "maxiter": a.sample_maxiter, "iterations": max(iters), "ms_wall": stat(cr_wall), "ms_matvec": stat(cr_mv),
                          "solve_ms_wall": stat(so_wall), "solve_ms_matvec": stat(so_mv),
                          "create_over_solve_wall": round(statistics.median(cr_wall) / statistics.median(so_wall), 3)},
               "finite": bool(torch.isfinite(big).all().item() and torch.isfinite(g256).all().item())}
        print(json.dumps(row), flush=True)
        rows.append(row)
        smp.free()
        dev.free()
        del V, out, X, big, f256, g256
    ctx.close()
    if a.sample_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.sample_out)), exist_ok=True)
        with open(a.sample_out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def xgrad_child(a):
    """one leg of --xgrad in a process of its own (the library is chosen by SVGP_MI355X_LIB before the import): per dtype, after a warm-up,
    the wall time of one blocking gradient call at N = --n, d = --d, 16 Rademacher probes, tol 1e-6 and --xgrad-maxiter iterations.
    leg `new`: svgp_cg_lml_grad_inputs into device memory, the device time of its data-sized kernels alone (svgp_last_timing) and, with
    --xgrad-kernel, svgp_cg_sampler_eval_grad (16 samples, no features) over the same N points in the same run.  leg `prev`: svgp_cg_lml_grad
    of a library that lacks the new symbol.  Both print the outputs of svgp_cg_lml_grad in hex, for the bitwise comparison."""
    import torch

    from approxgp import _ffi
    if a.xgrad_child == "prev":
        _ffi.SYMBOLS.pop("svgp_cg_lml_grad_inputs", None)
    from approxgp import DeviceConjugateGradients, draw_probes
    from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel
    from approxgp.pathwise import draw_basis
    from approxgp.synthetic import synth_arrays

    ctx = _ffi.Context(0)
    N, d, T = a.n, a.d, 16
    for dt in (np.float64, np.float32):
        tdt = torch.float64 if dt == np.float64 else torch.float32
        p = synth_arrays(0, N, 64, d, dtype=dt)
        kernel = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.asarray(p["inv_lengthscale"], dtype=np.float64))), p["variance"])
        x = np.asarray(p["x"])[:, :N]
        dev = DeviceConjugateGradients(ctx, x, p["y"][:N], dt)
        desc, keep = dev.desc(kernel, p["sigma2"], tol=1e-6, maxiter=a.xgrad_maxiter)
        z = draw_probes(N, T, 0)
        new = a.xgrad_child == "new"
        xt = torch.zeros((d, N), dtype=tdt, device="cuda") if new else None
        torch.cuda.synchronize()
        call = (lambda: dev.lml_grad(desc, z, wrt_inputs=True, x_grad_out=xt)) if new else (lambda: dev.lml_grad(desc, z))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lml0, g0, _ = dev.lml_grad(desc, z)   # the existing call (and the warm-up of the solve's shapes)
            call()
            t0 = time.perf_counter()
            lml, g, info = call()
            wall = 1e3 * (time.perf_counter() - t0)
        row = {"leg": a.xgrad_child, "dtype": np.dtype(dt).name, "N": N, "d": d, "T": T, "maxiter": a.xgrad_maxiter, "iterations": info.iterations,
               "ms_wall": round(wall, 2), "lml_grad_hex": [float(v).hex() for v in (lml0, g0["variance"], g0["diag"], g0["mean_const"], *g0["inv_lengthscale"])]}
        if new:
            row["ms_xgrad_kernels"] = round(ctx.timing().ms_strip, 3)
            row["same_as_lml_grad"] = bool(lml == lml0 and all(g[k] == g0[k] for k in ("variance", "diag", "mean_const"))
                                           and np.array_equal(g["inv_lengthscale"], g0["inv_lengthscale"]))
            row["finite"] = bool(torch.isfinite(xt).all().item())
            if a.xgrad_kernel:
                passes = ((2 * T + 1 + 15) // 16) * ((d + 7) // 8)
                basis = draw_basis(_ffi.KERNEL_SE, N, 0, 16, np.random.default_rng(0), dt, d=d)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    smp = dev.sampler(desc, basis)
                G = torch.empty((16, d, N), dtype=tdt, device="cuda")
                torch.cuda.synchronize()
                smp.eval_grad(dev.data, values=False, grad_out=G)
                xs, eg = [], []
                for _ in range(3):
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        call()
                    xs.append(ctx.timing().ms_strip)
                    smp.eval_grad(dev.data, values=False, grad_out=G)
                    eg.append(ctx.timing().ms_strip)
                mx, me = statistics.median(xs), statistics.median(eg)
                row["kernel"] = {"passes": passes, "ms_xgrad": stat(xs), "ms_eval_grad_16x8": stat(eg),
                                 "ns_per_generated_entry": {"xgrad": float(f"{1e6 * mx / (passes * N * N):.4g}"), "eval_grad": float(f"{1e6 * me / (N * N):.4g}")},
                                 "xgrad_over_eval_grad_per_entry": round((mx / passes) / me, 3)}
                smp.free()
                del G
        print("XGRAD " + json.dumps(row), flush=True)
        dev.free()
    ctx.close()


def xgrad_leg(a):
    """--xgrad: what the input gradient of the exact GP costs.  svgp_cg_lml_grad_inputs of this tree against svgp_cg_lml_grad of the
    library --prev-lib (tools/build_prev.sh builds the parent commit's), one process per call, interleaved new / prev, median of
    --xgrad-reps wall times; the new kernel family alone against svgp_cg_sampler_eval_grad's gradient form per generated kernel entry;
    and whether svgp_cg_lml_grad's outputs are bitwise the parent's."""
    import subprocess

    if not os.path.exists(a.prev_lib):
        raise SystemExit(f"{a.prev_lib} is missing: tools/build_prev.sh builds the parent commit's library")
    runs = {"new": [], "prev": []}
    for rep in range(a.xgrad_reps):
        for leg in ("new", "prev"):
            env = dict(os.environ)
            if leg == "prev":
                env["SVGP_MI355X_LIB"] = os.path.abspath(a.prev_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--xgrad-child", leg, "--n", str(a.n), "--d", str(a.d), "--xgrad-maxiter", str(a.xgrad_maxiter)]
            if leg == "new" and rep == 0:
                cmd.append("--xgrad-kernel")
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"the {leg} leg failed with status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[leg].append([json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("XGRAD ")])
    rows = []
    for i, name in enumerate(("float64", "float32")):
        new, prev = [r[i] for r in runs["new"]], [r[i] for r in runs["prev"]]
        mn, mp = statistics.median(r["ms_wall"] for r in new), statistics.median(r["ms_wall"] for r in prev)
        row = {"dtype": name, "N": a.n, "d": a.d, "T": 16, "tol": 1e-6, "maxiter": a.xgrad_maxiter, "iterations": new[0]["iterations"], "reps": a.xgrad_reps,
               "ms_lml_grad_inputs_wall": stat([r["ms_wall"] for r in new]), "ms_parent_lml_grad_wall": stat([r["ms_wall"] for r in prev]),
               "inputs_over_parent": round(mn / mp, 3), "ms_xgrad_kernels": stat([r["ms_xgrad_kernels"] for r in new]), "kernel": new[0].get("kernel"),
               "other_outputs_bitwise_lml_grad": all(r["same_as_lml_grad"] for r in new),
               "lml_grad_bitwise_parent": all(r["lml_grad_hex"] == prev[0]["lml_grad_hex"] for r in new + prev), "finite": all(r["finite"] for r in new)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.xgrad_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.xgrad_out)), exist_ok=True)
        with open(a.xgrad_out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def noise_child(a):
    """one leg of --noise in a process of its own (the library is chosen by SVGP_MI355X_LIB before the import): per dtype at N = --n, d = --d,
    S = --cols, after a warm-up of every shape: the device time of svgp_cg_matvec (median of 5) and the wall time of one blocking
    svgp_cg_lml_grad (16 Rademacher probes, tol 1e-6, --noise-maxiter iterations) WITHOUT a noise vector - the calls the parent has too,
    their outputs in hex for the bitwise comparison.  leg `new` adds: the same two WITH a vector (s = exp(U[log 0.02, log 0.5]),
    default_rng(11)), svgp_cg_lml_grad_noise with it, and one svgp_cg_precond_apply at k = --noise-k with and without it."""
    import warnings

    import torch

    from approxgp import DeviceConjugateGradients, _ffi, draw_probes
    from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel
    from approxgp.synthetic import synth_arrays

    new = a.noise_child == "new"
    if not new:   # the parent's library lacks the new symbols
        _ffi.SYMBOLS.pop("svgp_cg_set_noise", None)
        _ffi.SYMBOLS.pop("svgp_cg_lml_grad_noise", None)
    ctx = _ffi.Context(0)
    N, d, S, T = a.n, a.d, a.cols, 16
    wall = lambda fn: (lambda t0: (fn(), 1e3 * (time.perf_counter() - t0))[1])(time.perf_counter())
    for dt in (np.float64, np.float32):
        tdt = torch.float64 if dt == np.float64 else torch.float32
        p = synth_arrays(0, N, 64, d, dtype=dt)
        kernel = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.asarray(p["inv_lengthscale"], dtype=np.float64))), p["variance"])
        x = np.asarray(p["x"])[:, :N]
        dev = DeviceConjugateGradients(ctx, x, p["y"][:N], dt)
        desc, keep = dev.desc(kernel, p["sigma2"], tol=1e-6, maxiter=a.noise_maxiter)
        z = draw_probes(N, T, 0)
        V = torch.randn((S, N), dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        out = torch.empty_like(V)
        torch.cuda.synchronize()

        def matvec_ms():
            dev.matvec(desc, V, out=out)
            ts = []
            for _ in range(5):
                dev.matvec(desc, V, out=out)
                ts.append(ctx.timing().ms_strip)
            return round(statistics.median(ts), 3)

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            row = {"leg": a.noise_child, "dtype": np.dtype(dt).name, "N": N, "d": d, "S": S, "T": T, "maxiter": a.noise_maxiter}
            row["ms_matvec"] = matvec_ms()
            row["matvec_hex"] = [float(v).hex() for v in out[0, :4].cpu().numpy()]
            lml0, g0, info = dev.lml_grad(desc, z)
            row["ms_lml_grad_wall"] = round(wall(lambda: dev.lml_grad(desc, z)), 2)
            row["iterations"] = info.iterations
            row["lml_grad_hex"] = [float(v).hex() for v in (lml0, g0["variance"], g0["diag"], g0["mean_const"], *g0["inv_lengthscale"])]
            if new:
                s = np.exp(np.random.default_rng(11).uniform(np.log(0.02), np.log(0.5), size=N)).astype(dt)
                sb = torch.zeros(N, dtype=tdt, device="cuda")
                torch.cuda.synchronize()
                dev.lml_grad(desc, z, wrt_noise=True, noise_grad_out=sb)
                row["ms_lml_grad_noise_wall_no_vector"] = round(wall(lambda: dev.lml_grad(desc, z, wrt_noise=True, noise_grad_out=sb)), 2)
                k = a.noise_k
                dev.set_preconditioner(x[:, np.random.default_rng([0, 2]).choice(N, size=k, replace=False)], 1e-4)
                pout = torch.empty_like(V)

                def apply_ms():
                    dev.precond_apply(desc, V, out=pout)
                    ts, st = [], []
                    for _ in range(5):
                        dev.precond_apply(desc, V, out=pout)
                        ts.append(ctx.timing().ms_strip)
                        st.append(ctx.timing().ms_prep)
                    return round(statistics.median(ts), 3), round(statistics.median(st), 3)

                row["ms_precond_apply"], row["ms_precond_setup"] = apply_ms()
                dev.set_noise(s)
                row["ms_precond_apply_vector"], row["ms_precond_setup_vector"] = apply_ms()
                dev.set_preconditioner(None)
                row["ms_matvec_vector"] = matvec_ms()
                dev.lml_grad(desc, z)
                row["ms_lml_grad_wall_vector"] = round(wall(lambda: dev.lml_grad(desc, z)), 2)
                dev.lml_grad(desc, z, wrt_noise=True, noise_grad_out=sb)
                row["ms_lml_grad_noise_wall_vector"] = round(wall(lambda: dev.lml_grad(desc, z, wrt_noise=True, noise_grad_out=sb)), 2)
                row["finite"] = bool(torch.isfinite(sb).all().item() and torch.isfinite(pout).all().item())
                del pout, sb
        print("NOISE " + json.dumps(row), flush=True)
        dev.free()
        del V, out
    ctx.close()


def noise_leg(a):
    """--noise: what per-point noise variances cost.  This tree against the library --prev-lib (tools/build_prev.sh builds the parent
    commit's), one process per leg, interleaved new / prev, medians of --noise-reps: svgp_cg_matvec and a --noise-maxiter-iteration
    svgp_cg_lml_grad without a vector on both, whether their outputs are bitwise the parent's, and on this tree the same calls with a
    vector, svgp_cg_lml_grad_noise and one preconditioner application at k = --noise-k.  `spread` is (max - min) / median of the
    parent's own repeats: a difference between the legs below it is not resolved by this run."""
    import subprocess

    if not os.path.exists(a.prev_lib):
        raise SystemExit(f"{a.prev_lib} is missing: tools/build_prev.sh builds the parent commit's library")
    runs = {"new": [], "prev": []}
    for rep_ in range(a.noise_reps):
        for leg in ("new", "prev"):
            env = dict(os.environ)
            if leg == "prev":
                env["SVGP_MI355X_LIB"] = os.path.abspath(a.prev_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--noise-child", leg, "--n", str(a.n), "--d", str(a.d), "--cols", str(a.cols),
                   "--noise-maxiter", str(a.noise_maxiter), "--noise-k", str(a.noise_k)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"the {leg} leg failed with status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[leg].append([json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("NOISE ")])
    rows = []
    med = lambda rs, k: stat([r[k] for r in rs])
    spread = lambda v: round((v[2] - v[1]) / v[0], 4) if v[0] > 0 else None
    for i, name in enumerate(("float64", "float32")):
        new, prev = [r[i] for r in runs["new"]], [r[i] for r in runs["prev"]]
        mvn, mvp, lgn, lgp = med(new, "ms_matvec"), med(prev, "ms_matvec"), med(new, "ms_lml_grad_wall"), med(prev, "ms_lml_grad_wall")
        row = {"dtype": name, "N": a.n, "d": a.d, "S": a.cols, "T": 16, "maxiter": a.noise_maxiter, "iterations": new[0]["iterations"], "reps": a.noise_reps,
               "matvec": {"ms_parent": mvp, "ms_no_vector": mvn, "ms_vector": med(new, "ms_matvec_vector"), "no_vector_over_parent": round(mvn[0] / mvp[0], 4),
                          "vector_over_parent": round(med(new, "ms_matvec_vector")[0] / mvp[0], 4), "spread_parent": spread(mvp), "spread_new": spread(mvn)},
               "lml_grad": {"ms_parent_wall": lgp, "ms_no_vector_wall": lgn, "ms_vector_wall": med(new, "ms_lml_grad_wall_vector"),
                            "no_vector_over_parent": round(lgn[0] / lgp[0], 4), "vector_over_parent": round(med(new, "ms_lml_grad_wall_vector")[0] / lgp[0], 4),
                            "spread_parent": spread(lgp), "spread_new": spread(lgn)},
               "lml_grad_noise": {"ms_no_vector_wall": med(new, "ms_lml_grad_noise_wall_no_vector"), "ms_vector_wall": med(new, "ms_lml_grad_noise_wall_vector"),
                                  "over_lml_grad_no_vector": round(med(new, "ms_lml_grad_noise_wall_no_vector")[0] / lgn[0], 4),
                                  "over_lml_grad_vector": round(med(new, "ms_lml_grad_noise_wall_vector")[0] / med(new, "ms_lml_grad_wall_vector")[0], 4)},
               "precond_apply": {"k": a.noise_k, "ms_no_vector": med(new, "ms_precond_apply"), "ms_vector": med(new, "ms_precond_apply_vector"),
                                 "ms_setup_no_vector": med(new, "ms_precond_setup"), "ms_setup_vector": med(new, "ms_precond_setup_vector")},
               "bitwise_parent": all(r["lml_grad_hex"] == prev[0]["lml_grad_hex"] and r["matvec_hex"] == prev[0]["matvec_hex"] for r in new + prev),
               "finite": all(r["finite"] for r in new)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.noise_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.noise_out)), exist_ok=True)
        with open(a.noise_out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", action="store_true", help="the per-point-noise leg alone (svgp_cg_set_noise, svgp_cg_lml_grad_noise)")
    ap.add_argument("--noise-child", choices=("new", "prev"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--noise-reps", type=int, default=3)
    ap.add_argument("--noise-maxiter", type=int, default=20)
    ap.add_argument("--noise-k", type=int, default=256)
    ap.add_argument("--noise-out", default=None, help="e.g. profiles/cg/cg_noise_time.jsonl")
    ap.add_argument("--xgrad", action="store_true", help="the input gradient's leg alone (svgp_cg_lml_grad_inputs)")
    ap.add_argument("--xgrad-child", choices=("new", "prev"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--xgrad-kernel", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--xgrad-reps", type=int, default=3)
    ap.add_argument("--xgrad-maxiter", type=int, default=20)
    ap.add_argument("--xgrad-out", default=None, help="e.g. profiles/cg/cg_xgrad_time.jsonl")
    ap.add_argument("--prev-lib", default=os.path.join(ROOT, "approximategps.jl_amd", "csrc", "ablate", "libsvgp_prev.so"))
    ap.add_argument("--sample", action="store_true", help="the pathwise sampler's leg alone (svgp_cg_sampler_*)")
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--sample-reps", type=int, default=3)
    ap.add_argument("--sample-maxiter", type=int, default=30)
    ap.add_argument("--sample-out", default=None, help="e.g. profiles/cg/cg_sample_time.jsonl")
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
    if a.noise_child:
        return noise_child(a)
    if a.noise:
        return noise_leg(a)
    if a.xgrad_child:
        return xgrad_child(a)
    if a.xgrad:
        return xgrad_leg(a)
    if a.sample:
        return sample_leg(a)
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
