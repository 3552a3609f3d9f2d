"""What a natural-gradient step costs beyond the value-and-gradient it contains: svgp_natgrad_step (with grads_out) of this tree against
svgp_elbo_grad of the PARENT commit (tools/build_prev.sh -> csrc/ablate/libsvgp_prev.so), one process per library, the two interleaved
on the same box as tools/lib_ab.sh does.  Shapes: H (N = 1e6, M = 1024, d = 8, fp64), C5w (a 2^18-point window, M = 1024, d = 4, fp32),
MB (a 16 384-point minibatch, M = 1024, d = 8, fp64).  Wall times by the host clock around calls that block until their results are on
the host, behind a model update each, after a warm-up; the median of --reps repeats with min and max.

    python tools/natgrad_time.py [--rounds 2] [--reps 5] [--out profiles/natgrad/natgrad_time.jsonl]
    python tools/natgrad_time.py --worker this|prev [--shapes H C5w MB]      (one library: what the driver starts)

Per shape the driver reports: elbo_grad of this tree and of the parent (the same call: its time must stay inside the run-to-run spread,
its outputs - hashed - must be bitwise equal), natgrad_step at gamma = 0.5 and at gamma = 1 (no Lambda), the extra time of the M-sized
tail in ms and as a ratio, and for MB the host-side training step: update_keep_q + natgrad_step against model_update + elbo_grad."""
import argparse
import hashlib
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

PREV = os.path.join(ROOT, "approximategps.jl_amd", "csrc", "ablate", "libsvgp_prev.so")
SHAPES = {"H": (0, 1_000_000, 1024, 8, np.float64), "C5w": (5, 1 << 18, 1024, 4, np.float32), "MB": (2, 16_384, 1024, 8, np.float64)}
NEW_SYMBOLS = ("svgp_natgrad_step", "svgp_natgrad_step_ext", "svgp_model_update_keep_q")


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [round(1e3 * statistics.median(ts), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)]


def worker(role, shapes, reps):
    import torch  # noqa: F401  (its HIP runtime first)

    from approxgp import _ffi
    from approxgp.synthetic import synth_arrays

    if role == "prev":
        for s in NEW_SYMBOLS:
            _ffi.SYMBOLS.pop(s, None)
    ctx = _ffi.Context(0)
    for name in shapes:
        cid, n, M, d, dt = SHAPES[name]
        p = synth_arrays(cid, n, M, d, dtype=dt)
        mk = lambda: _ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"], p["jitter"],
                                    lik_sigma2=p["sigma2"])
        model = _ffi.DeviceModel(ctx, *mk())
        data = _ffi.DeviceData(ctx, p["x"], p["y"], dt)
        gout = model.elbo_grad(data, 0, n, float(n))[2]    # warm-up; its arrays are reused (no fresh M^2 pages per step)

        def upd(fn):
            def run():
                model.update(*mk())
                fn()
            return run

        row = {"shape": name, "lib": role, "n": n, "M": M, "d": d, "dtype": np.dtype(dt).name, "reps": reps}
        row["elbo_grad_ms"] = timed(upd(lambda: model.elbo_grad(data, 0, n, float(n), out=gout)), reps)
        model.update(*mk())
        v, t, g = model.elbo_grad(data, 0, n, float(n))
        h = hashlib.sha256(np.float64(v).tobytes())
        for f, _ in _ffi.Terms._fields_:
            h.update(np.float64(getattr(t, f)).tobytes())
        for k in ("variance", "lik_sigma2", "mean_const"):
            h.update(np.float64(g[k]).tobytes())
        for k in ("inv_lengthscale", "z", "m", "Lq"):
            h.update(np.ascontiguousarray(g[k]).tobytes())
        row["elbo_grad_outputs_sha16"] = h.hexdigest()[:16]
        if role == "this":
            for key, gamma in (("natgrad_step_ms", 0.5), ("natgrad_step_gamma1_ms", 1.0)):
                fn = upd(lambda: model.natgrad_step(data, 0, n, float(n), gamma=gamma, want_grads=True, fetch=False))
                fn()
                row[key] = timed(fn, reps)
            if name == "MB":   # the host-side training step: hyperparameters up, value and gradient (+ the step on q) back
                def keep_q_step():
                    model.update_keep_q(*mk())
                    model.natgrad_step(data, 0, n, float(n), gamma=0.5, want_grads=True, fetch=False)
                keep_q_step()
                row["step_update_keep_q_natgrad_ms"] = timed(keep_q_step, reps)
                row["step_model_update_elbo_grad_ms"] = row["elbo_grad_ms"]
                row["update_ms"] = timed(lambda: model.update(*mk()), reps)
                row["update_keep_q_ms"] = timed(lambda: model.update_keep_q(*mk()), reps)
        print(json.dumps(row), flush=True)
        model.free()
        data.free()
    ctx.close()


def driver(a):
    if not os.path.exists(PREV):
        sys.exit(f"{PREV} is missing: build the parent commit's library with tools/build_prev.sh")
    rows = []
    for r in range(a.rounds):
        for role in ("this", "prev"):
            env = dict(os.environ)
            if role == "prev":
                env["SVGP_MI355X_LIB"] = PREV
            else:
                env.pop("SVGP_MI355X_LIB", None)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", role, "--reps", str(a.reps), "--shapes", *a.shapes],
                                 env=env, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                sys.exit(f"worker {role} failed ({res.returncode}):\n{res.stderr[-2000:]}")
            print(f"# round {r} {role}: done", file=sys.stderr, flush=True)
            for line in res.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), round=r))
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")
    for name in a.shapes:
        mine = [x for x in rows if x["shape"] == name and x["lib"] == "this"]
        prev = [x for x in rows if x["shape"] == name and x["lib"] == "prev"]
        med = lambda xs, k: round(statistics.median(x[k][0] for x in xs), 3)
        row = {k: mine[0][k] for k in ("shape", "n", "M", "d", "dtype", "reps")}
        row["rounds"] = a.rounds
        row["elbo_grad_ms_this_rounds"] = [x["elbo_grad_ms"][0] for x in mine]
        row["elbo_grad_ms_parent_rounds"] = [x["elbo_grad_ms"][0] for x in prev]
        row["elbo_grad_ms_this"], row["elbo_grad_ms_parent"] = med(mine, "elbo_grad_ms"), med(prev, "elbo_grad_ms")
        row["elbo_grad_outputs_bitwise_equal_to_parent"] = len({x["elbo_grad_outputs_sha16"] for x in mine + prev}) == 1
        row["natgrad_step_ms"], row["natgrad_step_gamma1_ms"] = med(mine, "natgrad_step_ms"), med(mine, "natgrad_step_gamma1_ms")
        row["tail_ms"] = round(row["natgrad_step_ms"] - row["elbo_grad_ms_parent"], 3)
        row["tail_gamma1_ms"] = round(row["natgrad_step_gamma1_ms"] - row["elbo_grad_ms_parent"], 3)
        row["natgrad_over_parent_elbo_grad"] = round(row["natgrad_step_ms"] / row["elbo_grad_ms_parent"], 4)
        if name == "MB":
            for k in ("step_update_keep_q_natgrad_ms", "step_model_update_elbo_grad_ms", "update_ms", "update_keep_q_ms"):
                row[k] = med(mine, k)
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["this", "prev"], default=None)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.shapes, a.reps)
    else:
        driver(a)


if __name__ == "__main__":
    main()
