"""What the predictive call costs against the forward evaluation it shares its data pass with: svgp_predictive of this tree - summary
only, and with all three per-point outputs - against svgp_elbo of the PARENT commit (tools/build_prev.sh -> csrc/ablate/libsvgp_prev.so),
one process per library, the two interleaved on the same box as tools/natgrad_time.py does.  Shapes: H (N = 1e6, M = 1024, d = 8, fp64)
and C5 (2^18 points, M = 1024, d = 8, fp32).  Wall times by the host clock around calls that block until their results are on the host,
after a warm-up; the median of --reps repeats with min and max.  The strips are shared, so the expectation is a ratio near 1; the
per-point outputs add three device-to-host copies of N doubles.

    python tools/predictive_time.py [--rounds 2] [--reps 7] [--out profiles/predictive/predictive_time.jsonl]
    python tools/predictive_time.py --worker this|prev [--shapes H C5]      (one library: what the driver starts)

Per shape the driver reports svgp_elbo of this tree and of the parent (the same call: its value must be bitwise equal), the two
svgp_predictive forms, and their ratios to the parent's svgp_elbo."""
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

PREV = os.path.join(ROOT, "approximategps.jl_amd", "csrc", "ablate", "libsvgp_prev.so")
SHAPES = {"H": (0, 1_000_000, 1024, 8, np.float64), "C5": (5, 1 << 18, 1024, 8, np.float32)}
NEW_SYMBOLS = ("svgp_predictive", "svgp_lik_predictive")


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
        model = _ffi.DeviceModel(ctx, *_ffi.make_desc(dt, _ffi.KERNEL_SE, p["variance"], p["inv_lengthscale"], p["z"], p["m"], p["Lq"],
                                                      p["jitter"], lik_sigma2=p["sigma2"]))
        data = _ffi.DeviceData(ctx, p["x"], p["y"], dt)
        row = {"shape": name, "lib": role, "n": n, "M": M, "d": d, "dtype": np.dtype(dt).name, "reps": reps}
        value = model.elbo(data, 0, n, float(n))[0]   # warm-up
        row["elbo_value_hex"] = float(value).hex()
        row["elbo_ms"] = timed(lambda: model.elbo(data, 0, n, float(n)), reps)
        if role == "this":
            model.predictive(data, 0, n)                # warm-up: the call's buffers
            row["predictive_summary_ms"] = timed(lambda: model.predictive(data, 0, n, want=("summary",)), reps)
            row["predictive_all_ms"] = timed(lambda: model.predictive(data, 0, n), reps)
            t = ctx.timing()
            row["predictive_all_device_ms"] = {"prep": round(t.ms_prep, 3), "strip": round(t.ms_strip, 3), "point_stage": round(t.ms_expect, 3)}
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
                                 env=env, capture_output=True, text=True, timeout=600)
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
        row["elbo_ms_this_rounds"] = [x["elbo_ms"][0] for x in mine]
        row["elbo_ms_parent_rounds"] = [x["elbo_ms"][0] for x in prev]
        row["elbo_ms_this"], row["elbo_ms_parent"] = med(mine, "elbo_ms"), med(prev, "elbo_ms")
        row["elbo_value_bitwise_equal_to_parent"] = len({x["elbo_value_hex"] for x in mine + prev}) == 1
        row["predictive_summary_ms"], row["predictive_all_ms"] = med(mine, "predictive_summary_ms"), med(mine, "predictive_all_ms")
        row["predictive_summary_over_parent_elbo"] = round(row["predictive_summary_ms"] / row["elbo_ms_parent"], 4)
        row["predictive_all_over_parent_elbo"] = round(row["predictive_all_ms"] / row["elbo_ms_parent"], 4)
        row["elbo_this_over_parent_elbo"] = round(row["elbo_ms_this"] / row["elbo_ms_parent"], 4)
        row["predictive_all_device_ms"] = mine[-1]["predictive_all_device_ms"]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.shapes, a.reps)
    else:
        driver(a)


if __name__ == "__main__":
    main()
