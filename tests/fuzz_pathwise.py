"""Seeded sweep of the pathwise sampler (svgp_sampler_create / _eval / _state) against the float64 restatement tests/pathwise_ref.py:
shapes drawn from the edges of the dispatch and of the paddings (tests/pathwise_cases.py: SWEEP), kernel family, parametrisation,
dtype, layout of z and of x, prior means, output kind and a random window.

    plan(rng, n)        -> n cases (no device, no reference: the draws alone)
    execute(ctx, plan)  -> one record per case; ctx = None runs the reference side alone

Every case is held to the bands of tests/test_gpu_pathwise.py (pathwise_cases.run_case: u 1e-10, V 1e-8, F fp64 1e-8 / fp32
max(1e-4, 4 e32) per sample column) and to the window contract: the window is bitwise equal to the same columns of the whole.  A case
whose restatement breaks the stated conditions (cond(Kuu) <= 1e4, max|V| <= 64) is skipped and counted; a slice with more than 5 % of
its cases skipped fails (`check_skips`).

    python tests/fuzz_pathwise.py [--seconds 120] [--seed 7]

is the long run for the GPU box (exit code 1 on a failure); it prints the worst error per dtype and kernel variant, the table of
profiles/sample/fuzz_pathwise.md."""
import argparse
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library, as tests/conftest.py: the device-output cases allocate their buffers with torch.cuda)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "approximategps.jl_amd", "tests"):
    if os.path.join(ROOT, p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, p))

import pathwise_cases as pc  # noqa: E402

SLICE_SEED, SLICE_CASES = 7, 60   # the seeded slice of tests/test_gpu_pathwise_edges.py; tests/test_pathwise_edges_cpu.py asserts its coverage
MAX_SKIPPED = 0.05


# Findings of the long run (profiles/sample/fuzz_pathwise.md; fp32 differences of scaled coordinates, since corrected in csrc/sample.hip),
# replayed by tests/test_gpu_pathwise_edges.py: name -> record of `plan`
REPLAYS = {
    "f32_M300_d1_n64_S3_L1_centered": dict(case=pc.Case(pc.F32, 300, 1, 64, 3, 1, pc.SE, True, pc.ROW, pc.COL, False, "host", 0),
                                           seed=361622964, window=(49, 3)),
    "f32_M300_d1_n1000_S3_L0": dict(case=pc.Case(pc.F32, 300, 1, 1000, 3, 0, pc.SE, False, pc.COL, pc.COL, False, "host_ld", 0),
                                    seed=136678254, window=(527, 398)),
}


def draw(rng):
    """One case and its seed -> dict(case, seed, window = (off, len))."""
    pick = lambda k: pc.SWEEP[k][int(rng.integers(len(pc.SWEEP[k])))]
    n = pick("n")
    off = int(rng.integers(0, n))
    length = int(rng.integers(1, n - off + 1))
    c = pc.Case(dtype=pc.F32 if rng.random() < 0.5 else pc.F64, M=pick("M"), d=pick("d"), n=n, S=pick("S"), L=pick("L"), family=pick("family"),
                centered=bool(rng.random() < 0.4), layout_z=pc.ROW if rng.random() < 0.4 else pc.COL, layout_x=pc.ROW if rng.random() < 0.4 else pc.COL,
                with_mean=bool(rng.random() < 0.3), out=pick("out"), off=0)
    return dict(case=c, seed=int(rng.integers(1, 1 << 30)), window=(off, length))


def plan(rng, n):
    return [draw(rng) for _ in range(n)]


def slice_plan():
    return plan(np.random.default_rng(SLICE_SEED), SLICE_CASES)


def run_one(ctx, rec):
    """-> dict(name, variants, skipped, [errors]).  Raises AssertionError when the device is outside a band or breaks the window contract."""
    c = rec["case"]
    p = pc.problem(c, seed=rec["seed"])
    out = dict(name=pc.case_name(c), variants=pc.variants_of([c]), cond=p["st"]["cond"], vmax=p["vmax"], skipped=not pc.meets_conditions(p))
    if out["skipped"] or ctx is None:
        return out
    # the random window goes through the case's output kind (sentinels beyond len included) and is compared bitwise with the whole
    out.update(pc.run_case(ctx, p, windows=False, window=rec["window"]))
    return out


def execute(ctx, plan_, log=None):
    results = []
    for i, rec in enumerate(plan_):
        try:
            r = run_one(ctx, rec)
        except AssertionError as e:
            r = dict(name=pc.case_name(rec["case"]), variants=pc.variants_of([rec["case"]]), skipped=False, failure=f"{rec}: {e}")
        if log:
            log(i, r)
        results.append(r)
    return results


def failures(results):
    return [r["failure"] for r in results if "failure" in r]


def skipped_share(results):
    return sum(r["skipped"] for r in results) / max(len(results), 1)


def check_skips(results):
    share = skipped_share(results)
    assert share <= MAX_SKIPPED, f"{share:.1%} of the cases break the stated conditions: " + ", ".join(
        f"{r['name']} (cond {r['cond']:.1e}, max|V| {r['vmax']:.1f})" for r in results if r["skipped"])


def worst(results, into=None):
    """(dtype, DREG, NSB) -> the largest F error of a case that launched it, as a multiple of its tolerance and in absolute terms."""
    into = {} if into is None else into
    for r in results:
        if "F" not in r:
            continue
        for v in r["variants"]:
            w = into.setdefault(v, dict(F=0.0, share=0.0, xe32=0.0, n=0))
            w["n"] += 1
            w["F"] = max(w["F"], r["F"])
            w["share"] = max(w["share"], r["F"] / r["tol"])
            if r["e32"]:
                w["xe32"] = max(w["xe32"], r["F"] / r["e32"])
    return into


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=SLICE_SEED)
    args = ap.parse_args()
    from approxgp import _ffi

    rng = np.random.default_rng(args.seed)
    ctx = _ffi.Context(0)
    t0, results = time.time(), []
    while time.time() - t0 < args.seconds:
        results += execute(ctx, plan(rng, 20), log=lambda i, r: print("CASE", r["name"], "SKIPPED" if r["skipped"] else r.get("failure") or
                                                                       f"ok F {r['F']:.2e} of {r['tol']:.2e}", flush=True))
    ctx.close()
    bad = failures(results)
    print(f"SUMMARY {len(results)} cases in {time.time() - t0:.0f} s, {len(bad)} failures, {sum(r['skipped'] for r in results)} skipped")
    print("| dtype | DREG | NSB | cases | worst F | of its tolerance | x e32 |\n|---|---|---|---|---|---|---|")
    for (dt, R, NSB), w in sorted(worst(results).items()):
        print(f"| {dt} | {R} | {NSB} | {w['n']} | {w['F']:.2e} | {w['share']:.3f} | {'-' if dt == 'float64' else format(w['xe32'], '.2f')} |")
    for b in bad:
        print("  BAD", b)
    check_skips(results)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
