"""GPU checks of the pathwise sampler (svgp_sampler_*; csrc/sample.hip, sample_api.hip) where tests/test_gpu_pathwise.py is blind:

1. every one of the 20 kernels sample_eval_kernel<T, DREG, NSB>, every dispatch boundary of d, the column blocks (an NSB = 4 launch at
   s0 = 64 with a partial block, three and five launches, S > 256), the row paddings of L and M and the point-group edges of n* - the
   case table of tests/pathwise_cases.py against the float64 restatement tests/pathwise_ref.py, with the protocol and the bands of
   test_gpu_pathwise.py::test_device_matches_restatement (no new tolerance), a per-sample-column bound so that a wrong column block
   names itself, and the bitwise window contract on every case;
2. call order on ONE busy context: the state the sampler shares with other calls (the staged prior means, the model's prep, the
   host-output staging buffer), each ordering bitwise against the same calls on a context opened for them alone;
3. one seeded slice of tests/fuzz_pathwise.py.

tests/test_pathwise_edges_cpu.py asserts what the table and the slice cover.  Observed errors: profiles/sample/accuracy.md."""
import time

import numpy as np
import pytest

import fuzz_families as ff
import fuzz_pathwise as fp
import pathwise_cases as pc
import pathwise_ref as pw
import prior_mean_ref as pmr
import svgp_oracle as o
from approxgp import _ffi

pytestmark = pytest.mark.gpu
OBSERVED = {}
BLOCK64 = 1e-6   # fp64 arrays of marginals (tests/fuzz_families.py: tolerance, the keys that are not VALUE_KEYS)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _alone(ctx, fn):
    """fn on a context of the same device that has run nothing else."""
    c = ff.fresh_context(ctx)
    try:
        return fn(c)
    finally:
        c.close()


def _problem(name, _cache={}):
    if name not in _cache:
        _cache[name] = pc.problem(pc.TABLE[name])
    return _cache[name]


# ---- 1. the case table ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pc.TABLE))
def test_device_matches_restatement_at_the_edges(ctx, name):
    p = _problem(name)
    r = pc.run_case(ctx, p)
    OBSERVED[name] = r
    print(f"{name}: F {r['F']:.2e} (tolerance {r['tol']:.2e}, e32 {r['e32']}), u {r['u']:.2e}, V {r['V']:.2e}, cond {r['cond']:.1e}, "
          f"max|V| {r['vmax']:.1f}; launches {pc.variant(pc.TABLE[name].dtype, pc.TABLE[name].d, pc.TABLE[name].S)}")


def test_report_observed_errors():
    """Prints the rows profiles/sample/accuracy.md records (run the module with -s)."""
    for name, r in OBSERVED.items():
        print(pc.report_line(name, r))
    x = [r["F"] / r["e32"] for n, r in OBSERVED.items() if r["e32"] and 9 <= pc.TABLE[n].d <= 16]
    if x:
        print(f"fp32 expansion form at d = 9..16: {min(x):.2f} - {max(x):.2f} x e32")


# ---- 2. call order on one busy context ------------------------------------------------------------------------------------------------

def _sampler_eval(c, p, off, length, kind="host"):
    """model + data + sampler of the problem on context c, one window -> (S, length)."""
    mdl, dat = pc.model(c, p), pc.data(c, p)
    try:
        smp = mdl.sampler(p["basis"])
        try:
            return smp.eval(dat, off, length, prior_mean=pc.window_mean(p, off, length))
        finally:
            smp.free()
    finally:
        mdl.free()
        dat.free()


def test_staged_prior_means_do_not_leak_between_calls(ctx):
    """sampler.eval with a prior mean, svgp_marginals_with_mean of ANOTHER model with its own mean (another window length and offset: the
    same staging buffer of the context, api_forward.hip: stage_point_mean), the same eval again."""
    pa = _problem("f32_M130_d16_n63_S33_L257")   # with_mean: muz and mux
    pb = _problem("f64_M37_d32_n129_S1_L31")     # another model with means, another dtype (the staging buffer holds another element size)
    wa, wb = (3, 50), (70, 59)
    yb = np.sin(pb["x"][0])
    mb, db = pc.model(ctx, pb), pc.data(ctx, pb, y=yb)
    ma, da = pc.model(ctx, pa), pc.data(ctx, pa)
    try:
        smp = ma.sampler(pa["basis"])
        f1 = smp.eval(da, *wa, prior_mean=pc.window_mean(pa, *wa))
        mu, var = mb.marginals(db, *wb, prior_mean=pc.window_mean(pb, *wb))
        f2 = smp.eval(da, *wa, prior_mean=pc.window_mean(pa, *wa))
        smp.free()
    finally:
        for h in (ma, da, mb, db):
            h.free()
    assert np.array_equal(f1, f2)
    assert np.array_equal(f1, _alone(ctx, lambda c: _sampler_eval(c, pa, *wa)))

    def marg(c):
        m_, d_ = pc.model(c, pb), pc.data(c, pb, y=yb)
        try:
            return m_.marginals(d_, *wb, prior_mean=pc.window_mean(pb, *wb))
        finally:
            m_.free()
            d_.free()
    mu0, var0 = _alone(ctx, marg)
    assert np.array_equal(mu, mu0) and np.array_equal(var, var0)
    # ... and both are right
    pc.check_columns(f1, pa["F"][:, wa[0]:wa[0] + wa[1]], pc.tolerance(pa), float(np.abs(pa["F"]).max()))
    rmu, rvar = pmr.marginals(pb["sva"], pb["x"][:, wb[0]:wb[0] + wb[1]], pc.window_mean(pb, *wb), pb["muz"])
    assert pc.rel(mu, rmu) <= BLOCK64 and pc.rel(var, rvar) <= BLOCK64, (pc.rel(mu, rmu), pc.rel(var, rvar))


def test_host_staging_is_reused_at_a_smaller_then_a_larger_size(ctx):
    """Two live samplers of different dtype, S and n*, host output: large, small, large (ctx->smp_out is sized by the last call)."""
    pl, ps = _problem("f64_M130_d33_n257_S16_L33"), _problem("f32_M17_d2_n17_S129_L0")
    ml, dl, ms, ds = pc.model(ctx, pl), pc.data(ctx, pl), pc.model(ctx, ps), pc.data(ctx, ps)
    try:
        sl, ss = ml.sampler(pl["basis"]), ms.sampler(ps["basis"])
        a = sl.eval(dl)
        b = ss.eval(ds, 2, 9)
        c_ = sl.eval(dl)
        d_ = ss.eval(ds, ldo=40)
        sl.free()
        ss.free()
    finally:
        for h in (ml, dl, ms, ds):
            h.free()
    assert np.array_equal(a, c_)
    assert np.array_equal(a, _alone(ctx, lambda c: _sampler_eval(c, pl, 0, 257)))
    assert np.array_equal(b, _alone(ctx, lambda c: _sampler_eval(c, ps, 2, 9)))
    assert np.array_equal(d_[:, :17], _alone(ctx, lambda c: _sampler_eval(c, ps, 0, 17))) and np.all(d_[:, 17:] == 0.0)
    pc.check_columns(a, pl["F"], pc.tolerance(pl))
    pc.check_columns(d_[:, :17], ps["F"], pc.tolerance(ps))
    pc.check_columns(b, ps["F"][:, 2:11], pc.tolerance(ps), float(np.abs(ps["F"]).max()))


@pytest.mark.parametrize("centered", [False, True])
def test_sampler_after_keep_q_and_an_unfetched_step(ctx, centered):
    """svgp_model_update_keep_q (new kernel parameters and z; the prep is stale), an UNFETCHED natgrad_step, then the sampler: equal to
    a sampler of a fresh model built at the new parameters and the fetched q, and to the restatement there."""
    p = _problem("f64_M127_d4_n65_S16_L31")
    base = p["sva"]
    sva = o.SVA(base.kernel, base.z, base.m, base.Lq, jitter=pc.JITTER, mean_const=pc.MEAN_CONST, centered=False)
    if centered:
        Kuu = o.kuu(sva)
        Lk = np.linalg.cholesky(Kuu)
        sva = o.SVA(base.kernel, base.z, pc.MEAN_CONST + Lk @ base.m, Lk @ base.Lq, jitter=pc.JITTER, mean_const=pc.MEAN_CONST, centered=True)
    k2 = o.Kernel(base.kernel.family, 0.9, 1.1 * base.kernel.inv_lengthscale)
    z2 = 0.95 * base.z
    par = _ffi.CENTERED if centered else _ffi.NONCENTERED
    y = np.sin(p["x"][0]) + 0.3
    dat = pc.data(ctx, p, y=y)

    def moved(fetch):
        mdl = pc.model(ctx, p, sva)
        desc, keep = _ffi.make_desc(np.float64, k2.family, k2.variance, k2.inv_lengthscale, z2, sva.m, sva.Lq, pc.JITTER, parametrization=par,
                                    lik_sigma2=0.1, mean_const=pc.MEAN_CONST)
        mdl.update_keep_q(desc, keep)
        return mdl, mdl.natgrad_step(dat, gamma=0.7, fetch=fetch)[3:]
    try:
        unfetched, q = moved(False)
        try:
            assert q == (None, None)
            s1 = unfetched.sampler(p["basis"])
            f1 = s1.eval(dat)
            s1.free()
        finally:
            unfetched.free()
        fetched, (mq, Lq) = moved(True)
        fetched.free()
        at_q = o.SVA(k2, z2, mq.astype(np.float64), np.tril(Lq).astype(np.float64), jitter=pc.JITTER, mean_const=pc.MEAN_CONST, centered=centered)
        fresh = pc.model(ctx, p, at_q)
        try:
            s2 = fresh.sampler(p["basis"])
            f2 = s2.eval(dat)
            s2.free()
        finally:
            fresh.free()
    finally:
        dat.free()
    assert np.all(np.isfinite(f1)) and np.array_equal(f1, f2)
    omega, tau, w, eps = (a.astype(np.float64) for a in p["basis"])
    st = pw.setup(at_q, omega, tau, w, eps)
    assert st["cond"] <= pc.COND_MAX and np.abs(st["V"]).max() <= pc.V_MAX, (st["cond"], np.abs(st["V"]).max())
    pc.check_columns(f1, pw.evaluate(at_q, st, p["x"], omega, tau, w), pc.TOL64)


def test_reads_between_create_and_eval_change_nothing(ctx):
    """elbo, grad, predict and collapsed_bound on the SAME model between svgp_sampler_create and _eval: each bitwise what it was before the
    create, and the sampler (its samples, u and V) bitwise what it is without them."""
    p = _problem("f32_M256_d6_n129_S65_L100")
    c = p["case"]
    y = np.sin(p["x"][0])
    xq = pc._laid_out(p["x"], c.d, c.layout_x)
    mdl, dat = pc.model(ctx, p), pc.data(ctx, p, y=y)

    def reads():
        v, t, g = mdl.elbo_grad(dat)
        return dict(elbo=mdl.elbo(dat)[0], value=v, predict_mean=mdl.predict(xq, True, True, False, layout=c.layout_x)[0],
                    predict_var=mdl.predict(xq, True, True, False, layout=c.layout_x)[1], bound=mdl.collapsed_bound(dat)[0],
                    **ff._grads_raw(g))
    try:
        before = reads()
        smp = mdl.sampler(p["basis"])
        between = reads()
        F = smp.eval(dat)
        after = reads()
        F2 = smp.eval(dat)
        u, V = smp.state()
        smp.free()
        # the same sampler with nothing between create and eval
        quiet = mdl.sampler(p["basis"])
        F0 = quiet.eval(dat)
        u0, V0 = quiet.state()
        quiet.free()
    finally:
        mdl.free()
        dat.free()
    assert ff._same(before, between) is None, ff._same(before, between)
    assert ff._same(before, after) is None, ff._same(before, after)
    assert np.array_equal(F, F0) and np.array_equal(F, F2) and np.array_equal(u, u0) and np.array_equal(V, V0)
    assert np.array_equal(F, _alone(ctx, lambda c_: _sampler_eval(c_, p, 0, c.n)))
    pc.check_columns(F, p["F"], pc.tolerance(p))


def test_a_failed_create_leaves_the_live_sampler_and_the_context_whole(ctx):
    """SVGP_NOT_POSDEF from svgp_sampler_create (a NaN inducing input) while another sampler is live: the early return releases its
    half-built sampler and workspace, the live sampler's next eval is bitwise unchanged, the next create is healthy."""
    live, nxt = _problem("f64_M37_d3_n17_S81_L33"), _problem("f32_M37_d9_n64_S16_L256")
    ml, dl = pc.model(ctx, live), pc.data(ctx, live)
    try:
        smp = ml.sampler(live["basis"])
        F0 = smp.eval(dl, prior_mean=live["mux"])
        sva = live["sva"]
        z = sva.z.copy()
        z[1, 5] = np.nan
        bad = o.SVA(sva.kernel, z, sva.m, sva.Lq, jitter=pc.JITTER, mean_const=pc.MEAN_CONST, centered=sva.centered)
        singular = pc.model(ctx, live, bad)
        try:
            for _ in range(2):
                with pytest.raises(_ffi.PosDefException):
                    singular.sampler(live["basis"])
        finally:
            singular.free()
        F1 = smp.eval(dl, prior_mean=live["mux"])
        u, V = smp.state()
        smp.free()
    finally:
        ml.free()
        dl.free()
    assert np.array_equal(F0, F1)
    assert pc.rel(u, live["st"]["u"]) <= pc.TOL_U and pc.rel(V, live["st"]["V"]) <= pc.TOL_V
    pc.check_columns(F0, live["F"], pc.tolerance(live))
    pc.run_case(ctx, nxt, windows=False)   # a following create on a healthy model matches the restatement


# ---- 3. the seeded slice --------------------------------------------------------------------------------------------------------------

def test_seeded_slice_of_the_sweep(ctx):
    t0 = time.time()
    results = fp.execute(ctx, fp.slice_plan())
    dt = time.time() - t0
    for (dtn, R, NSB), w in sorted(fp.worst(results).items()):
        print(f"{dtn} DREG {R} NSB {NSB}: {w['n']} cases, worst F {w['F']:.2e} = {w['share']:.3f} of its tolerance" + (
            f", {w['xe32']:.2f} x e32" if dtn == "float32" else ""))
    print(f"{len(results)} cases in {dt:.1f} s, {sum(r['skipped'] for r in results)} skipped")
    assert not fp.failures(results), "\n".join(fp.failures(results))
    fp.check_skips(results)
    done = [r for r in results if "F" in r]
    assert pc.ALL_VARIANTS == set().union(*(r["variants"] for r in done))


@pytest.mark.parametrize("name", list(fp.REPLAYS))
def test_replayed_findings_of_the_long_run(ctx, name):
    """The two cases of the long run (seed 41, 5520 cases, profiles/sample/fuzz_pathwise.md) that were outside the fp32 band, both fp32,
    M = 300, d = 1, SE, inside the stated conditions: 1.29e-4 (centered, n* = 64, L = 1) and 1.12e-4 (n* = 1000, L = 0) of max|F|
    against max(1e-4, 4 e32) = 1e-4, in all three samples.  Cause: the by-differences path of sample_eval_kernel subtracted the SCALED
    coordinates (eps32 |xs| absolutely, |xs| up to 300 here); it now scales the difference of the unscaled ones."""
    r = fp.run_one(ctx, fp.REPLAYS[name])
    assert not r["skipped"]
    print(f"{name}: F {r['F']:.2e} (tolerance {r['tol']:.2e}, e32 {r['e32']})")
