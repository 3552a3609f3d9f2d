"""GPU checks of pathwise posterior function samples (svgp_sampler_create / _eval / _state / _free; csrc/sample.hip, sample_api.hip)
against the float64 restatement tests/pathwise_ref.py (itself pinned by tests/test_pathwise_cpu.py) on the SAME (omega, tau, w, eps).

Shapes: the smallest at which the tiling can go wrong - M = 1, below, one past and between the 128-row panels (37, 130, 257, 300);
d = 1, 2, 3 (one MFMA k-step), 17 and 64 (the widest fragment); n* = 1, 129 (one past two 64-point wave tiles), 1000 (several
workgroups, a ragged last one); S = 1, 3, 17 (two 16-column blocks), 70 (a second launch of the 64-column block loop); L = 0, 1, 100
(padded to 128), 1030 (33 chunks of 32).  Three families with ARD, both dtypes, both parametrisations, ColVecs / RowVecs / Vec,
mean_const != 0, svgp_model_set_mean_z + pm, host and device output with ldo > len.

Conditions: z ~ U[-3, 3]^d, inverse lengthscales 0.8 M^(1/d) / 3 * U[0.8, 1.25], jitter 1e-3 (pathwise_ref.recipe).  The amplification
of Kuu^-1 is a stated condition: every case asserts cond(Kuu) <= 1e4 and max|V| <= 64 on the restatement before the device is called.

Tolerances: fp64 1e-8 of max|F| (the project's contract).  fp32: max(1e-4, F32_FACTOR e32) max|F| per case, e32 = the error of the
restatement's own float32 data stage against its float64 one, computed here; the factor covers the device's single MFMA chain over
M + L terms and, at d > 8, its expansion-form distances, which numpy's evaluation does not share (at d <= 8 the fp32 kernel forms r^2
by differences too: the expansion loses eps32 (|xs|^2 + |zs|^2), above the 1e-4 contract at M = 37, d = 1).  The factor was 8 and is
tightened to 4 after the measurement: observed 0.8 - 3.2 e32, <= 5.5e-6 of max|F|; per case in profiles/sample/accuracy.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import pathwise_ref as pw
import svgp_oracle as o
from approxgp import _ffi
from approxgp.pathwise import draw_basis

pytestmark = pytest.mark.gpu
JITTER = 1e-3
TOL64 = 1e-8
F32_FACTOR = 4.0   # the band started at 8 e32; observed on an MI355X: 0.8 - 3.2 e32 (profiles/sample/accuracy.md), so it is tightened
SE, M32, M52 = o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52
COL, ROW = _ffi.COLVECS, _ffi.ROWVECS

# name: (M, d, n*, S, L, family, centered, layout, mean_const, muz + pm, output: "host" | "host_ld" | "dev_ld")
CASES = {
    "M1_d1_n1_S1_L0": (1, 1, 1, 1, 0, SE, False, COL, 0.0, False, "host"),
    "M37_d1_n129_S3_L1": (37, 1, 129, 3, 1, M32, True, COL, 0.7, False, "host"),
    "M130_d2_n1000_S17_L100": (130, 2, 1000, 17, 100, M52, False, COL, 0.0, False, "dev_ld"),
    "M257_d3_n1000_S70_L1030": (257, 3, 1000, 70, 1030, SE, True, ROW, -0.4, True, "host"),
    "M300_d17_n129_S17_L100": (300, 17, 129, 17, 100, M32, False, COL, 0.0, False, "host"),
    "M130_d64_n129_S17_L100": (130, 64, 129, 17, 100, SE, False, ROW, 0.0, False, "host_ld"),
    "M300_d2_n1_S70_L0": (300, 2, 1, 70, 0, M52, True, COL, 0.2, True, "host"),
    "f32_M37_d1_n1000_S3_L100": (37, 1, 1000, 3, 100, SE, False, COL, 0.0, False, "host"),
    "f32_M257_d3_n1000_S70_L1030": (257, 3, 1000, 70, 1030, M52, True, COL, -0.4, True, "dev_ld"),
    "f32_M300_d17_n129_S17_L100": (300, 17, 129, 17, 100, M32, False, ROW, 0.5, False, "host_ld"),
    "f32_M130_d64_n129_S1_L1": (130, 64, 129, 1, 1, SE, True, COL, 0.0, False, "host"),
    "f32_M1_d2_n129_S17_L0": (1, 2, 129, 17, 0, M32, False, COL, 0.0, False, "host"),
}
OBSERVED = {}   # name -> relative error of the device against the float64 restatement (printed by the last test)


def _dtype(name):
    return np.float32 if name.startswith("f32") else np.float64


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Everything of a case, computed once and shared read-only: the model, the points, the basis (rounded to the case's dtype, so that
    the restatement and the device start from the same numbers) and the restatement's results."""
    M, d, n, S, L, family, centered, layout, mc, with_mean, out = CASES[name]
    dt = _dtype(name)
    rd = lambda a: np.asarray(a, dtype=dt).astype(np.float64)
    seed = 1000 + 7 * M + 13 * d + n + S + L
    sva, muz = pw.recipe(M, d, family, seed, centered=centered, mean_const=mc, with_muz=with_mean, jitter=JITTER, dtype=dt)
    rng = np.random.default_rng(seed + 1)
    x = rd(rng.uniform(-3.0, 3.0, size=(d, n)))
    mux = rd(0.3 * np.cos(x[0])) if with_mean else None
    basis = draw_basis(family, M, L, S, rng, dt, d=d)
    omega, tau, w, eps = (a.astype(np.float64) for a in basis)
    st = pw.setup(sva, omega, tau, w, eps, muz=muz)
    F = pw.evaluate(sva, st, x, omega, tau, w, mux=mux)
    e32 = None
    if dt == np.float32:
        e32 = float(np.abs(pw.evaluate(sva, st, x, omega, tau, w, mux=mux, f32=True).astype(np.float64) - F).max() / np.abs(F).max())
    for a in (x, F, st["u"], st["V"]) + tuple(basis) + ((muz, mux) if with_mean else ()):
        a.setflags(write=False)
    return dict(sva=sva, muz=muz, x=x, mux=mux, basis=basis, st=st, F=F, e32=e32)


def _tolerance(name):
    p = _problem(name)
    return TOL64 if p["e32"] is None else max(1e-4, F32_FACTOR * p["e32"])


def _model(ctx, name, sva=None):
    M, d, n, S, L, family, centered, layout, mc, with_mean, out = CASES[name]
    p = _problem(name)
    sva = sva if sva is not None else p["sva"]
    z = sva.z[0] if d == 1 else (sva.z if layout == COL else np.ascontiguousarray(sva.z.T))
    desc, keep = _ffi.make_desc(_dtype(name), sva.kernel.family, sva.kernel.variance, sva.kernel.inv_lengthscale, z, sva.m, sva.Lq,
                                sva.jitter, parametrization=_ffi.CENTERED if sva.centered else _ffi.NONCENTERED, lik_sigma2=0.1,
                                mean_const=sva.mean_const, layout_z=layout)
    model = _ffi.DeviceModel(ctx, desc, keep)
    if p["muz"] is not None:
        model.set_mean_z(p["muz"])
    return model


def _data(ctx, name, x=None, y=None):
    d, layout = CASES[name][1], CASES[name][7]
    x = _problem(name)["x"] if x is None else x
    xd = x[0] if d == 1 else (x if layout == COL else np.ascontiguousarray(x.T))
    return _ffi.DeviceData(ctx, xd, y, _dtype(name), layout=layout)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _eval_device_memory(sampler, data, n, ldo, prior_mean=None, off=0):
    """eval into device memory, rows ldo apart -> the (S, ldo) buffer on the host (columns >= n keep the sentinel)."""
    import torch

    tdt = torch.float32 if sampler.dtype == _ffi.F32 else torch.float64
    buf = torch.full((sampler.n_samples, ldo), -777.0, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    sampler.eval(data, off, n, prior_mean=prior_mean, out=buf, ldo=ldo)
    return buf.cpu().numpy()


def _run(ctx, name):
    """The case on the device -> (F (S, n), u, V)."""
    n, S, out = CASES[name][2], CASES[name][3], CASES[name][10]
    p = _problem(name)
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        smp = model.sampler(p["basis"])
        try:
            if out == "dev_ld":
                full = _eval_device_memory(smp, data, n, n + 5, prior_mean=p["mux"])
                assert np.all(full[:, n:] == -777.0), "columns beyond len were written"
                F = full[:, :n]
            elif out == "host_ld":
                full = smp.eval(data, prior_mean=p["mux"], ldo=n + 3)
                assert np.all(full[:, n:] == 0.0), "columns beyond len were written"
                F = full[:, :n]
            else:
                F = smp.eval(data, prior_mean=p["mux"])
            u, V = smp.state()
        finally:
            smp.free()
    finally:
        model.free()
        data.free()
    assert F.shape == (S, n) and F.dtype == _dtype(name)
    return F, u, V


@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_restatement(ctx, name):
    p = _problem(name)
    st = p["st"]
    assert st["cond"] <= 1e4 and np.abs(st["V"]).max() <= 64.0, (st["cond"], np.abs(st["V"]).max())   # the stated conditions
    F, u, V = _run(ctx, name)
    # the M-sized stage is fp64 for both dtypes: u and V agree with the restatement far below the data stage's tolerance
    eu, eV = _rel(u, st["u"]), _rel(V, st["V"])
    err, tol = _rel(F, p["F"]), _tolerance(name)
    OBSERVED[name] = (err, tol, p["e32"], eu, eV, st["cond"], float(np.abs(st["V"]).max()))
    print(f"{name}: F {err:.2e} (tolerance {tol:.2e}, e32 {p['e32']}), u {eu:.2e}, V {eV:.2e}, cond {st['cond']:.1e}, max|V| {np.abs(st['V']).max():.1f}")
    assert eu <= 1e-10 and eV <= 1e-8, (eu, eV)
    assert np.all(np.isfinite(F))
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("name", ["M257_d3_n1000_S70_L1030", "M37_d1_n129_S3_L1", "f32_M300_d17_n129_S17_L100"])
def test_identity_at_the_inducing_points(ctx, name):
    """eval at x* = z plus jitter V equals u of svgp_sampler_state (pm = muz there): the update term is exact whatever L is."""
    p = _problem(name)
    model = _model(ctx, name)
    data = _data(ctx, name, x=p["sva"].z)
    try:
        smp = model.sampler(p["basis"])
        F = smp.eval(data, prior_mean=p["muz"]).astype(np.float64)
        u, V = smp.state()
        smp.free()
    finally:
        model.free()
        data.free()
    err = float(np.abs(F.T + JITTER * V - u).max() / np.abs(u).max())
    print(f"{name}: |f(z) + jitter V - u| / max|u| = {err:.2e}")
    # fp64: rounding of the data stage (the contract); fp32: the data stage's own tolerance
    assert err <= _tolerance(name)


@pytest.mark.parametrize("name", ["M130_d2_n1000_S17_L100", "f32_M257_d3_n1000_S70_L1030"])
def test_windows_and_repeats_are_bitwise(ctx, name):
    """A sample is a function: the value of a point does not depend on the window or the call it is evaluated in."""
    n = CASES[name][2]
    p = _problem(name)
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        smp = model.sampler(p["basis"])
        whole = smp.eval(data, prior_mean=p["mux"])
        again = smp.eval(data, prior_mean=p["mux"])
        cut = 389
        a = smp.eval(data, 0, cut, prior_mean=None if p["mux"] is None else p["mux"][:cut])
        b = smp.eval(data, cut, n - cut, prior_mean=None if p["mux"] is None else p["mux"][cut:])
        one = smp.eval(data, 700, 1, prior_mean=None if p["mux"] is None else p["mux"][700:701])
        # a second sampler from the same model and basis is the same functions
        smp2 = model.sampler(p["basis"])
        other = smp2.eval(data, prior_mean=p["mux"])
        smp2.free()
        smp.free()
    finally:
        model.free()
        data.free()
    assert np.array_equal(whole, again)
    assert np.array_equal(whole, np.concatenate([a, b], axis=1))
    assert np.array_equal(whole[:, 700:701], one)
    assert np.array_equal(whole, other)


@pytest.mark.parametrize("name", ["M130_d2_n1000_S17_L100", "f32_M37_d1_n1000_S3_L100"])
def test_sampler_is_a_snapshot_and_leaves_the_elbo_alone(ctx, name):
    """Bitwise unchanged after svgp_model_update and after svgp_model_free; svgp_elbo bitwise equal before and after."""
    M, d, n = CASES[name][:3]
    p = _problem(name)
    sva = p["sva"]
    y = np.sin(p["x"][0])
    model, data = _model(ctx, name), _data(ctx, name, y=y)
    try:
        e0 = model.elbo(data)[0]
        smp = model.sampler(p["basis"])
        before = smp.eval(data)
        e1 = model.elbo(data)[0]
        assert e0 == e1
        k2 = o.Kernel(sva.kernel.family, 0.6, 1.7 * sva.kernel.inv_lengthscale)
        other = o.SVA(k2, 0.5 * sva.z, sva.m + 1.0, sva.Lq * 0.5, jitter=sva.jitter, mean_const=2.0, centered=sva.centered)
        z = other.z[0] if d == 1 else other.z
        desc, keep = _ffi.make_desc(_dtype(name), k2.family, k2.variance, k2.inv_lengthscale, z, other.m, other.Lq, other.jitter,
                                    parametrization=_ffi.NONCENTERED, lik_sigma2=0.1, mean_const=2.0)
        model.update(desc, keep)
        assert model.elbo(data)[0] != e0
        after_update = smp.eval(data)
        model.free()
        after_free = smp.eval(data)
        smp.free()
    finally:
        model.free()
        data.free()
    assert np.array_equal(before, after_update) and np.array_equal(before, after_free)


@pytest.mark.parametrize("centered", [False, True])
def test_sampler_reads_the_device_resident_q(ctx, centered):
    """A sampler created right after an UNFETCHED svgp_collapsed_q / svgp_natgrad_step equals one created from the fetched q."""
    name = "M130_d2_n1000_S17_L100"
    p = _problem(name)
    base = p["sva"]
    sva = o.SVA(base.kernel, base.z, base.m, base.Lq, jitter=JITTER, mean_const=0.3, centered=False)
    if centered:
        Kuu = o.kuu(sva)
        Lk = np.linalg.cholesky(Kuu)
        sva = o.SVA(base.kernel, base.z, 0.3 + Lk @ base.m, Lk @ base.Lq, jitter=JITTER, mean_const=0.3, centered=True)
    y = np.sin(p["x"][0]) + 0.3
    data = _data(ctx, name, y=y)
    results = {}
    try:
        for call in ("collapsed", "natgrad"):
            step = (lambda m, fetch: m.collapsed_q(data, fetch=fetch)[1:]) if call == "collapsed" else (
                lambda m, fetch: m.natgrad_step(data, gamma=0.7, fetch=fetch)[3:])
            unfetched, fetched = _model(ctx, name, sva), _model(ctx, name, sva)
            try:
                assert step(unfetched, False) == (None, None)
                s1 = unfetched.sampler(p["basis"])
                f1 = s1.eval(data)
                s1.free()
                mq, Lq = step(fetched, True)
            finally:
                unfetched.free()
                fetched.free()
            fresh = _model(ctx, name, o.SVA(sva.kernel, sva.z, mq, Lq, jitter=JITTER, mean_const=0.3, centered=centered))
            try:
                s2 = fresh.sampler(p["basis"])
                f2 = s2.eval(data)
                s2.free()
            finally:
                fresh.free()
            results[call] = (f1, f2)
    finally:
        data.free()
    for call, (f1, f2) in results.items():
        assert np.all(np.isfinite(f1)), call
        assert np.array_equal(f1, f2), call
    assert not np.array_equal(results["collapsed"][0], results["natgrad"][0])


def test_statuses_then_a_healthy_call(ctx):
    name = "M37_d1_n129_S3_L1"
    p = _problem(name)
    lib = ctx.lib
    omega, tau, w, eps = p["basis"]
    ptr = _ffi._ptr
    model, data = _model(ctx, name), _data(ctx, name)
    other_d = _ffi.DeviceData(ctx, np.zeros((2, 5)), None, np.float64)
    other_t = _ffi.DeviceData(ctx, np.zeros(5), None, np.float32)
    try:
        h = C.c_void_p()
        bad = [_ffi.SampleBasis(1, 0, ptr(omega), ptr(tau), ptr(w), ptr(eps)),     # S < 1
               _ffi.SampleBasis(-1, 3, ptr(omega), ptr(tau), ptr(w), ptr(eps)),    # L < 0
               _ffi.SampleBasis(1, 3, None, ptr(tau), ptr(w), ptr(eps)),           # NULL arrays that L makes non-empty
               _ffi.SampleBasis(1, 3, ptr(omega), None, ptr(w), ptr(eps)),
               _ffi.SampleBasis(1, 3, ptr(omega), ptr(tau), None, ptr(eps)),
               _ffi.SampleBasis(0, 3, None, None, None, None)]                     # NULL eps (M >= 1)
        for b in bad:
            assert lib.svgp_sampler_create(ctx.h, model.h, C.byref(b), C.byref(h)) == _ffi.INVALID_ARG and not h.value
        assert lib.svgp_sampler_create(ctx.h, None, C.byref(bad[0]), C.byref(h)) == _ffi.INVALID_ARG
        smp = model.sampler(p["basis"])
        buf = np.zeros((3, 129))
        ev = lambda d_, off, n, ldo, out=buf: lib.svgp_sampler_eval(ctx.h, smp.h, d_.h, off, n, None, ptr(out), ldo, 0)
        assert ev(other_d, 0, 5, 5) == _ffi.INVALID_ARG       # d mismatch
        assert ev(other_t, 0, 5, 5) == _ffi.INVALID_ARG       # dtype mismatch
        assert ev(data, 0, 0, 129) == _ffi.INVALID_ARG        # empty window
        assert ev(data, 100, 30, 129) == _ffi.INVALID_ARG     # window past the data
        assert ev(data, -1, 5, 129) == _ffi.INVALID_ARG
        assert ev(data, 0, 129, 128) == _ffi.INVALID_ARG      # ldo < len
        assert lib.svgp_sampler_eval(ctx.h, smp.h, data.h, 0, 129, None, None, 129, 0) == _ffi.INVALID_ARG
        assert np.all(buf == 0.0)
        # Kuu that is not positive definite, as svgp_elbo meets it: a NaN inducing input (include/svgp_mi355x.h: LAPACK's rule)
        sva = p["sva"]
        z = sva.z.copy()
        z[0, 1] = np.nan
        desc, keep = _ffi.make_desc(np.float64, sva.kernel.family, sva.kernel.variance, sva.kernel.inv_lengthscale, z[0], sva.m, sva.Lq, JITTER,
                                    parametrization=_ffi.CENTERED, mean_const=sva.mean_const)
        singular = _ffi.DeviceModel(ctx, desc, keep)
        try:
            with pytest.raises(_ffi.PosDefException):
                singular.sampler(p["basis"])
        finally:
            singular.free()
        # non-finite inputs: non-finite outputs, SVGP_OK
        xn = p["x"].copy()
        xn[0, 3] = np.nan
        dn = _data(ctx, name, x=xn)
        Fn = smp.eval(dn)
        dn.free()
        assert np.all(np.isnan(Fn[:, 3])) and np.all(np.isfinite(np.delete(Fn, 3, axis=1)))
        # ... and the same context, model and sampler are healthy
        F = smp.eval(data)
        smp.free()
    finally:
        model.free()
        data.free()
        other_d.free()
        other_t.free()
    assert _rel(F, p["F"]) <= TOL64


@pytest.mark.parametrize("name", ["M300_d2_n1_S70_L0", "M130_d2_n1000_S17_L100", "f32_M257_d3_n1000_S70_L1030"])
def test_no_features_and_no_noise_is_the_posterior_mean(ctx, name):
    """L = 0 and eps = 0: every sample equals svgp_predict's mean (plus the caller's offsets)."""
    M, d, n, S = CASES[name][:4]
    layout = CASES[name][7]
    p = _problem(name)
    dt = _dtype(name)
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        smp = model.sampler((np.zeros((0, d), dt), np.zeros(0, dt), np.zeros((2, 0), dt), np.zeros((2, M), dt)))
        F = smp.eval(data, prior_mean=p["mux"]).astype(np.float64)
        smp.free()
        x = p["x"]
        xd = x[0] if d == 1 else (x if layout == COL else np.ascontiguousarray(x.T))
        mean = model.predict(xd, True, False, False, layout=layout)[0].astype(np.float64)
    finally:
        model.free()
        data.free()
    if p["mux"] is not None:
        mean = mean + p["mux"]
    scale = max(np.abs(mean).max(), 1e-300)
    err = float(np.abs(F - mean[None, :]).max() / scale)
    print(f"{name}: |sample - predict mean| / max|mean| = {err:.2e}")
    assert np.array_equal(F[0], F[1])
    assert err <= _tolerance(name)


def test_report_observed_errors():
    """Prints the table profiles/sample/accuracy.md records (run the module with -s)."""
    for name, (err, tol, e32, eu, eV, cond, vmax) in OBSERVED.items():
        print(f"| {name} | {err:.2e} | {tol:.2e} | {'-' if e32 is None else format(e32, '.2e')} | {eu:.1e} | {eV:.1e} | {cond:.1e} | {vmax:.1f} |")
