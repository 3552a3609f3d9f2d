"""GPU checks of the input gradient of the pathwise function samples (svgp_sampler_eval_grad; csrc/sample_grad.hip, sample_api.hip)
through the C ABI, against the float64 restatement tests/pathwise_grad_ref.py (pinned by tests/test_pathwise_grad_cpu.py) on the
SAME numbers (pathwise_ref.recipe), and against the shipped value call itself.

Shapes: the smallest at which each code path can fail - d = 1, 2, 3 (one MFMA k-step), 8 and 9 (the by-differences / raw-row boundary
of fp32, and the second coordinate block of 8), 17, 33 (f64: the widest point-group form), 64 (the 4-coordinate blocks of f64); n* = 1,
17, 33, 65, 100, 129, 1000 (ragged last groups and workgroups); S = 2, 3, 5, 17 (two column blocks), 70 (five); L = 0, 1, 32, 64, 100
(padded), 1030 (33 chunks); M = 37, 64, 96, 130, 257, 300 (padded panels).  The families rotate over the table, every family in both
dtypes; Centered and NonCentered, with and without prior mean offsets.

Tolerances, per coordinate c and relative to max|G_c|: fp64 1e-8 (the project's contract); fp32 max(1e-4, 8 e32_c), e32_c the error of
the restatement's own float32 data stage on the same numbers, 1e-4 the project's fp32 contract and 8 the factor the value path started
from before it was measured.  The observed multiples are printed by the last test (profiles/sample/accuracy_grad.md)."""
import ctypes as C
import functools

import numpy as np
import pytest

import pathwise_grad_ref as pg
import pathwise_ref as pw
import svgp_oracle as o
from approxgp import _ffi
from approxgp.pathwise import draw_basis

pytestmark = pytest.mark.gpu
JITTER = 1e-3
TOL64 = 1e-8
F32_FACTOR = 8.0
STEPS = (2e-3, 1e-3)   # central-difference steps, times 1 / invl_c
FAMILIES = (o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52)
COL, ROW = _ffi.COLVECS, _ffi.ROWVECS

# (M, d, n*, S, L, centered, layout, mean_const, muz + pm)
SHAPES = [
    (37, 1, 129, 3, 1, True, COL, 0.7, False),
    (130, 2, 1000, 17, 100, False, COL, 0.0, False),
    (257, 3, 1000, 70, 1030, True, ROW, -0.4, True),
    (300, 2, 1, 70, 0, True, COL, 0.2, True),
    (64, 8, 100, 5, 64, False, COL, 0.0, False),
    (64, 9, 100, 5, 64, True, COL, 0.3, True),
    (96, 17, 65, 3, 32, False, ROW, 0.0, False),
    (64, 33, 33, 17, 32, False, COL, 0.0, False),
    (64, 64, 17, 2, 32, True, COL, 0.0, False),
]
CASES = {}
for _i, _s in enumerate(SHAPES):
    _tag = "M%d_d%d_n%d_S%d_L%d" % _s[:5]
    CASES[_tag] = _s + (FAMILIES[_i % 3],)
    CASES["f32_" + _tag] = _s + (FAMILIES[(_i + 1) % 3],)
assert {(n.startswith("f32"), c[-1]) for n, c in CASES.items()} == {(f, k) for f in (False, True) for k in FAMILIES}
F64_CASES = [n for n in CASES if not n.startswith("f32")]
OBSERVED = {}


def _dtype(name):
    return np.float32 if name.startswith("f32") else np.float64


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Everything of a case, computed once and shared read-only."""
    M, d, n, S, L, centered, layout, mc, with_mean, family = CASES[name]
    dt = _dtype(name)
    rd = lambda a: np.asarray(a, dtype=dt).astype(np.float64)
    seed = 3000 + 7 * M + 13 * d + n + S + L
    sva, muz = pw.recipe(M, d, family, seed, centered=centered, mean_const=mc, with_muz=with_mean, jitter=JITTER, dtype=dt)
    rng = np.random.default_rng(seed + 1)
    x = rd(rng.uniform(-3.0, 3.0, size=(d, n)))
    mux = rd(0.3 * np.cos(x[0])) if with_mean else None
    basis = draw_basis(family, M, L, S, rng, dt, d=d)
    omega, tau, w, eps = (a.astype(np.float64) for a in basis)
    st = pw.setup(sva, omega, tau, w, eps, muz=muz)
    G = pg.gradient(sva, st, x, omega, tau, w)
    e32 = None
    if dt == np.float32:
        G32 = pg.gradient(sva, st, x, omega, tau, w, f32=True).astype(np.float64)
        e32 = np.array([np.abs(G32[:, c] - G[:, c]).max() / np.abs(G[:, c]).max() for c in range(d)])
    for a in (x, G, st["V"]) + tuple(basis) + ((muz, mux) if with_mean else ()):
        a.setflags(write=False)
    return dict(sva=sva, muz=muz, x=x, mux=mux, basis=basis, st=st, G=G, e32=e32, wide=(omega, tau, w))


def _tolerances(name):
    p = _problem(name)
    d = CASES[name][1]
    return np.full(d, TOL64) if p["e32"] is None else np.maximum(1e-4, F32_FACTOR * p["e32"])


def _errors(G, ref):
    G, ref = np.asarray(G, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.array([np.abs(G[:, c] - ref[:, c]).max() / max(np.abs(ref[:, c]).max(), 1e-300) for c in range(ref.shape[1])])


def _model(ctx, name):
    M, d, n, S, L, centered, layout, mc, with_mean, family = CASES[name]
    p = _problem(name)
    sva = p["sva"]
    z = sva.z[0] if d == 1 else (sva.z if layout == COL else np.ascontiguousarray(sva.z.T))
    desc, keep = _ffi.make_desc(_dtype(name), sva.kernel.family, sva.kernel.variance, sva.kernel.inv_lengthscale, z, sva.m, sva.Lq,
                                sva.jitter, parametrization=_ffi.CENTERED if sva.centered else _ffi.NONCENTERED, lik_sigma2=0.1,
                                mean_const=sva.mean_const, layout_z=layout)
    model = _ffi.DeviceModel(ctx, desc, keep)
    if p["muz"] is not None:
        model.set_mean_z(p["muz"])
    return model


def _layout(name, x):
    d, layout = CASES[name][1], CASES[name][6]
    return x[0] if d == 1 else (x if layout == COL else np.ascontiguousarray(x.T))


def _data(ctx, name, x=None, y=None):
    x = _problem(name)["x"] if x is None else x
    return _ffi.DeviceData(ctx, _layout(name, x), y, _dtype(name), layout=CASES[name][6])


def _device_memory(sampler, data, off, length, prior_mean, values, ldo, ldg):
    """eval_grad into device memory -> (F buffer (S, ldo) or None, G buffer (S, d, ldg)) on the host; unwritten entries keep -777."""
    import torch

    tdt = torch.float32 if sampler.dtype == _ffi.F32 else torch.float64
    fb = torch.full((sampler.n_samples, ldo), -777.0, dtype=tdt, device="cuda") if values else None
    gb = torch.full((sampler.n_samples, sampler.d, ldg), -777.0, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    sampler.eval_grad(data, off, length, prior_mean=prior_mean, values=values, out=fb, grad_out=gb, ldo=ldo, ldg=ldg)
    return (fb.cpu().numpy() if values else None), gb.cpu().numpy()


class _Session:
    """A case's model, data and sampler on the device."""

    def __init__(self, ctx, name, x=None, y=None, basis=None):
        self.model, self.data = _model(ctx, name), _data(ctx, name, x=x, y=y)
        try:
            self.smp = self.model.sampler(_problem(name)["basis"] if basis is None else basis)
        except Exception:
            self.close()
            raise

    def close(self):
        for h in (getattr(self, "smp", None), self.model, self.data):
            if h is not None:
                h.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_restatement(ctx, name):
    M, d, n, S = CASES[name][:4]
    p = _problem(name)
    with _Session(ctx, name) as s:
        F, G = s.smp.eval_grad(s.data, prior_mean=p["mux"])
        F0 = s.smp.eval(s.data, prior_mean=p["mux"])
    assert G.shape == (S, d, n) and G.dtype == _dtype(name) and F.shape == (S, n)
    assert np.all(np.isfinite(G))
    assert np.array_equal(F, F0)                      # contract (a)
    err, tol = _errors(G, p["G"]), _tolerances(name)
    worst = int(np.argmax(err / tol))
    mult = None if p["e32"] is None else float((err / np.maximum(p["e32"], 1e-300)).max())
    OBSERVED[name] = (float(err.max()), float(tol[worst]), None if p["e32"] is None else float(p["e32"].max()), mult,
                      p["st"]["cond"], float(np.abs(p["st"]["V"]).max()))
    print(f"{name}: max_c error {err.max():.2e} of max|G_c| (tolerance {tol[worst]:.2e}), e32 {None if p['e32'] is None else p['e32'].max()}, "
          f"multiple of e32 {mult}, cond {p['st']['cond']:.1e}, max|V| {np.abs(p['st']['V']).max():.1f}")
    assert np.all(err <= tol), (err, tol)


@pytest.mark.parametrize("name", F64_CASES)
def test_gradient_is_the_derivative_of_the_value_call(ctx, name):
    """fp64 central differences of svgp_sampler_eval at two steps: the truncation error of the differences alone is left, so halving
    the step divides the error by 4.  Ties the gradient to the shipped value call without the restatement."""
    M, d, n, S = CASES[name][:4]
    p = _problem(name)
    invl = p["sva"].kernel.inv_lengthscale
    model = _model(ctx, name)
    try:
        smp = model.sampler(p["basis"])

        def f(xx):
            data = _data(ctx, name, x=xx)
            try:
                return smp.eval(data)
            finally:
                data.free()

        data = _data(ctx, name)
        G = smp.eval_grad(data, values=False)[1]
        data.free()
        ratios = []
        for c in range(d):
            scale = np.abs(G[:, c]).max()
            errs = [np.abs(pg.central_differences(f, p["x"], c, h / invl[c]) - G[:, c]).max() / scale for h in STEPS]
            ratios.append(errs[0] / errs[1])
        smp.free()
    finally:
        model.free()
    print(f"{name}: error ratios between the steps {min(ratios):.3f} .. {max(ratios):.3f}")
    assert 3.5 <= min(ratios) and max(ratios) <= 4.5, ratios


BITWISE = ["M130_d2_n1000_S17_L100", "f32_M257_d3_n1000_S70_L1030", "f32_M64_d8_n100_S5_L64", "M64_d9_n100_S5_L64", "M96_d17_n65_S3_L32",
           "f32_M64_d33_n33_S17_L32", "M64_d64_n17_S2_L32"]


@pytest.mark.parametrize("name", BITWISE)
def test_contracts_are_bitwise(ctx, name):
    """(a) values = svgp_sampler_eval's; (b) a point's gradient does not depend on the window, the call, the kind of output memory or
    whether the values were asked for; (c) svgp_elbo, svgp_sampler_eval and svgp_sampler_state are unchanged by the call."""
    M, d, n, S = CASES[name][:4]
    p = _problem(name)
    mux = p["mux"]
    cut = lambda off, ln: None if mux is None else mux[off:off + ln]
    with _Session(ctx, name, y=np.sin(p["x"][0])) as s:
        e0 = s.model.elbo(s.data)[0]
        F0 = s.smp.eval(s.data, prior_mean=mux)
        u0, V0 = s.smp.state()
        F, G = s.smp.eval_grad(s.data, prior_mean=mux)
        F2, G2 = s.smp.eval_grad(s.data, prior_mean=mux)
        _, Gonly = s.smp.eval_grad(s.data, values=False)
        assert np.array_equal(F, F0) and np.array_equal(F2, F0)
        assert np.array_equal(G, G2) and np.array_equal(G, Gonly)
        for ln in (1, 17, 129):
            ln = min(ln, n)
            for off in sorted({0, (n - ln) // 2, n - ln}):
                Fw, Gw = s.smp.eval_grad(s.data, off, ln, prior_mean=cut(off, ln))
                assert np.array_equal(Fw, F0[:, off:off + ln]), (off, ln)
                assert np.array_equal(Gw, G[:, :, off:off + ln]), (off, ln)
                assert np.array_equal(s.smp.eval_grad(s.data, off, ln, values=False)[1], Gw), (off, ln)
        # host rows further apart than the window
        Fl, Gl = s.smp.eval_grad(s.data, prior_mean=mux, ldo=n + 3, ldg=n + 2)
        assert np.array_equal(Fl[:, :n], F0) and np.all(Fl[:, n:] == 0) and np.array_equal(Gl[:, :, :n], G) and np.all(Gl[:, :, n:] == 0)
        # device memory, rows further apart than the window; nothing beyond the window is written
        ln = min(129, n)
        off = n - ln
        Fd, Gd = _device_memory(s.smp, s.data, off, ln, cut(off, ln), True, ln + 5, ln + 7)
        assert np.array_equal(Fd[:, :ln], F0[:, off:]) and np.all(Fd[:, ln:] == -777.0)
        assert np.array_equal(Gd[:, :, :ln], G[:, :, off:]) and np.all(Gd[:, :, ln:] == -777.0)
        _, Gd = _device_memory(s.smp, s.data, 0, n, None, False, n, n)
        assert np.array_equal(Gd, G)
        # (c)
        assert s.model.elbo(s.data)[0] == e0
        assert np.array_equal(s.smp.eval(s.data, prior_mean=mux), F0)
        u1, V1 = s.smp.state()
        assert np.array_equal(u0, u1) and np.array_equal(V0, V1)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][-1] != o.KERNEL_SE and CASES[n][0] <= 130 and CASES[n][1] in (1, 2, 8, 9, 17)])
def test_at_the_inducing_points(ctx, name):
    """x equal to inducing points: r = 0 in one term of every point.  Finite, and inside the case's band."""
    p = _problem(name)
    sva = p["sva"]
    omega, tau, w = p["wide"]
    x = np.array(sva.z)
    ref = pg.gradient(sva, p["st"], x, omega, tau, w)
    if p["e32"] is None:
        tol = np.full(x.shape[0], TOL64)
    else:
        G32 = pg.gradient(sva, p["st"], x, omega, tau, w, f32=True).astype(np.float64)
        tol = np.maximum(1e-4, F32_FACTOR * _errors(G32, ref))
    with _Session(ctx, name, x=x) as s:
        G = s.smp.eval_grad(s.data, values=False)[1]
    assert np.all(np.isfinite(G))
    err = _errors(G, ref)
    print(f"{name} at x = z: max_c error {err.max():.2e} (tolerance {tol.min():.2e} ..)")
    assert np.all(err <= tol), (err, tol)


@pytest.mark.parametrize("name", ["M300_d2_n1_S70_L0", "M130_d2_n1000_S17_L100", "M64_d9_n100_S5_L64"])
def test_no_features_and_no_noise_is_the_gradient_of_the_predicted_mean(ctx, name):
    """L = 0 and eps = 0: the gradient of svgp_predict's mean, by the ratio test on its central differences (fp64)."""
    M, d, n = CASES[name][:3]
    layout = CASES[name][6]
    p = _problem(name)
    invl = p["sva"].kernel.inv_lengthscale
    zero = (np.zeros((0, d)), np.zeros(0), np.zeros((2, 0)), np.zeros((2, M)))
    with _Session(ctx, name, basis=zero) as s:
        G = s.smp.eval_grad(s.data, values=False)[1].astype(np.float64)
        f = lambda xx: s.model.predict(_layout(name, xx), True, False, False, layout=layout)[0].astype(np.float64)[None, :]
        ratios, small = [], []
        for c in range(d):
            scale = np.abs(G[:1, c]).max()
            errs = [np.abs(pg.central_differences(f, p["x"], c, h / invl[c]) - G[:1, c]).max() / scale for h in STEPS]
            ratios.append(errs[0] / errs[1])
            small.append(errs[1])
    assert np.array_equal(G[0], G[1])
    print(f"{name}: error ratios {min(ratios):.3f} .. {max(ratios):.3f}, smaller error <= {max(small):.2e}")
    assert 3.5 <= min(ratios) and max(ratios) <= 4.5, ratios


def test_statuses_then_a_healthy_call(ctx):
    name = "M37_d1_n129_S3_L1"
    p = _problem(name)
    lib, ptr = ctx.lib, _ffi._ptr
    other_d = _ffi.DeviceData(ctx, np.zeros((2, 5)), None, np.float64)
    other_t = _ffi.DeviceData(ctx, np.zeros(5), None, np.float32)
    try:
        with _Session(ctx, name) as s:
            F0 = s.smp.eval(s.data)
            G0 = s.smp.eval_grad(s.data, values=False)[1]
            out, grad = np.zeros((3, 129)), np.zeros((3, 1, 129))
            bad_pm = _ffi.PointMean()
            call = lambda d_, off, n, ldo, ldg, o_=out, g_=grad, pm=None, dev=0: lib.svgp_sampler_eval_grad(
                ctx.h, s.smp.h, d_.h, off, n, pm, ptr(o_), ldo, ptr(g_), ldg, dev)
            assert call(other_d, 0, 5, 5, 5) == _ffi.INVALID_ARG            # d mismatch
            assert call(other_t, 0, 5, 5, 5) == _ffi.INVALID_ARG            # dtype mismatch
            assert call(s.data, 0, 0, 129, 129) == _ffi.INVALID_ARG         # empty window
            assert call(s.data, 100, 30, 129, 129) == _ffi.INVALID_ARG      # window past the data
            assert call(s.data, -1, 5, 129, 129) == _ffi.INVALID_ARG
            assert call(s.data, 0, 129, 128, 129) == _ffi.INVALID_ARG       # ldo < len
            assert call(s.data, 0, 129, 129, 128) == _ffi.INVALID_ARG       # ldg < len
            assert call(s.data, 0, 129, 129, 129, g_=None) == _ffi.INVALID_ARG   # NULL grad_out
            assert call(s.data, 0, 129, 129, 129, dev=2) == _ffi.INVALID_ARG
            assert lib.svgp_sampler_eval_grad(ctx.h, None, s.data.h, 0, 129, None, ptr(out), 129, ptr(grad), 129, 0) == _ffi.INVALID_ARG
            assert lib.svgp_sampler_eval_grad(ctx.h, s.smp.h, None, 0, 129, None, ptr(out), 129, ptr(grad), 129, 0) == _ffi.INVALID_ARG
            # what svgp_sampler_eval rejects in pm is rejected here as well: the same call, side by side
            rc_eval = lib.svgp_sampler_eval(ctx.h, s.smp.h, s.data.h, 0, 129, C.byref(bad_pm), ptr(out), 129, 0)
            rc_grad = call(s.data, 0, 129, 129, 129, pm=C.byref(bad_pm))
            assert rc_eval == _ffi.INVALID_ARG and rc_grad == _ffi.INVALID_ARG   # NULL offsets
            bad_pm = _ffi.PointMean(ptr(np.zeros(129)), 2, 0)
            assert call(s.data, 0, 129, 129, 129, pm=C.byref(bad_pm)) == _ffi.INVALID_ARG   # on_device neither 0 nor 1
            assert np.all(out == 0.0) and np.all(grad == 0.0)
            # a NULL out is no error, and ldo is then not read
            assert call(s.data, 0, 129, 0, 129, o_=None) == _ffi.OK
            assert np.array_equal(grad, G0)
            # non-finite inputs: non-finite outputs, SVGP_OK
            xn = p["x"].copy()
            xn[0, 3] = np.nan
            dn = _data(ctx, name, x=xn)
            Fn, Gn = s.smp.eval_grad(dn)
            dn.free()
            assert np.all(np.isnan(Gn[:, :, 3])) and np.all(np.isfinite(np.delete(Gn, 3, axis=2))) and np.all(np.isnan(Fn[:, 3]))
            # ... and the same context, model and sampler are healthy
            F, G = s.smp.eval_grad(s.data)
    finally:
        other_d.free()
        other_t.free()
    assert np.array_equal(F, F0) and np.array_equal(G, G0)
    assert np.all(_errors(G, p["G"]) <= TOL64)


@pytest.mark.parametrize("name", ["M130_d2_n1000_S17_L100", "f32_M64_d9_n100_S5_L64"])
def test_a_sampler_outlives_its_model(ctx, name):
    p = _problem(name)
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        smp = model.sampler(p["basis"])
        F, G = smp.eval_grad(data, prior_mean=p["mux"])
        model.free()
        F1, G1 = smp.eval_grad(data, prior_mean=p["mux"])
        smp.free()
    finally:
        model.free()
        data.free()
    assert np.array_equal(F, F1) and np.array_equal(G, G1)


def test_python_mirror(ctx):
    """FunctionSamples.grad / value_and_grad: shapes (n, S, d), and the values are fs(x)'s."""
    import approxgp as ag

    rng = np.random.default_rng(5)
    M = 20
    z = np.linspace(-1, 1, M)
    f = ag.GP(1.3 * ag.with_lengthscale(ag.SqExponentialKernel(), 0.3))
    m, Lq = 0.5 * rng.standard_normal(M), np.tril(0.1 * rng.standard_normal((M, M))) + 0.5 * np.eye(M)
    post = ag.posterior(ag.SparseVariationalApproximation(f(z, 1e-3), ag.MvNormal.from_cholesky(m, Lq)), ctx=ctx)
    fs = post.function_samples(3, n_features=64, rng=rng)
    x = rng.uniform(-1, 1, 60)
    try:
        F = fs(x)
        F1, G = fs.value_and_grad(x)
        G1 = fs.grad(x)
    finally:
        fs.free()
    assert F1.shape == (60, 3) and G.shape == (60, 3, 1)
    assert np.array_equal(F, F1) and np.array_equal(G, G1) and np.all(np.isfinite(G))


def test_report_observed_errors():
    """Prints the table profiles/sample/accuracy_grad.md records (run the module with -s)."""
    for name, (err, tol, e32, mult, cond, vmax) in OBSERVED.items():
        print(f"| {name} | {err:.2e} | {tol:.2e} | {'-' if e32 is None else format(e32, '.2e')} | {'-' if mult is None else format(mult, '.2f')} | {cond:.1e} | {vmax:.1f} |")
