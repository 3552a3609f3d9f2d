"""GPU checks of the Laplace approximation (csrc/laplace.hip, svgp_laplace_*) against the float64 reference of tests/laplace_ref.py
(itself pinned to the reference package's Laplace optimum and to finite differences in tests/test_laplace_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import minimize

import laplace_ref as lr
import svgp_oracle as o
from approxgp import (GP, BernoulliLikelihood, DeviceLaplace, GaussianLikelihood, LaplaceApproximation, LatentGP, SEKernel,
                      _ffi, approx_lml, approx_lml_and_gradient, build_laplace_objective, posterior, with_lengthscale)
from approxgp.gp import ExponentialLikelihood, GammaLikelihood, NormalCDFLink, PoissonLikelihood
from approxgp.kernels import Matern32Kernel, Matern52Kernel, ARDTransform, ScaledKernel, TransformedKernel
from test_reference_literal_pin import LBFGS, NELDER_MEAD, X, Y

pytestmark = pytest.mark.gpu

BASES = {o.KERNEL_SE: SEKernel, o.KERNEL_MATERN32: Matern32Kernel, o.KERNEL_MATERN52: Matern52Kernel}


def _lik(code, s2):
    return {0: lambda: GaussianLikelihood(s2), 1: lambda: BernoulliLikelihood(), 2: lambda: PoissonLikelihood(),
            3: lambda: ExponentialLikelihood(), 4: lambda: GammaLikelihood(s2), 5: lambda: BernoulliLikelihood(NormalCDFLink())}[code]()


def _kernel(family, var, il):
    return ScaledKernel(TransformedKernel(BASES[family](), ARDTransform(np.asarray(il, dtype=np.float64))), var)


def _s2(lik):
    return 0.3 if lik == 0 else (2.0 if lik == 4 else 1.0)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _dev(ctx, x, y, dtype, layout):
    if layout == _ffi.ROWVECS:
        return DeviceLaplace(ctx, np.asarray(x).T, y, dtype, layout=_ffi.ROWVECS)
    if layout == _ffi.VEC:
        return DeviceLaplace(ctx, np.asarray(x)[0], y, dtype)
    return DeviceLaplace(ctx, x, y, dtype)


def test_reference_pin_with_device_value_and_gradient(ctx):
    """test/LaplaceApproximationModule.jl:150-176: the optimum of approx_lml over theta, reached with the device's f64 value
    and gradient (softplus variance and lengthscale, jitter 1e-8)."""
    dev = DeviceLaplace(ctx, X, Y, np.float64)

    def fg(theta):
        v, l = o.softplus(theta[0]), o.softplus(theta[1])
        desc, keep = dev.desc(_kernel(o.KERNEL_SE, v, [1.0 / l]), BernoulliLikelihood(), 1e-8)
        lml, dv, dil, _ = dev.lml_grad(desc)
        sig = 1.0 / (1.0 + np.exp(-np.asarray(theta)))
        return -lml, -np.array([dv * sig[0], float(np.sum(dil)) * (-1.0 / l ** 2) * sig[1]])

    res = minimize(fg, np.array([5.0, 1.0]), jac=True, method="L-BFGS-B", options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 500})
    dev.free()
    np.testing.assert_allclose(res.x, LBFGS, rtol=1e-6)
    np.testing.assert_allclose(res.x, NELDER_MEAD, rtol=1e-4)


def _cases():
    """A seeded selection covering every likelihood, kernel family, isotropic / ARD, layout, dtype and N in the list."""
    rng = np.random.default_rng(7)
    ns = [1, 37, 128, 129, 1000, 2048]
    cases = []
    for i in range(18):
        lik = i % 6
        fam = (i // 6 + i) % 3
        cases.append((lik, fam, bool(i % 2), [_ffi.COLVECS, _ffi.ROWVECS, _ffi.VEC][i % 3], [np.float64, np.float32][(i // 3) % 2],
                      ns[i % 6] if i < 12 else int(rng.choice(ns[:5]))))
    return cases


@pytest.mark.parametrize("lik,fam,ard,layout,dtype,n", _cases())
def test_parity_with_reference(ctx, lik, fam, ard, layout, dtype, n):
    d = 1 if layout == _ffi.VEC else 3
    x, y = lr.synth(lik, n, d, seed=100 + n + lik)
    il = np.array([0.7, 1.3, 0.9][:d]) if ard else np.full(d, 0.8)
    s2 = _s2(lik)
    x = x.astype(dtype)
    y = y.astype(dtype)
    eps = np.finfo(dtype).eps
    ref, cache, it_ref, conv_ref = lr.fit(lr.kernel_of(fam, 1.2, il), x, y, lik, s2, jitter=1e-6, eps=eps)
    dev = _dev(ctx, x, y, dtype, layout)
    desc, keep = dev.desc(_kernel(fam, 1.2, il), _lik(lik, s2), 1e-6)
    lml, info = dev.fit(desc)
    f, g, w = dev.mode()
    dev.free()
    assert np.isfinite(lml)
    if dtype == np.float32:
        assert abs(lml - ref) <= 1e-4 * abs(ref), (lml, ref)
    elif info.iterations == it_ref:
        assert abs(lml - ref) <= 1e-10 * abs(ref), (lml, ref)
        assert np.max(np.abs(f - cache["f"])) <= 1e-7 * max(np.max(np.abs(cache["f"])), 1e-300)
    else:
        assert abs(info.iterations - it_ref) == 1
        assert abs(lml - ref) <= 1e-7 * abs(ref), (lml, ref)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_maxiter_one_keeps_fnew(ctx, dtype):
    x, y = lr.synth(1, 200, 2, seed=3)
    ref, cache, it, conv = lr.fit(lr.kernel_of(0, 1.5, [0.8, 0.8]), x, y, 1, jitter=1e-6, maxiter=1, eps=np.finfo(dtype).eps)
    dev = _dev(ctx, x.astype(dtype), y.astype(dtype), dtype, _ffi.COLVECS)
    desc, keep = dev.desc(_kernel(0, 1.5, [0.8, 0.8]), BernoulliLikelihood(), 1e-6, maxiter=1)
    lml, info = dev.fit(desc)
    f, _, _ = dev.mode()
    dev.free()
    assert info.iterations == 1 and not info.converged and not conv
    tol = 1e-10 if dtype == np.float64 else 1e-4
    assert abs(lml - ref) <= tol * abs(ref)
    assert np.max(np.abs(f - cache["f"])) <= (1e-9 if dtype == np.float64 else 1e-4) * np.max(np.abs(cache["f"]))


def test_conjugate_case_is_the_exact_gp(ctx):
    """Gaussian likelihood: the Laplace lml is the exact GP log marginal likelihood, its predictions the exact posterior's."""
    x, y = lr.synth(0, 300, 2, seed=5)
    s2, il = 0.05, np.array([0.9, 1.1])
    k = lr.kernel_of(o.KERNEL_MATERN52, 1.4, il)
    K = o.kernelmatrix(k, x) + 1e-6 * np.eye(300)
    C_ = K + s2 * np.eye(300)
    Lc = np.linalg.cholesky(C_)
    alpha = np.linalg.solve(C_, y)
    exact = -0.5 * y @ alpha - np.sum(np.log(np.diag(Lc))) - 150 * np.log(2 * np.pi)
    dev = DeviceLaplace(ctx, x, y, np.float64)
    desc, keep = dev.desc(_kernel(o.KERNEL_MATERN52, 1.4, il), GaussianLikelihood(s2), 1e-6)
    lml, _ = dev.fit(desc)
    xs = np.random.default_rng(1).uniform(-2, 2, size=(2, 50))
    m, v, _ = dev.predict(xs)
    dev.free()
    assert abs(lml - exact) <= 1e-10 * abs(exact), (lml, exact)
    ks = o.kernelmatrix(k, x, xs)
    np.testing.assert_allclose(m, ks.T @ alpha, rtol=0, atol=1e-9 * np.max(np.abs(m)))
    v_ex = 1.4 - np.sum(ks * np.linalg.solve(C_, ks), axis=0)
    np.testing.assert_allclose(v, v_ex, rtol=0, atol=1e-9)


@pytest.mark.parametrize("lik,fam", [(1, 0), (2, 1), (5, 2), (4, 0), (3, 2)])
def test_gradient(ctx, lik, fam):
    x, y = lr.synth(lik, 150, 2, seed=20 + lik)
    s2, var, il = _s2(lik), 1.1, np.array([0.8, 1.3])
    lik_o = _lik(lik, s2)
    dev = DeviceLaplace(ctx, x, y, np.float64)

    def grad(v, l, dv=dev):
        desc, keep = dv.desc(_kernel(fam, v, l), lik_o, 1e-6, maxiter=200)
        return dv.lml_grad(desc)

    lml, gv, gil, _ = grad(var, il)
    val = lambda v, l: grad(v, l)[0]
    h = 1e-5   # the Newton stop leaves ~1e-10 of noise in the lml: differences of the reference at this h agree to ~5e-10
    fd = np.array([(val(var + h, il) - val(var - h, il)) / (2 * h)] +
                  [(val(var, il + h * e) - val(var, il - h * e)) / (2 * h) for e in np.eye(2)])
    g = np.concatenate([[gv], gil])
    _, rv, ril = lr.lml_grad(lr.kernel_of(fam, var, il), x, y, lik, s2, jitter=1e-6, maxiter=200)
    scale = np.max(np.abs(g))
    assert np.max(np.abs(g - np.concatenate([[rv], ril]))) <= 1e-6 * scale
    assert np.max(np.abs(g - fd)) <= 1e-6 * scale, (g, fd)
    dev32 = DeviceLaplace(ctx, x.astype(np.float32), y.astype(np.float32), np.float32)
    _, gv32, gil32, _ = grad(var, il, dev32)
    dev32.free()
    dev.free()
    assert np.max(np.abs(np.concatenate([[gv32], gil32]) - g)) <= 1e-3 * scale


def test_gradient_stays_finite_where_w_vanishes(ctx):
    """Exponential likelihood with y = 0 at some points: W = y exp(-f) is exactly 0 there for every f.  Nothing may divide by
    sqrt(W) (the reference's rrule does): the value and the gradient stay finite and match the reference's closed form."""
    x, y = lr.synth(3, 120, 2, seed=4)
    y[::7] = 0.0
    il = np.array([0.9, 1.2])
    dev = DeviceLaplace(ctx, x, y, np.float64)
    desc, keep = dev.desc(_kernel(o.KERNEL_MATERN52, 1.3, il), ExponentialLikelihood(), 1e-6)
    lml, gv, gil, _ = dev.lml_grad(desc)
    _, _, w = dev.mode()
    dev.free()
    assert np.any(w == 0.0) and np.all(w[y == 0] == 0.0)
    assert np.isfinite(lml) and np.isfinite(gv) and np.all(np.isfinite(gil))
    ref, rv, ril = lr.lml_grad(lr.kernel_of(o.KERNEL_MATERN52, 1.3, il), x, y, o.LIK_EXPONENTIAL_EXP, jitter=1e-6)
    g, gr = np.concatenate([[gv], gil]), np.concatenate([[rv], ril])
    assert abs(lml - ref) <= 1e-10 * abs(ref)
    assert np.max(np.abs(g - gr)) <= 1e-6 * np.max(np.abs(gr))


def test_warm_start(ctx):
    x, y = lr.synth(1, 500, 2, seed=9)
    obj = build_laplace_objective(lambda t: LatentGP(GP(_kernel(0, t[0], [t[1], t[1]])), BernoulliLikelihood(), 1e-8), x, y,
                                  ctx=ctx)
    v1 = obj([1.5, 0.9])
    it1 = obj.last_info.iterations
    v2 = obj([1.5, 0.9])
    it2 = obj.last_info.iterations
    cold = build_laplace_objective(lambda t: LatentGP(GP(_kernel(0, t[0], [t[1], t[1]])), BernoulliLikelihood(), 1e-8), x, y,
                                   newton_warmstart=False, ctx=ctx)
    cold([1.5, 0.9])
    v3 = cold([1.5, 0.9])
    assert cold.last_info.iterations == it1
    obj.free()
    cold.free()
    assert it2 < it1
    assert abs(v2 - v1) <= 1e-7 * abs(v1) and abs(v3 - v1) <= 1e-12 * abs(v1)


def test_predictions(ctx):
    x, y = lr.synth(5, 500, 2, seed=11)
    xs = np.random.default_rng(2).uniform(-2, 2, size=(2, 300))
    ys = np.random.default_rng(3).uniform(-2, 2, size=(2, 120))
    il = np.array([0.8, 1.2])
    lf = LatentGP(GP(_kernel(o.KERNEL_MATERN32, 1.3, il)), BernoulliLikelihood(NormalCDFLink()), 1e-6)
    post = posterior(LaplaceApproximation(), lf(x), y, ctx=ctx)
    m, v = post.mean_and_var(xs)
    c = post.cov(xs)
    cx = post.cov(xs, ys)
    m2, c2 = post.mean_and_cov(xs)
    _, cache, _, _ = lr.fit(lr.kernel_of(o.KERNEL_MATERN32, 1.3, il), x, y, 5, jitter=1e-6)
    rm, rv, rc = lr.predict(cache, lr.kernel_of(o.KERNEL_MATERN32, 1.3, il), x, xs)
    _, _, rcx = lr.predict(cache, lr.kernel_of(o.KERNEL_MATERN32, 1.3, il), x, xs, ys)
    post.dev.free()
    tol = 1e-9
    np.testing.assert_allclose(m, rm, rtol=0, atol=tol * np.max(np.abs(rm)))
    np.testing.assert_allclose(v, rv, rtol=0, atol=tol)
    np.testing.assert_allclose(c, rc, rtol=0, atol=tol)
    np.testing.assert_allclose(cx, rcx, rtol=0, atol=tol)
    np.testing.assert_allclose(np.diag(c), v, rtol=0, atol=1e-12)
    assert np.array_equal(m2, m) and np.array_equal(c2, c)
    assert np.max(np.abs(c - c.T)) <= 1e-12


def test_argument_errors(ctx):
    x, y = lr.synth(1, 64, 2, seed=1)
    dev = DeviceLaplace(ctx, x, y, np.float64)
    lib = ctx.lib
    lml, info = C.c_double(), _ffi.LaplaceInfo()
    good, keep = dev.desc(_kernel(0, 1.0, [1.0, 1.0]), BernoulliLikelihood(), 1e-6)

    def status(**kw):
        ds, keep2 = dev.desc(_kernel(0, 1.0, [1.0, 1.0]), BernoulliLikelihood(), 1e-6)
        for k_, v_ in kw.items():
            setattr(ds, k_, v_)
        return lib.svgp_laplace_fit(ctx.h, dev.h, C.byref(ds), None, C.byref(lml), C.byref(info))

    assert status(maxiter=0) == _ffi.INVALID_ARG
    assert status(jitter=-1.0) == _ffi.INVALID_ARG
    assert status(variance=0.0) == _ffi.INVALID_ARG
    assert status(reserved=1) == _ffi.INVALID_ARG
    assert status(warm_start=2) == _ffi.INVALID_ARG
    assert status(d=3) == _ffi.INVALID_ARG
    assert status(dtype=_ffi.F32) == _ffi.INVALID_ARG
    assert lib.svgp_laplace_fit(ctx.h, dev.h, None, None, C.byref(lml), None) == _ffi.INVALID_ARG
    assert lib.svgp_laplace_fit(ctx.h, dev.h, C.byref(good), None, None, None) == _ffi.INVALID_ARG
    assert lib.svgp_laplace_mode(ctx.h, dev.h, None, None, None) == _ffi.INVALID_ARG   # no fit yet
    h = C.c_void_p()
    nodata = _ffi.DeviceData(ctx, x, None, np.float64)
    assert lib.svgp_laplace_create(ctx.h, nodata.h, C.byref(h)) == _ffi.INVALID_ARG
    nodata.free()
    big = _ffi.DeviceData(ctx, np.zeros(8193), np.zeros(8193), np.float64)
    assert lib.svgp_laplace_create(ctx.h, big.h, C.byref(h)) == _ffi.UNSUPPORTED
    big.free()
    # a healthy fit on the same context afterwards
    val, info2 = dev.fit(good)
    dev.free()
    ref = lr.fit(lr.kernel_of(0, 1.0, [1.0, 1.0]), x, y, 1, jitter=1e-6)[0]
    assert abs(val - ref) <= 1e-9 * abs(ref)


def test_top_size(ctx):
    """N = 8192: fp64 against the reference once, fp32 against fp64.  The reference starts from the device's mode: one host
    Newton step confirms it is the reference's fixed point (isapprox holds at once) and gives the lml there - two host
    factorisations instead of a whole host Newton run."""
    n = 8192
    x, y = lr.synth(1, n, 8, seed=12)
    il = np.full(8, 0.5)
    vals = {}
    for dt in (np.float64, np.float32):
        dev = DeviceLaplace(ctx, x.astype(dt), y.astype(dt), dt)
        desc, keep = dev.desc(_kernel(0, 1.0, il), BernoulliLikelihood(), 1e-6)
        vals[dt], info = dev.fit(desc)
        assert info.converged
        if dt == np.float64:
            f64_mode = dev.mode()[0]
        dev.free()
        assert np.isfinite(vals[dt])
    ref, _, it, conv = lr.fit(lr.kernel_of(0, 1.0, il), x, y, 1, jitter=1e-6, f_init=f64_mode)
    assert it == 1 and conv
    assert abs(vals[np.float64] - ref) <= 1e-10 * abs(ref)
    assert abs(vals[np.float32] - vals[np.float64]) <= 1e-4 * abs(vals[np.float64])


def test_fp32_top_size(ctx):
    n = 16384
    x, y = lr.synth(1, n, 8, seed=13)
    dev = DeviceLaplace(ctx, x.astype(np.float32), y.astype(np.float32), np.float32)
    desc, keep = dev.desc(_kernel(0, 1.0, np.full(8, 0.5)), BernoulliLikelihood(), 1e-6)
    lml, info = dev.fit(desc)
    dev.free()
    assert np.isfinite(lml) and info.converged


def test_approx_lml_dispatch(ctx):
    lf = LatentGP(GP(_kernel(0, 2.0, [0.7])), BernoulliLikelihood(), 1e-8)
    v = approx_lml(LaplaceApproximation(), lf(X), Y, ctx=ctx)
    v2, g = approx_lml_and_gradient(LaplaceApproximation(), lf(X), Y, ctx=ctx)
    ref, rv, ril = lr.lml_grad(lr.kernel_of(0, 2.0, [0.7]), X, Y, 1, jitter=1e-8)
    assert abs(v - ref) <= 1e-10 * abs(ref) and v2 == v
    np.testing.assert_allclose(g["inv_lengthscale"], ril, rtol=1e-6)
    assert abs(g["variance"] - rv) <= 1e-6 * abs(rv)
