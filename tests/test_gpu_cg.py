"""GPU checks of the exact GP by matrix-free conjugate gradients (csrc/cg.hip, cg_api.hip; svgp_cg_*) against dense numpy and the
float64 restatement tests/cg_ref.py (itself pinned to the oracle's exact GP and to central differences in tests/test_cg_cpu.py).
Inputs are seeded: x ~ U[-3, 3]^d, lengthscale 0.7, variance 1.3.

Bounds.  matvec, fp64: error <= 1e-12 max_i sum_j |Khat_ij V_js|, the N eps forward bound at N = 1000 (1.1e-13) with a tenfold margin
for the expansion form of r^2.  matvec, fp32: at most 4 x the error of cg_ref's float32 chain on the same case, both measured against
the float64 product of the float32-rounded inputs (summation order, kexp's 2 ulp).  solve: converged, reported residual <= tol and
|x - x*| / |x*| <= cond(Khat) tol with cond computed here.  lml / gradient / predictions: the project's parity contracts, 1e-8
relative in fp64 and 1e-4 in fp32.  The shifted fp32 case (d = 9, x + 30) bounds the lengthscale block by 4 x the float32 restatement's
own error.  test_report_observed_errors prints every measured figure (profiles/cg/accuracy.md records a run on an MI355X)."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import cg_ref as cr
import svgp_oracle as o
from approxgp import (GP, ConjugateGradients, CustomMean, DeviceConjugateGradients, SEKernel, _ffi, approx_lml, approx_lml_and_gradient,
                      draw_probes, posterior)
from approxgp.kernels import ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, TransformedKernel

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
SE, M32, M52 = o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52
FAMILIES = [SE, M32, M52]
BASES = {SE: SEKernel, M32: Matern32Kernel, M52: Matern52Kernel}
VAR, LS = 1.3, 0.7
OBSERVED = {}   # name -> text of the measured figures (printed by the last test)


def _kernel(family, d):
    return ScaledKernel(TransformedKernel(BASES[family](), ARDTransform(np.full(d, 1.0 / LS))), VAR)


def _okernel(family, d, dtype=F64):
    il = np.full(d, 1.0 / LS).astype(dtype).astype(F64)
    return o.Kernel(family, float(dtype(VAR)), il)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _xy(N, d, seed=0, shift=0.0):
    rng = np.random.default_rng(1000 + 7 * N + 13 * d + seed)
    x = rng.uniform(-3, 3, size=(d, N)) + shift
    y = np.sin(x.sum(0) - d * shift) + 0.1 * rng.standard_normal(N)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _dev(ctx, x, y, dtype, layout=_ffi.COLVECS):
    if x.shape[0] == 1 and layout == _ffi.VEC:
        return DeviceConjugateGradients(ctx, x[0], y, dtype)
    if layout == _ffi.ROWVECS:
        return DeviceConjugateGradients(ctx, np.ascontiguousarray(x.T), y, dtype, layout=_ffi.ROWVECS)
    return DeviceConjugateGradients(ctx, x, y, dtype)


# ---- 1. matvec ----------------------------------------------------------------------------------------------------------------------
NS = [1, 17, 63, 65, 257, 1000]
SS = [1, 16, 17, 64, 65, 130]
DS = [1, 8, 9, 17, 33, 64]


def _matvec_cases():
    """36 cases, a Latin square: every (N, S), (N, d) and (S, d) pair of the three lists occurs; families, dtypes and layouts rotate"""
    cases = []
    for i in range(6):
        for j in range(6):
            N, S, d = NS[i], SS[j], DS[(i + j) % 6]
            family = FAMILIES[(i + 2 * j) % 3]
            dtype = [F64, F32][(i + j // 2) % 2]
            layout = _ffi.VEC if d == 1 and (i % 2) else [_ffi.COLVECS, _ffi.ROWVECS][(i + j) % 2]
            cases.append(pytest.param(N, S, d, family, dtype, layout, id=f"N{N}_S{S}_d{d}_k{family}_{np.dtype(dtype).name}_l{layout}"))
    return cases


@pytest.mark.parametrize("N,S,d,family,dtype,layout", _matvec_cases())
def test_matvec_against_dense(ctx, N, S, d, family, dtype, layout):
    x, y = _xy(N, d)
    x = x.astype(dtype)
    V = np.asfortranarray(np.random.default_rng(N + S + d).standard_normal((N, S)).astype(dtype))
    diag = 0.1
    dev = _dev(ctx, x, None, dtype, layout)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, tol=1e-8, maxiter=10)
        out = dev.matvec(desc, V)
        again = dev.matvec(desc, V)
        Vt = torch.from_numpy(np.ascontiguousarray(V.T)).cuda()
        ot = torch.empty_like(Vt)
        torch.cuda.synchronize()
        dev.matvec(desc, Vt, out=ot)
        on_dev = ot.cpu().numpy().T
    finally:
        dev.free()
    assert out.dtype == dtype and np.array_equal(out, again), "two calls differ"
    assert np.array_equal(out, on_dev), "host and device-memory outputs differ"
    ok = _okernel(family, d, dtype)
    Kh = cr.khat(ok, x.astype(F64), float(dtype(diag)))
    ref = Kh @ V.astype(F64)
    err = float(np.abs(out.astype(F64) - ref).max())
    scale = float((np.abs(Kh) @ np.abs(V.astype(F64))).max())
    name = f"matvec N{N} S{S} d{d} k{family} {np.dtype(dtype).name}"
    if dtype == F64:
        OBSERVED[name] = f"error {err:.2e}, bound {1e-12 * scale:.2e}"
        print(name, OBSERVED[name])
        assert err <= 1e-12 * scale, (err, scale)
    else:
        e_ref = float(np.abs(cr.kmv_f32(ok, x, V, diag).astype(F64) - ref).max())
        OBSERVED[name] = f"error {err:.2e}, float32 chain {e_ref:.2e}, ratio {err / max(e_ref, 1e-300):.2f}"
        print(name, OBSERVED[name])
        assert err <= 4.0 * e_ref, (err, e_ref)


# ---- 2. solve -----------------------------------------------------------------------------------------------------------------------
SOLVE_CASES = [(48, 1, 0.1), (300, 2, 0.1), (300, 2, 0.01)]


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,d,diag", SOLVE_CASES)
def test_solve_against_dense(ctx, N, d, diag, family, dtype):
    x, y = _xy(N, d)
    x = x.astype(dtype)
    B = np.asfortranarray(np.column_stack([y, np.random.default_rng(3).standard_normal((N, 2))]).astype(dtype))
    tol = 1e-10 if dtype == F64 else 1e-5
    dev = _dev(ctx, x, None, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, tol=tol, maxiter=2000)
        X, iters, rel, info = dev.solve(desc, B)
    finally:
        dev.free()
    Kh = cr.khat(_okernel(family, d, dtype), x.astype(F64), float(dtype(diag)))
    ref = np.linalg.solve(Kh, B.astype(F64))
    cond = np.linalg.cond(Kh)
    err = np.linalg.norm(X.astype(F64) - ref, axis=0) / np.linalg.norm(ref, axis=0)
    name = f"solve N{N} d{d} diag{diag} k{family} {np.dtype(dtype).name}"
    OBSERVED[name] = f"iterations {iters.max()}, residual {rel.max():.2e}, error {err.max():.2e}, cond tol {cond * tol:.2e}"
    print(name, OBSERVED[name])
    assert info.converged == 1 and info.n_unconverged == 0 and info.iterations == iters.max()
    assert rel.max() <= tol and info.max_rel_residual == rel.max()
    assert err.max() <= cond * tol, (err, cond)


# ---- 3. column independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_columns_do_not_depend_on_their_neighbours(ctx, dtype):
    N, d = 300, 2
    x, y = _xy(N, d)
    B = np.asfortranarray(np.random.default_rng(9).standard_normal((N, 70)).astype(dtype))
    B[:, 5] = 0
    dev = _dev(ctx, x.astype(dtype), None, dtype)
    try:
        desc, keep = dev.desc(_kernel(M32, d), 0.1, tol=1e-10 if dtype == F64 else 1e-5, maxiter=2000)
        X, iters, rel, info = dev.solve(desc, B)
        X2, iters2, rel2, _ = dev.solve(desc, B)
        X0, it0, rel0, _ = dev.solve(desc, B[:, :1])
        X66, it66, rel66, _ = dev.solve(desc, B[:, 66:67])
    finally:
        dev.free()
    assert np.array_equal(X, X2) and np.array_equal(iters, iters2) and np.array_equal(rel, rel2)
    assert np.array_equal(X[:, 0], X0[:, 0]) and iters[0] == it0[0] and rel[0] == rel0[0]
    assert np.array_equal(X[:, 66], X66[:, 0]) and iters[66] == it66[0] and rel[66] == rel66[0]
    assert iters[5] == 0 and not X[:, 5].any() and rel[5] == 0 and info.converged == 1
    assert len(set(iters.tolist())) > 1   # the columns did stop at different iterations


# ---- 4. - 6. lml and gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
def test_lml_with_unit_probes_is_the_exact_gp(ctx, family, dtype):
    N = 48
    x, y = _xy(N, 1)
    x, y = x.astype(dtype), y.astype(dtype)
    dev = _dev(ctx, x, y, dtype, _ffi.VEC)
    try:
        desc, keep = dev.desc(_kernel(family, 1), 0.1, tol=1e-12 if dtype == F64 else 1e-5, maxiter=2000)
        lml, info = dev.fit(desc, cr.unit_probes(N))
    finally:
        dev.free()
    ref = o.exact_gp_logpdf(_okernel(family, 1, dtype), x.astype(F64), float(dtype(0.1)), y.astype(F64))
    err = abs(lml - ref) / abs(ref)
    OBSERVED[f"lml unit probes k{family} {np.dtype(dtype).name}"] = f"relative error {err:.2e}, iterations {info.iterations}"
    assert lml == info.lml and info.converged == 1
    assert err <= (1e-8 if dtype == F64 else 1e-4), (lml, ref)


def _grad_err(g, ref):
    out = {k: abs(g[k] - ref[k]) / max(abs(ref[k]), 1e-300) for k in ("variance", "diag", "mean_const")}
    out["inv_lengthscale"] = float(np.abs(g["inv_lengthscale"] - ref["inv_lengthscale"]).max() / np.abs(ref["inv_lengthscale"]).max())
    return out


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
def test_lml_and_gradient_with_rademacher_probes(ctx, family, dtype):
    N, d, diag = 300, 2, 0.1
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    z = draw_probes(N, 16, 4)
    tol = 1e-12 if dtype == F64 else 1e-5   # fp64: two CG runs at one tol differ by up to cond tol in alpha; 1e-12 keeps that below the contract
    dev = _dev(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, mean_const=0.25, tol=tol, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, z)
        lml2, info2 = dev.fit(desc, z)
        alpha = dev.alpha()
    finally:
        dev.free()
    ok = _okernel(family, d, dtype)
    r = cr.estimate(ok, x.astype(F64), float(dtype(diag)), y.astype(F64) - 0.25, z, tol, 2000, grad=True)
    c = 1e-8 if dtype == F64 else 1e-4
    ge = _grad_err(g, r["grad"])
    OBSERVED[f"lml rademacher k{family} {np.dtype(dtype).name}"] = (
        f"lml {abs(lml - r['lml']) / abs(r['lml']):.2e}, gradient " + ", ".join(f"{k} {v:.2e}" for k, v in ge.items()))
    assert lml == lml2 and info.converged == 1 and info.quad == info2.quad
    assert abs(lml - r["lml"]) <= c * abs(r["lml"]) and abs(info.quad - r["quad"]) <= c * abs(r["quad"])
    assert abs(info.logdet - r["logdet"]) <= c * max(abs(r["logdet"]), abs(r["lml"]))
    cond = np.linalg.cond(cr.khat(ok, x.astype(F64), float(dtype(diag))))
    np.testing.assert_allclose(alpha.astype(F64), r["alpha"], atol=2 * cond * tol * np.abs(r["alpha"]).max())   # each within cond tol
    for k, v in ge.items():
        assert v <= c, (k, v, g, r["grad"])   # each block relative to its largest entry


@pytest.mark.parametrize("d", [17, 33])
def test_gradient_with_wide_inputs(ctx, d):
    """fp64 at d = 17 and 33 with 17 columns: the four-column-block kernels of 32 and 64 features, both profiles"""
    N, diag = 65, 0.1
    x, y = _xy(N, d)
    x = x / np.sqrt(d)   # r^2 of order one, so that K is not the identity
    z = draw_probes(N, 16, 4)
    dev = _dev(ctx, x, y, F64)
    try:
        desc, keep = dev.desc(_kernel(M52, d), diag, tol=1e-12, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, z)
    finally:
        dev.free()
    r = cr.estimate(_okernel(M52, d), x, diag, y, z, 1e-12, 2000, grad=True)
    ge = _grad_err(g, r["grad"])
    OBSERVED[f"lml rademacher d{d} float64"] = f"lml {abs(lml - r['lml']) / abs(r['lml']):.2e}, gradient " + ", ".join(f"{k} {v:.2e}" for k, v in ge.items())
    assert info.converged == 1 and abs(lml - r["lml"]) <= 1e-8 * abs(r["lml"])
    for k, v in ge.items():
        assert v <= 1e-8, (k, v, g, r["grad"])


def test_shifted_fp32_lengthscale_gradient(ctx):
    """d = 9 in fp32 with x shifted by +30 per coordinate: |xs| ~ 43 against differences of order one.  The lengthscale block is bounded
    by 4 x the float32 restatement's own error against the float64 restatement, on the same float32-rounded inputs."""
    N, d, diag = 300, 9, 0.1
    x, y = _xy(N, d, shift=30.0)
    x, y = x.astype(F32), y.astype(F32)
    z = draw_probes(N, 16, 4)
    dev = _dev(ctx, x, y, F32)
    try:
        desc, keep = dev.desc(_kernel(SE, d), diag, tol=1e-5, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, z)
    finally:
        dev.free()
    ok = _okernel(SE, d, F32)
    r64 = cr.estimate(ok, x.astype(F64), float(F32(diag)), y.astype(F64), z, 1e-5, 2000, grad=True)
    r32 = cr.estimate(ok, x.astype(F64), float(F32(diag)), y.astype(F64), z, 1e-5, 2000, dtype=F32, grad=True)
    e_dev = _grad_err(g, r64["grad"])["inv_lengthscale"]
    e_ref = _grad_err(r32["grad"], r64["grad"])["inv_lengthscale"]
    OBSERVED["shifted fp32 d9 lengthscale block"] = f"device {e_dev:.2e}, float32 restatement {e_ref:.2e}, ratio {e_dev / max(e_ref, 1e-300):.2f}"
    print(OBSERVED["shifted fp32 d9 lengthscale block"])
    assert e_dev <= 4.0 * e_ref, (e_dev, e_ref)


@pytest.mark.parametrize("family", FAMILIES)
def test_unit_probe_gradient_against_central_differences(ctx, family):
    N, d = 48, 2
    x, y = _xy(N, d)
    dev = _dev(ctx, x, y, F64)
    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, tol=1e-12, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, cr.unit_probes(N))
    finally:
        dev.free()
    h = 1e-6
    il = np.full(d, 1.0 / LS)
    f = lambda var, il_, dg, mc=0.0: o.exact_gp_logpdf(o.Kernel(family, var, il_), x, dg, y - mc)
    fd = {"variance": (f(VAR + h, il, 0.1) - f(VAR - h, il, 0.1)) / (2 * h), "diag": (f(VAR, il, 0.1 + h) - f(VAR, il, 0.1 - h)) / (2 * h),
          "mean_const": (f(VAR, il, 0.1, h) - f(VAR, il, 0.1, -h)) / (2 * h),
          "inv_lengthscale": np.array([(f(VAR, il + h * np.eye(d)[c], 0.1) - f(VAR, il - h * np.eye(d)[c], 0.1)) / (2 * h) for c in range(d)])}
    ge = _grad_err(g, fd)
    OBSERVED[f"gradient vs central differences k{family}"] = ", ".join(f"{k} {v:.2e}" for k, v in ge.items())
    for k, v in ge.items():
        # (sum alpha may be near zero: there the central difference's own noise, eps |lml| / h ~ 1e-8, is the floor)
        assert v <= 1e-6 or (k == "mean_const" and abs(g[k] - fd[k]) <= 1e-7), (k, v, g[k], fd[k])


# ---- 7. predict ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("ns", [1, 65, 130])
def test_predict_against_the_exact_posterior(ctx, ns, dtype):
    N, d, diag = 300, 2, 0.1
    family = FAMILIES[ns % 3]
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    xs = np.random.default_rng(ns).uniform(-3, 3, size=(d, ns)).astype(dtype)
    tol = 1e-10 if dtype == F64 else 1e-5
    dev = _dev(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, tol=tol, maxiter=2000)
        dev.fit(desc, None)
        m, v, info = dev.predict(xs)
        m_only = dev.predict(xs, var=False)[0]
    finally:
        dev.free()
    ok = _okernel(family, d, dtype)
    mr, cov = o.exact_gp_posterior(ok, x.astype(F64), float(dtype(diag)), y.astype(F64), xs.astype(F64))
    cond = np.linalg.cond(cr.khat(ok, x.astype(F64), float(dtype(diag))))
    em, ev = np.abs(m - mr).max(), np.abs(v - np.diag(cov)).max()
    OBSERVED[f"predict n{ns} k{family} {np.dtype(dtype).name}"] = f"mean {em:.2e} (max {np.abs(mr).max():.2f}), var {ev:.2e}, cond tol {cond * tol:.2e}"
    assert info.converged == 1 and np.array_equal(m, m_only)
    assert em <= cond * tol * np.abs(mr).max() and ev <= cond * tol * ok.variance, (em, ev, cond * tol)


def test_custom_mean_goes_through_the_python_layer(ctx):
    N, d = 300, 2
    x, y = _xy(N, d)
    trend = lambda xx: 0.5 * np.asarray(xx)[0] - 0.2
    k = _kernel(SE, d)
    f = GP(CustomMean(trend), k)
    cg = ConjugateGradients(tol=1e-10, maxiter=2000, n_probes=4)
    yt = y + trend(x)
    xs = np.random.default_rng(2).uniform(-3, 3, size=(d, 17))
    post = posterior(cg, f(x, 0.1), yt, ctx=ctx)
    try:
        m, v = post.mean_and_var(xs)
        ym, yv = post.predict_y(xs)
        lpd = post.log_predictive_density(xs, np.zeros(17))
        alpha = post.alpha
    finally:
        post.dev.free()
    mr, cov = o.exact_gp_posterior(_okernel(SE, d), x, 0.1, y, xs)
    np.testing.assert_allclose(m, mr + trend(xs), atol=1e-6 * np.abs(mr).max())   # cond tol = 3e3 x 1e-10
    np.testing.assert_allclose(v, np.diag(cov), atol=1e-6 * VAR)
    np.testing.assert_allclose(ym, m, atol=1e-12)
    np.testing.assert_allclose(yv, v + 0.1, atol=1e-12)
    np.testing.assert_allclose(lpd, -0.5 * (np.log(2 * np.pi * yv) + m ** 2 / yv), atol=1e-9)
    assert alpha.shape == (N,) and post.info.converged == 1
    # approx_lml / gradient through the dispatchers: common random numbers make two calls equal
    a = approx_lml(cg, f(x, 0.1), yt, ctx=ctx)
    b, g = approx_lml_and_gradient(cg, f(x, 0.1), yt, ctx=ctx)
    assert a == b == post.lml and set(g) == {"variance", "inv_lengthscale", "diag", "mean_const"}


# ---- 8. statuses, then a healthy call on the same context --------------------------------------------------------------------------
def test_statuses_leave_the_context_healthy(ctx):
    from helpers import device_model

    x8, y8, sva, s2 = o.synth_problem(1, 500, 64, 2)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x8, y8, F64)
    elbo0 = model.elbo(data, 0, 500, 500.0)[0]

    N, d = 300, 2
    x, y = _xy(N, d)
    lib, h = ctx.lib, ctx.h
    dev = _dev(ctx, x, y, F64)
    noy = _dev(ctx, x, None, F64)
    k = _kernel(M32, d)
    desc, keep = dev.desc(k, 0.01, tol=1e-10, maxiter=2000)
    B = np.asfortranarray(y[:, None].copy())
    X = np.zeros_like(B)
    out, info = C.c_double(), _ffi.CGInfo()
    dp = C.POINTER(C.c_double)
    z = draw_probes(N, 2, 0)

    def solve(ds, S=1, b=B, xo=X, ldb=N, ldx=N, on=0):
        return lib.svgp_cg_solve(h, dev.h, ds, S, _ffi._ptr(b) if b is not None else None, ldb, _ffi._ptr(xo) if xo is not None else None, ldx,
                                 on, None, None, C.byref(info))

    def variant(**kw):
        ds, _ = dev.desc(k, kw.pop("diag", 0.01), tol=kw.pop("tol", 1e-10), maxiter=kw.pop("maxiter", 2000))
        for name, val in kw.items():
            setattr(ds, name, val)
        return C.byref(ds)

    INV = _ffi.INVALID_ARG
    try:
        # NULL required pointers
        assert solve(None) == INV and solve(C.byref(desc), b=None) == INV and solve(C.byref(desc), xo=None) == INV
        assert lib.svgp_cg_matvec(h, dev.h, C.byref(desc), 1, None, N, _ffi._ptr(X), N, 0) == INV
        assert lib.svgp_cg_matvec(h, None, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0) == INV
        hh = C.c_void_p()
        assert lib.svgp_cg_create(h, None, C.byref(hh)) == INV and lib.svgp_cg_create(h, dev.data.h, None) == INV
        # dtype / d mismatch, descriptor fields
        assert solve(variant(dtype=_ffi.F32)) == INV and solve(variant(d=3)) == INV and solve(variant(kernel=7)) == INV
        assert solve(variant(maxiter=0)) == INV and solve(variant(tol=0.0)) == INV and solve(variant(tol=float("nan"))) == INV
        assert solve(variant(diag=-1e-3)) == INV and solve(variant(variance=0.0)) == INV and solve(variant(reserved=1)) == INV
        assert solve(variant(inv_lengthscale=None)) == INV
        # shapes
        assert solve(C.byref(desc), S=0) == INV and solve(C.byref(desc), ldb=N - 1) == INV and solve(C.byref(desc), ldx=N - 1) == INV
        assert solve(C.byref(desc), on=2) == INV
        assert lib.svgp_cg_matvec(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N - 1, _ffi._ptr(X), N, 0) == INV
        # fit: data without y and no delta, T < 0, T > 0 with NULL probes
        assert lib.svgp_cg_fit(h, noy.h, C.byref(desc), None, 0, None, C.byref(out), C.byref(info)) == INV
        assert lib.svgp_cg_fit(h, dev.h, C.byref(desc), None, -1, None, C.byref(out), C.byref(info)) == INV
        assert lib.svgp_cg_fit(h, dev.h, C.byref(desc), None, 2, None, C.byref(out), C.byref(info)) == INV
        assert lib.svgp_cg_lml_grad(h, dev.h, C.byref(desc), None, 2, z.ctypes.data_as(dp), C.byref(out), C.byref(info), None, None, None, None) == INV
        # alpha / predict before a successful fit
        with pytest.raises(ValueError, match="fit"):
            dev.alpha()
        with pytest.raises(ValueError, match="fit"):
            dev.predict(x[:, :3])
        # a caller's delta makes y unnecessary
        lml_d, info_d = noy.fit(desc, z, delta=y)
        lml_y, info_y = dev.fit(desc, z)
        assert lml_d == lml_y and info_d.quad == info_y.quad
        # out of iterations: SVGP_OK, converged = 0
        short, _ = dev.desc(k, 0.01, tol=1e-10, maxiter=3)
        Xs, iters, rel, inf = dev.solve(short, B)
        assert inf.converged == 0 and inf.n_unconverged == 1 and iters[0] == 3 and rel[0] > 1e-10 and np.isfinite(Xs).all()
        with pytest.warns(RuntimeWarning, match="residual"):
            approx_lml(ConjugateGradients(tol=1e-10, maxiter=3, n_probes=2), GP(k)(x, 0.01), y, ctx=ctx)
        # the cap of the predictive variance
        m1 = np.zeros(1)
        big = (1 << 28) // N + 1
        assert lib.svgp_cg_predict(h, dev.h, _ffi.COLVECS, big, _ffi._ptr(X), _ffi._ptr(m1), _ffi._ptr(m1), C.byref(info)) == _ffi.UNSUPPORTED
        assert lib.svgp_cg_predict(h, dev.h, _ffi.COLVECS, 0, _ffi._ptr(X), _ffi._ptr(m1), _ffi._ptr(m1), C.byref(info)) == INV
        # a NaN coordinate: SVGP_NOT_POSDEF with NaN outputs
        xn = x.copy()
        xn[1, 7] = np.nan
        bad = _dev(ctx, xn, y, F64)
        try:
            Xn = np.zeros_like(B)
            rc = lib.svgp_cg_solve(h, bad.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(Xn), N, 0, None, None, C.byref(info))
            assert rc == _ffi.NOT_POSDEF and np.isnan(Xn).all() and np.isnan(info.max_rel_residual)
            with pytest.raises(_ffi.PosDefException):
                bad.fit(desc, z)
            with pytest.raises(ValueError, match="fit"):
                bad.alpha()
        finally:
            bad.free()
        # and a healthy call afterwards
        Xh, iters, rel, inf = dev.solve(desc, B)
        assert inf.converged == 1 and np.abs(cr.khat(_okernel(M32, d), x, 0.01) @ Xh[:, 0] - y).max() <= 1e-8 * np.abs(y).max()
    finally:
        dev.free()
        noy.free()
    assert model.elbo(data, 0, 500, 500.0)[0] == elbo0   # bitwise
    model.free()
    data.free()


def test_report_observed_errors():
    """Prints the table profiles/cg/accuracy.md records (run the module with -s); SVGP_CG_ACCURACY_MD=path also writes it there."""
    lines = ["| check | measured |", "|---|---|"] + [f"| {name} | {text} |" for name, text in OBSERVED.items()]
    print("\n".join(lines))
    path = os.environ.get("SVGP_CG_ACCURACY_MD")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
