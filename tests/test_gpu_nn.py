"""GPU checks of the NearestNeighbors (Vecchia) approximation (csrc/nn.hip, svgp_nn_*) against the float64 restatement of
tests/nn_ref.py (itself pinned to the reference package's values and to finite differences in tests/test_nn_cpu.py).

Tolerances: fp64 lml 1e-8 relative, fp32 1e-4 against the float64 restatement on the fp32-rounded inputs (the restatement's own two
formulations agree to 5e-14 and its float32 run to 1e-5 on these inputs: tests/test_nn_cpu.py); gradients and predictions as
tests/test_gpu_laplace.py / test_gpu_laplace_edges.py: gradient 1e-6 (fp64) / 1e-3 (fp32) of the largest kernel-parameter entry,
predictions 1e-9 (fp64) / 1e-4 (fp32) of the largest mean and of the prior variance."""
import ctypes as C

import numpy as np
import pytest
import torch

import nn_ref as nr
import svgp_oracle as o
from approxgp import (GP, DeviceNearestNeighbors, NearestNeighbors, SEKernel, _ffi, approx_lml, approx_lml_and_gradient, posterior)
from approxgp.kernels import ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, TransformedKernel

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
BASES = {o.KERNEL_SE: SEKernel, o.KERNEL_MATERN32: Matern32Kernel, o.KERNEL_MATERN52: Matern52Kernel}
VAR, DIAG = 1.2, 1e-2
XR = np.array([1.0, 2.0, 3.5, 4.2, 5.9, 8.0])   # test/NearestNeighborsModule.jl:2-6
YR = np.sin(XR)


def _kernel(family, var, il):
    return ScaledKernel(TransformedKernel(BASES[family](), ARDTransform(np.asarray(il, dtype=np.float64))), var)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _dev(ctx, x, y, dtype, layout=_ffi.COLVECS):
    if layout == _ffi.ROWVECS:
        return DeviceNearestNeighbors(ctx, np.asarray(x).T, y, dtype, layout=_ffi.ROWVECS)
    if layout == _ffi.VEC:
        return DeviceNearestNeighbors(ctx, np.asarray(x)[0], y, dtype)
    return DeviceNearestNeighbors(ctx, x, y, dtype)


NS = [1, 2, 17, 64, 65, 66, 300, 1000]
KS = [1, 3, 16, 17, 32, 33, 64, None]   # None: k >= n
DS = [1, 3, 8, 64]


def _cases():
    """24 cases: every n, k (both bucket edges 16 / 17 and 32 / 33, and k >= n) and d of the lists, every layout, dtype and family,
    isotropic and ARD"""
    cases = []
    for i in range(24):
        n = NS[i % 8]
        k = KS[(i + 3 + i // 8) % 8]   # the k >= n cases land on n = 65, 64, 17: k >= n counts as n - 1 neighbours, at most 64
        d = DS[(i + i // 4) % 4]
        layout = _ffi.VEC if d == 1 else [_ffi.COLVECS, _ffi.ROWVECS][i % 2]
        cases.append((n, n + 3 if k is None else k, d, layout, [F64, F32][(i // 2 + i // 8) % 2], i % 3, bool((i // 3) % 2)))
    assert {c[0] for c in cases} == set(NS) and {c[2] for c in cases} == set(DS) and {c[3] for c in cases} == {0, 1, 2}
    assert {1, 3, 16, 17, 32, 33, 64} <= {c[1] for c in cases} and any(c[1] >= c[0] > 2 for c in cases) and all(min(c[1], c[0] - 1) <= 64 for c in cases)
    assert {(c[4], c[5]) for c in cases} == {(t, f) for t in (F64, F32) for f in range(3)} and {c[6] for c in cases} == {True, False}
    return cases


@pytest.mark.parametrize("n,k,d,layout,dtype,fam,ard", _cases())
def test_lml_parity(ctx, n, k, d, layout, dtype, fam, ard):
    x, y = nr.synth(n, d, seed=1000 + n + k, dtype=dtype)
    il = nr.invl_for(d, ard)
    ref = nr.lml(nr.kernel_of(fam, VAR, il), x, y, k, DIAG, mean_const=0.1)
    dev = _dev(ctx, x, y, dtype, layout)
    desc, keep = dev.desc(_kernel(fam, VAR, il), k, DIAG, 0.1)
    val, info = dev.lml(desc)
    val2, _ = dev.fit(desc)
    dev.free()
    print(f"n {n} k {k} d {d} {np.dtype(dtype).name} family {fam}: lml {val:.12g} ref {ref:.12g} rel {abs(val - ref) / abs(ref):.2e}")
    assert info.first_bad == 0 and info.n_neg_f == 0
    assert abs(val - ref) <= (1e-8 if dtype == F64 else 1e-4) * abs(ref), (val, ref)
    assert val2 == val   # the fit computes the same terms


@pytest.fixture(scope="module")
def problem():
    """n = 300, d = 2: shared by the factor, prediction and repeatability tests; the references are computed once per (k, dtype)"""
    x, y = nr.synth(300, 2, seed=7)
    il = np.array([0.8, 1.1])
    kern = nr.kernel_of(o.KERNEL_MATERN52, VAR, il)
    cache = {}

    def ref(k, dtype):
        if (k, dtype) not in cache:
            cache[(k, dtype)] = nr.fit(kern, x.astype(dtype).astype(F64), y.astype(dtype).astype(F64), k, DIAG, mean_const=0.2)   # float64 on the rounded inputs
        return cache[(k, dtype)]

    return dict(x=x, y=y, il=il, kern=kern, ref=ref, dkern=_kernel(o.KERNEL_MATERN52, VAR, il))


@pytest.mark.parametrize("dtype,k", [(F64, 33), (F64, 64), (F32, 16)])
def test_factors(ctx, problem, dtype, k):
    """b_i, F_i and alpha element-wise.  fp64: 1e-9 of the largest entry (the prediction tolerance).  fp32: the two sides solve
    C b = c in different precisions, so they differ by cond(C) eps32 at most, cond(C) <= (k variance + diag) / diag: 4 eps32 k variance / diag"""
    p = problem
    r = p["ref"](k, dtype)
    dev = _dev(ctx, p["x"].astype(dtype), p["y"].astype(dtype), dtype)
    desc, keep = dev.desc(p["dkern"], k, DIAG, 0.2)
    dev.fit(desc)
    B, F, alpha = dev.factors()
    dev.free()
    tol = 1e-9 if dtype == F64 else 4 * np.finfo(F32).eps * k * VAR / DIAG
    band = nr.banded(r["B"], k)
    assert B.shape == band.shape == (300, k)
    for i in range(k):   # the ramp-up rows: point i has i neighbours, the band's first k - i entries are exactly zero
        assert np.all(B[i, :k - i] == 0)
        assert np.max(np.abs(B[i, k - i:] - band[i, k - i:]), initial=0.0) <= tol * max(np.max(np.abs(band[i])), 1.0)
    print(f"{np.dtype(dtype).name} k {k}: B {np.max(np.abs(B - band)) / np.max(np.abs(band)):.2e} F {np.max(np.abs(F - r['F']) / r['F']):.2e} "
          f"alpha {np.max(np.abs(alpha - r['alpha'])) / np.max(np.abs(r['alpha'])):.2e}")
    assert np.max(np.abs(B - band)) <= tol * np.max(np.abs(band))
    assert np.max(np.abs(F - r["F"]) / r["F"]) <= tol
    assert np.max(np.abs(alpha - r["alpha"])) <= tol * np.max(np.abs(r["alpha"]))


@pytest.mark.parametrize("k,fam", [(3, o.KERNEL_SE), (33, o.KERNEL_MATERN32), (64, o.KERNEL_MATERN52)])
def test_gradient(ctx, k, fam):
    d = 3
    x, y = nr.synth(300, d, seed=30 + k)
    il = np.array([0.8, 0.95, 1.1])
    ref, rv, ril, rd = nr.lml_grad(nr.kernel_of(fam, VAR, il), x, y, k, DIAG, 0.1)
    dev = _dev(ctx, x, y, F64)
    desc, keep = dev.desc(_kernel(fam, VAR, il), k, DIAG, 0.1)
    lml, gv, gil, gd, _ = dev.lml_grad(desc)
    dev.free()
    g, gr = np.concatenate([[gv], gil]), np.concatenate([[rv], ril])
    scale = np.max(np.abs(gr))
    print(f"k {k} family {fam}: kernel parameters {np.max(np.abs(g - gr)) / scale:.2e} diag {abs(gd - rd) / abs(rd):.2e}")
    assert abs(lml - ref) <= 1e-8 * abs(ref)
    assert np.max(np.abs(g - gr)) <= 1e-6 * scale, (g, gr)
    assert abs(gd - rd) <= 1e-6 * abs(rd), (gd, rd)   # d / d diag is orders of magnitude larger: its own scale
    dev32 = _dev(ctx, x.astype(F32), y.astype(F32), F32)
    desc32, keep32 = dev32.desc(_kernel(fam, VAR, il), k, DIAG, 0.1)
    _, gv32, gil32, gd32, _ = dev32.lml_grad(desc32)
    dev32.free()
    print(f"  fp32: kernel parameters {np.max(np.abs(np.concatenate([[gv32], gil32]) - gr)) / scale:.2e} diag {abs(gd32 - rd) / abs(rd):.2e}")
    assert np.max(np.abs(np.concatenate([[gv32], gil32]) - gr)) <= 1e-3 * scale
    assert abs(gd32 - rd) <= 1e-3 * abs(rd)


def test_gradient_on_the_reference_data_without_diag(ctx):
    ref, rv, ril, rd = nr.lml_grad(nr.kernel_of(o.KERNEL_SE, 1.0, [1.0]), XR, YR, 3, 0.0)
    dev = DeviceNearestNeighbors(ctx, XR, YR, F64)
    desc, keep = dev.desc(_kernel(o.KERNEL_SE, 1.0, [1.0]), 3)
    lml, gv, gil, gd, _ = dev.lml_grad(desc)
    dev.free()
    assert abs(lml - (-6.070853690320693)) <= 1e-8 * abs(lml)
    scale = max(abs(rv), abs(ril[0]))
    assert abs(gv - rv) <= 1e-6 * scale and abs(gil[0] - ril[0]) <= 1e-6 * scale and abs(gd - rd) <= 1e-6 * abs(rd)


@pytest.mark.parametrize("nstar", [1, 15, 16, 129])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_predictions(ctx, problem, dtype, nstar):
    p = problem
    k = 17
    r = p["ref"](k, dtype)
    rng = np.random.default_rng(100 + nstar)
    xs = rng.uniform(-2, 2, size=(2, nstar)).astype(dtype)
    ys = rng.uniform(-2, 2, size=(2, 7)).astype(dtype)
    dev = _dev(ctx, p["x"].astype(dtype), p["y"].astype(dtype), dtype)
    desc, keep = dev.desc(p["dkern"], k, DIAG, 0.2)
    dev.fit(desc)
    m, v, c = dev.predict(xs, cov=True)
    cx = dev.cross_cov(xs, ys)
    m1, v1, _ = dev.predict(xs)
    dev.free()
    x_in = p["x"].astype(dtype).astype(F64)
    rm, rv, rc = nr.predict(r, p["kern"], x_in, xs.astype(F64))
    _, _, rcx = nr.predict(r, p["kern"], x_in, xs.astype(F64), ys.astype(F64))
    tol_m, tol_v = (1e-9 * np.max(np.abs(rm)), 1e-9) if dtype == F64 else (1e-4 * np.max(np.abs(rm)), 1e-4 * VAR)
    print(f"{np.dtype(dtype).name} n* {nstar}: mean {np.max(np.abs(m - rm)):.2e} var {np.max(np.abs(v - rv)):.2e} cov {np.max(np.abs(c - rc)):.2e} "
          f"cross {np.max(np.abs(cx - rcx)):.2e}")
    np.testing.assert_allclose(m, rm, rtol=0, atol=tol_m)
    np.testing.assert_allclose(v, rv, rtol=0, atol=tol_v)
    np.testing.assert_allclose(c, rc, rtol=0, atol=tol_v)
    np.testing.assert_allclose(cx, rcx, rtol=0, atol=tol_v)
    assert np.array_equal(m1, m) and np.array_equal(v1, v)
    if dtype == F64:
        np.testing.assert_allclose(np.diag(c), v, rtol=0, atol=1e-12)
        assert np.max(np.abs(c - c.T)) <= 1e-12


def test_reference_assertions_through_the_mirror(ctx):
    """test/NearestNeighborsModule.jl: mean_and_cov at 1.0:0.1:8 against the exact GP, atol 1e-4 (k = 5) / 1e-1 (k = 3); lml atol 1e-2"""
    f = GP(SEKernel())
    unit = nr.kernel_of(o.KERNEL_SE, 1.0, [1.0])
    xs = np.arange(1.0, 8.0 + 1e-9, 0.1)
    em, ec = nr.exact_predict(unit, XR, YR, 0.0, xs)
    for k, atol in ((5, 1e-4), (3, 1e-1)):
        post = posterior(NearestNeighbors(k), f(XR), YR, ctx=ctx)
        m, c = post.mean_and_cov(xs)
        post.dev.free()
        np.testing.assert_allclose(m, em, rtol=0, atol=atol)
        np.testing.assert_allclose(c, ec, rtol=0, atol=atol)
    v3 = approx_lml(NearestNeighbors(3), f(XR), YR, ctx=ctx)
    assert abs(v3 - nr.exact_lml(unit, XR, YR, 0.0)) <= 1e-2
    assert abs(v3 - (-6.070853690320693)) <= 1e-8 * abs(v3)
    assert abs(approx_lml(NearestNeighbors(5), f(XR), YR, ctx=ctx) - (-6.073251508326499)) <= 1e-8 * 6.07
    v, g = approx_lml_and_gradient(NearestNeighbors(3), f(XR), YR, ctx=ctx)
    assert v == v3 and set(g) == {"variance", "inv_lengthscale", "diag"}


def test_all_neighbours_is_the_exact_gp(ctx):
    n, d = 40, 2
    x, y = nr.synth(n, d, seed=1)
    il = np.array([0.8, 1.1])
    kern = nr.kernel_of(o.KERNEL_MATERN52, VAR, il)
    f = GP(0.3, _kernel(o.KERNEL_MATERN52, VAR, il))
    ex = nr.exact_lml(kern, x, y, DIAG, mean_const=0.3)
    for k in (n - 1, n + 7):
        v = approx_lml(NearestNeighbors(k, include_noise=True), f(x, DIAG), y, ctx=ctx)
        assert abs(v - ex) <= 1e-8 * abs(ex), (k, v, ex)
    post = posterior(NearestNeighbors(n - 1, include_noise=True), f(x, DIAG), y, ctx=ctx)
    xs = np.random.default_rng(2).uniform(-2, 2, size=(d, 30))
    m, c = post.mean_and_cov(xs)
    post.dev.free()
    em, ec = nr.exact_predict(kern, x, y, DIAG, xs, mean_const=0.3)
    np.testing.assert_allclose(m, em, rtol=0, atol=1e-9 * np.max(np.abs(em)))
    np.testing.assert_allclose(c, ec, rtol=0, atol=1e-9)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_bitwise_repeatability(ctx, problem, dtype):
    p = problem
    out = []
    for _handle in range(2):
        dev = _dev(ctx, p["x"].astype(dtype), p["y"].astype(dtype), dtype)
        desc, keep = dev.desc(p["dkern"], 33, DIAG, 0.2)
        for _call in range(2):
            lml, gv, gil, gd, _ = dev.lml_grad(desc)
            out.append(np.concatenate([[lml, gv, gd], gil]).tobytes())
        dev.free()
    assert len(set(out)) == 1


def test_errors_leave_the_context_healthy(ctx, problem):
    p = problem
    lib = ctx.lib
    ref = p["ref"](17, F64)["lml"]

    def healthy():
        dev = _dev(ctx, p["x"], p["y"], F64)
        desc, keep = dev.desc(p["dkern"], 17, DIAG, 0.2)
        v = dev.lml(desc)[0]
        dev.free()
        assert abs(v - ref) <= 1e-8 * abs(ref)

    # a duplicated point with diag = 0: an ordinary numerical status, with the point's 1-based index
    x = p["x"].copy()
    x[:, 123] = x[:, 122]
    dev = _dev(ctx, x, p["y"], F64)
    desc, keep = dev.desc(p["dkern"], 17, 0.0)
    lml, info = C.c_double(), _ffi.NNInfo()
    assert lib.svgp_nn_lml(ctx.h, dev.h, C.byref(desc), C.byref(lml), C.byref(info)) == _ffi.NOT_POSDEF
    assert info.first_bad == 124 and np.isnan(lml.value)
    with pytest.raises(_ffi.PosDefException) as ei:
        dev.lml(desc)
    assert ei.value.info == 124
    good, keep2 = dev.desc(p["dkern"], 17, DIAG)
    assert np.isfinite(dev.lml(good)[0])   # the same handle, with the diagonal term
    healthy()
    # k = 65
    big, keep3 = dev.desc(p["dkern"], 65, DIAG)
    assert lib.svgp_nn_lml(ctx.h, dev.h, C.byref(big), C.byref(lml), C.byref(info)) == _ffi.UNSUPPORTED
    healthy()
    # predict before fit, and the other argument errors
    xs = np.zeros((2, 4))
    m = np.zeros(4)
    assert lib.svgp_nn_predict(ctx.h, dev.h, _ffi.COLVECS, 4, _ffi._ptr(np.asfortranarray(xs)), _ffi._ptr(m), None, None) == _ffi.INVALID_ARG
    assert lib.svgp_nn_factors(ctx.h, dev.h, None, _ffi._ptr(m), None) == _ffi.INVALID_ARG

    def status(**kw):
        ds, keep4 = dev.desc(p["dkern"], 17, DIAG)
        for k_, v_ in kw.items():
            setattr(ds, k_, v_)
        return lib.svgp_nn_lml(ctx.h, dev.h, C.byref(ds), C.byref(lml), C.byref(info))

    assert status(k=0) == _ffi.INVALID_ARG
    assert status(d=3) == _ffi.INVALID_ARG
    assert status(dtype=_ffi.F32) == _ffi.INVALID_ARG
    assert status(variance=0.0) == _ffi.INVALID_ARG
    assert status(diag=-1.0) == _ffi.INVALID_ARG
    assert status(reserved=1) == _ffi.INVALID_ARG
    assert lib.svgp_nn_lml(ctx.h, dev.h, None, C.byref(lml), None) == _ffi.INVALID_ARG
    assert lib.svgp_nn_lml(ctx.h, dev.h, C.byref(good), None, None) == _ffi.INVALID_ARG
    h = C.c_void_p()
    nodata = _ffi.DeviceData(ctx, x, None, F64)
    assert lib.svgp_nn_create(ctx.h, nodata.h, C.byref(h)) == _ffi.INVALID_ARG
    nodata.free()
    dev.free()
    healthy()


def test_create_evaluate_free_returns_device_memory(ctx):
    """50 rounds of create / lml / lml_grad / fit / predict / free at n = 20000 (about 2 MB of handle buffers a round): the free device
    memory after the last round is that after the first"""
    x, y = nr.synth(20000, 2, seed=3)
    xs = x[:, :50].copy()
    kern = _kernel(o.KERNEL_SE, VAR, [0.9, 0.9])
    free, first = [], None
    for it in range(50):
        dev = _dev(ctx, x, y, F64)
        desc, keep = dev.desc(kern, 16, DIAG)
        v = dev.lml(desc)[0]
        dev.lml_grad(desc)
        dev.fit(desc)
        dev.predict(xs, cov=True)
        dev.free()
        first = v if first is None else first
        assert v == first
        if it in (0, 49):
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
    assert free[1] >= free[0], free
