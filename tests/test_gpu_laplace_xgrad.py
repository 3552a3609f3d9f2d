"""GPU checks of svgp_laplace_lml_grad_inputs (csrc/laplace_xgrad.hip): d approx_lml / d x of the Laplace approximation against the
closed form  x_bar[f, i] = 4 variance invl_f^2 sum_k P_ik kappa'(r2_ik) (x_if - x_kf)  evaluated in float64 numpy from the
restatement's a, R, g, u (tests/laplace_ref.py), itself pinned here to central differences of the restatement's approx_lml.

Measured on an MI355X (profiles/laplace/accuracy_xgrad.md), largest error over the parity cases relative to max |x_bar|:
f64 5.5e-14 (bound 1e-6), fp32 1.0e-5 (bound 1e-3)."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.linalg import solve_triangular

import laplace_ref as lr
import svgp_oracle as o
import test_gpu_laplace as base
from approxgp import BernoulliLikelihood, DeviceLaplace, GP, LaplaceApproximation, LatentGP, _ffi, approx_lml_and_gradient
from test_gpu_laplace import ctx  # noqa: F401  (the module's context fixture)

pytestmark = pytest.mark.gpu

# the bounds tests/test_gpu_laplace.py::test_gradient applies to d_inv_lengthscale, relative to the largest entry
TOL = {np.float64: 1e-6, np.float32: 1e-3}


def closed_form(kernel, x, y, lik, s2, jitter, eps=np.finfo(np.float64).eps, maxiter=100):
    """-> (lml, x_bar (d, n)) in float64: P of laplace_ref.lml_grad, contracted per row with d K / d x."""
    lml, c, _, _ = lr.fit(kernel, x, y, lik, s2, jitter, None, maxiter, eps)
    K, sW, g, a = c["K"], c["sW"], c["g"], c["a"]
    Linv = solve_triangular(c["L"], np.eye(K.shape[0]), lower=True)
    R = sW[:, None] * (Linv.T @ Linv) * sW[None, :]
    s2v = 0.5 * (np.diag(K) - np.einsum("ij,ji->i", K @ R, K)) * c["d3"]
    u = s2v - R @ (K @ s2v)
    P = 0.5 * (np.outer(a, a) - R + np.outer(u, g) + np.outer(g, u))
    xd = o._as_dn(np.asarray(x, dtype=np.float64))
    il = np.asarray(kernel.inv_lengthscale, dtype=np.float64)
    diff = xd[:, :, None] - xd[:, None, :]                                  # (d, n, n): x_if - x_kf
    r2 = np.einsum("f,fik->ik", il ** 2, diff ** 2)
    if kernel.family == o.KERNEL_SE:
        dk = -0.5 * np.exp(-0.5 * r2)
    elif kernel.family == o.KERNEL_MATERN32:
        dk = -1.5 * np.exp(-np.sqrt(3.0 * r2))
    else:
        dk = -(5.0 / 6.0) * (1.0 + np.sqrt(5.0 * r2)) * np.exp(-np.sqrt(5.0 * r2))
    return lml, 4.0 * kernel.variance * il[:, None] ** 2 * np.einsum("ik,fik->fi", P * dk, diff)


def _cases():
    """Every (N, d) of the issue's seams once - N under a tile, across one, across two with a ragged edge (N = 130: four column
    segments); d in the kernel's feature buckets DQ = 2 (d <= 8) and, from their low side, 4 and 8.  With i = 4 k + r: d from r, N from
    i % 5, dtype from k and ARD from k // 2, so that every d meets both dtypes with and without ARD; family, likelihood and layout
    rotate with periods 3 and 9.  Then the bucket DQ = 16 (d > 32: the largest LDS and register footprint) at d = 33 and at the
    full d = 64, and the buckets 4 and 8 filled to their tops, in both dtypes."""
    ns, ds = [1, 2, 63, 65, 130], [1, 3, 9, 17]
    cases = []
    for i in range(20):
        k, d = i // 4, ds[i % 4]
        layout = (_ffi.COLVECS if i == 8 else _ffi.VEC) if d == 1 else (_ffi.ROWVECS if i % 3 == 0 else _ffi.COLVECS)
        cases.append((ns[i % 5], d, (i // 3) % 3, (1, 2, 0)[i % 3], bool((k // 2) % 2), [np.float64, np.float32][k % 2], layout))
    cases += [(65, 33, 1, 1, True, np.float64, _ffi.COLVECS), (130, 64, 2, 2, False, np.float64, _ffi.ROWVECS),
              (130, 33, 0, 0, False, np.float32, _ffi.ROWVECS), (65, 64, 1, 2, True, np.float32, _ffi.COLVECS),
              (65, 16, 2, 1, True, np.float64, _ffi.ROWVECS), (130, 32, 0, 2, True, np.float64, _ffi.COLVECS),
              (130, 16, 1, 0, False, np.float32, _ffi.COLVECS), (65, 32, 2, 1, False, np.float32, _ffi.ROWVECS)]
    return cases


def _problem(n, d, fam, lik, ard, dtype, seed=0):
    x, y = lr.synth(lik, n, d, seed=300 + 7 * n + d + seed)
    il = (np.linspace(0.6, 1.4, d) if ard else np.full(d, 0.9)) / np.sqrt(d)
    return x.astype(dtype), y.astype(dtype), il, base._s2(lik)


@pytest.mark.parametrize("n,d,fam,lik,ard,dtype,layout", _cases())
def test_parity_with_closed_form(ctx, n, d, fam, lik, ard, dtype, layout):
    x, y, il, s2 = _problem(n, d, fam, lik, ard, dtype)
    lml_ref, ref = closed_form(lr.kernel_of(fam, 1.2, il), x, y, lik, s2, 1e-6, eps=np.finfo(dtype).eps)
    dev = base._dev(ctx, x, y, dtype, layout)
    desc, keep = dev.desc(base._kernel(fam, 1.2, il), base._lik(lik, s2), 1e-6)
    lml, dv, dil, xg, info = dev.lml_grad(desc, wrt_inputs=True)
    dev.free()
    assert xg.shape == (d, n) and xg.dtype == dtype
    scale = np.max(np.abs(ref))
    err = np.max(np.abs(xg - ref))
    print(f"xgrad n={n} d={d} fam={fam} lik={lik} {np.dtype(dtype).name}: err/scale {err / max(scale, 1e-300):.3e} scale {scale:.3e}")
    assert err <= TOL[dtype] * scale
    if n == 1:
        assert np.all(xg == 0)


@pytest.mark.parametrize("fam", [0, 1, 2])
@pytest.mark.parametrize("lik", [1, 2])
def test_closed_form_against_differences(ctx, fam, lik):
    """CPU: the closed form against central differences of the restatement's approx_lml in every coordinate (N = 17, d = 3), with
    the Newton loop run to rtol 1e-12 (eps = 1e-24) so that the lml carries ~1e-13 of noise: at h = 1e-4 the two agree to 2e-8 of the
    largest entry over the six cases (truncation h^2 |lml'''| / 6 and noise 1e-13 / h are both ~1e-9); asserted at 1e-6.  Then the
    device at the same point."""
    n, d = 17, 3
    x, y, il, s2 = _problem(n, d, fam, lik, True, np.float64, seed=1)
    k = lr.kernel_of(fam, 1.2, il)
    _, ref = closed_form(k, x, y, lik, s2, 1e-6, eps=1e-24)
    h, fd = 1e-4, np.zeros((d, n))
    for f in range(d):
        for i in range(n):
            e = np.zeros((d, n))
            e[f, i] = h
            fd[f, i] = (lr.fit(k, x + e, y, lik, s2, 1e-6, eps=1e-24)[0] - lr.fit(k, x - e, y, lik, s2, 1e-6, eps=1e-24)[0]) / (2 * h)
    scale = np.max(np.abs(ref))
    print(f"closed form vs differences fam={fam} lik={lik}: {np.max(np.abs(ref - fd)) / scale:.3e}")
    assert np.max(np.abs(ref - fd)) <= 1e-6 * scale
    dev = DeviceLaplace(ctx, x, y, np.float64)
    desc, keep = dev.desc(base._kernel(fam, 1.2, il), base._lik(lik, s2), 1e-6)
    xg = dev.lml_grad(desc, wrt_inputs=True)[3]
    dev.free()
    assert np.max(np.abs(xg - ref)) <= TOL[np.float64] * scale


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bitwise_contracts(ctx, dtype):
    n, d = 130, 9
    x, y, il, s2 = _problem(n, d, 2, 2, True, dtype)
    xs = np.random.default_rng(5).uniform(-2, 2, size=(d, 40)).astype(dtype)
    dev = DeviceLaplace(ctx, x, y, dtype)
    desc, keep = dev.desc(base._kernel(2, 1.2, il), base._lik(2, s2), 1e-6)
    lml0, dv0, dil0, _ = dev.lml_grad(desc)
    pred0 = dev.predict(xs)
    lml1, dv1, dil1, xg1, _ = dev.lml_grad(desc, wrt_inputs=True)
    pred1 = dev.predict(xs)
    out = torch.full((d, n), 7.0, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    lml2, dv2, dil2, xg2, _ = dev.lml_grad(desc, wrt_inputs=True, x_grad_out=out)
    torch.cuda.synchronize()
    dev.free()
    assert xg2 is out
    assert (lml0, dv0) == (lml1, dv1) == (lml2, dv2) and np.array_equal(dil0, dil1) and np.array_equal(dil0, dil2)
    assert np.array_equal(xg1, out.cpu().numpy()) and np.all(np.isfinite(xg1)) and np.any(xg1 != 0)
    assert np.array_equal(pred0[0], pred1[0]) and np.array_equal(pred0[1], pred1[1])


def test_errors_leave_a_healthy_context(ctx):
    n, d = 64, 2
    x, y = lr.synth(1, n, d, seed=23)   # the input of test_gpu_laplace_edges.py::test_a_nan_never_gives_a_finite_lml
    il = np.array([0.8, 1.1])
    xt, yt = torch.tensor(x, device="cuda").contiguous(), torch.tensor(y, device="cuda")
    data = _ffi.DeviceData.wrap(ctx, np.float64, d, n, n, xt.data_ptr(), yt.data_ptr())
    dev = DeviceLaplace(ctx, data=data)
    desc, keep = dev.desc(base._kernel(0, 1.0, il), BernoulliLikelihood(), 1e-6)
    lml, info, dv, dil, xg = C.c_double(), _ffi.LaplaceInfo(), C.c_double(), np.zeros(d), np.zeros((d, n))

    def call(h, gx):
        return ctx.lib.svgp_laplace_lml_grad_inputs(ctx.h, h, C.byref(desc), None, C.byref(lml), C.byref(info), C.byref(dv),
                                                    dil.ctypes.data_as(C.POINTER(C.c_double)), gx)

    assert call(dev.h, None) == _ffi.INVALID_ARG
    assert call(dev.h, C.byref(_ffi.InputGrad(_ffi._ptr(xg), n - 1, 0, 0))) == _ffi.INVALID_ARG
    assert call(dev.h, C.byref(_ffi.InputGrad(C.c_void_p(xt.data_ptr() + 8 * n), n, 1, 0))) == _ffi.INVALID_ARG   # inside x
    assert call(dev.h, C.byref(_ffi.InputGrad(C.c_void_p(yt.data_ptr()), n, 1, 0))) == _ffi.INVALID_ARG
    _, ref = closed_form(lr.kernel_of(0, 1.0, il), x, y, 1, 1.0, 1e-6)
    got = dev.lml_grad(desc, wrt_inputs=True)[3]   # the wrapped torch features, read in place
    assert np.max(np.abs(got - ref)) <= 1e-6 * np.max(np.abs(ref))
    dev.free()
    data.free()
    # a NaN coordinate: the parent call's status, NaN in every entry, and the context goes on
    xb = x.copy()
    xb[1, 40] = np.nan
    bad = DeviceLaplace(ctx, xb, y, np.float64)
    desc, keep = bad.desc(base._kernel(0, 1.0, il), BernoulliLikelihood(), 1e-6, maxiter=3)
    rc_parent = ctx.lib.svgp_laplace_lml_grad(ctx.h, bad.h, C.byref(desc), None, C.byref(lml), C.byref(info), C.byref(dv),
                                              dil.ctypes.data_as(C.POINTER(C.c_double)))
    xg[:] = 0.0
    assert call(bad.h, C.byref(_ffi.InputGrad(_ffi._ptr(xg), n, 0, 0))) == rc_parent and np.isnan(lml.value)
    assert np.all(np.isnan(xg))
    bad.free()
    good = DeviceLaplace(ctx, x, y, np.float64)
    desc, keep = good.desc(base._kernel(0, 1.0, il), BernoulliLikelihood(), 1e-6)
    assert np.array_equal(good.lml_grad(desc, wrt_inputs=True)[3], got)
    good.free()


def test_mirror_shapes(ctx):
    x, y = lr.synth(1, 40, 3, seed=2)
    lf = LatentGP(GP(base._kernel(1, 1.3, [0.7, 0.9, 1.1])), BernoulliLikelihood(), 1e-6)
    la = LaplaceApproximation()
    v, g = approx_lml_and_gradient(la, lf(x), y, ctx=ctx, wrt_inputs=True)
    vr, gr = approx_lml_and_gradient(la, lf(np.ascontiguousarray(x.T)), y, ctx=ctx, wrt_inputs=True, layout=_ffi.ROWVECS)
    assert g["x"].shape == (3, 40) and gr["x"].shape == (40, 3) and np.array_equal(gr["x"].T, g["x"]) and vr == v
    _, ref = closed_form(lr.kernel_of(1, 1.3, [0.7, 0.9, 1.1]), x, y, 1, 1.0, 1e-6)
    assert np.max(np.abs(g["x"] - ref)) <= 1e-6 * np.max(np.abs(ref))
    lf1 = LatentGP(GP(base._kernel(0, 1.3, [0.7])), BernoulliLikelihood(), 1e-6)
    _, g1 = approx_lml_and_gradient(la, lf1(x[0]), y, ctx=ctx, wrt_inputs=True)
    assert g1["x"].shape == (40,)
    assert "x" not in approx_lml_and_gradient(la, lf1(x[0]), y, ctx=ctx)[1]
