"""GPU checks of svgp_nn_lml_grad_inputs (csrc/nn_xgrad.hip): d lml / d x of the NearestNeighbors approximation at the fixed
conditioning sets against tests/nn_xgrad_ref.py (float64 torch autograd).  Shapes, inputs and the cycling of d, layout, dtype and
family are test_gpu_nn_noise.cases(): every (N, k) pair of N in {1, 2, 17, 65, 130, 301} x k in {3, 16, 17, 33, 64} once, both
vectors set, for the window, the device-built nearest table and a random table.  Tolerances are the suite's for gradients: 1e-6
(fp64) / 1e-3 (fp32) of the largest entry of x_bar; the scaling identity in fp64 to 1e-6 of sum |x x_bar|.  Measured worst cases:
profiles/nn/accuracy_xgrad.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import nn_noise_ref as nn
import nn_ref as nr
import nn_sets_ref as ns
import nn_xgrad_ref as nx
import svgp_oracle as o
from approxgp import GP, DeviceNearestNeighbors, Diagonal, NearestNeighbors, _ffi, approx_lml_and_gradient
from test_gpu_nn_noise import DIAG, MC, VAR, _dev, _hub_problem, _kernel, cases, inputs

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _check(dev, desc, kern, x64, y64, tab, s64, mu64, dtype, what, diag=DIAG):
    """one handle state: x_bar against the restatement, and every bitwise contract of the call -> the error of the largest entry"""
    d, n = x64.shape
    l0, g0, _ = dev.lml_grad_points(desc)
    l1, g1, _ = dev.lml_grad_points(desc, wrt_inputs=True)
    l2, g2, _ = dev.lml_grad_points(desc, wrt_inputs=True)
    xt = torch.full((d, n), 7.0, device="cuda", dtype=torch.float64 if dtype == F64 else torch.float32)
    l3, g3, _ = dev.lml_grad_points(desc, wrt_inputs=True, x_grad_out=xt)
    assert g3["x"] is xt and g1["x"].shape == (d, n) and g1["x"].dtype == dtype
    assert l0 == l1 == l2 == l3, what
    for key in ("variance", "diag", "mean_const", "inv_lengthscale", "mean", "noise"):
        assert np.array_equal(g0[key], g1[key]) and np.array_equal(g0[key], g3[key]), (what, key)
    assert np.array_equal(g1["x"], g2["x"]) and np.array_equal(g1["x"], xt.cpu().numpy()), what
    _, ref = nx.lml_and_xbar(kern, x64, y64, tab, diag, s64, mu64, MC)
    scale = np.max(np.abs(ref))
    err = np.max(np.abs(g1["x"] - ref)) / scale if scale > 0 else float(np.max(np.abs(g1["x"])))
    tol = 1e-6 if dtype == F64 else 1e-3
    print(f"{what}: x_bar {err:.2e} (allowed {tol:.0e})")
    assert err <= tol, what
    if dtype == F64:   # the scaling identity ties x_bar to the returned d_inv_lengthscale
        xx = x64 * g1["x"]
        assert np.max(np.abs(xx.sum(axis=1) - kern.inv_lengthscale * g1["inv_lengthscale"])) <= 1e-6 * max(np.sum(np.abs(xx)), 1e-300), what
    return err


@pytest.mark.parametrize("n,k,d,layout,dtype,fam", cases())
def test_x_bar_matches_the_restatement(ctx, n, k, d, layout, dtype, fam):
    (x, y, s, mu), (x64, y64, s64, mu64) = inputs(n, k, d, dtype)
    il = nr.invl_for(d, True)
    kern = nr.kernel_of(fam, VAR, il)
    dev = _dev(ctx, x, y, dtype, layout)
    desc, keep = dev.desc(_kernel(fam, VAR, il), k, DIAG, MC)
    dev.set_noise(s)
    dev.set_mean(mu)
    for form in ("window", "nearest", "random"):
        if form == "window":
            tab = ns.window_table(n, k)
        elif form == "nearest":
            dev.build_neighbors(k, il)
            tab = dev.neighbors()
        else:
            tab = nn.random_table(n, k, n + k)
            dev.set_neighbors(tab)
        _check(dev, desc, kern, x64, y64, tab, s64, mu64, dtype, f"n {n} k {k} d {d} fam {fam} {np.dtype(dtype).name} {form}")
    dev.free()


def test_no_vectors_set(ctx):
    n, k, d = 65, 16, 3
    (x, y, _, _), (x64, y64, _, _) = inputs(n, k, d, F64)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, F64)
    desc, keep = dev.desc(_kernel(o.KERNEL_MATERN32, VAR, il), k, DIAG, MC)
    kern = nr.kernel_of(o.KERNEL_MATERN32, VAR, il)
    _check(dev, desc, kern, x64, y64, ns.window_table(n, k), None, None, F64, "no vectors, window")
    tab = nn.random_table(n, k, 5)
    dev.set_neighbors(tab)
    _check(dev, desc, kern, x64, y64, tab, None, None, F64, "no vectors, random table")
    dev.free()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_hub_table_strides_the_reverse_lists(ctx, dtype):
    """point 0 is named by 129 > 64 pairs: the lanes of its gather stride the list"""
    n, k, d, (x, y, s, mu), (x64, y64, s64, mu64), tab = _hub_problem(dtype)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, dtype)
    desc, keep = dev.desc(_kernel(o.KERNEL_MATERN52, VAR, il), k, DIAG, MC)
    dev.set_neighbors(tab)
    dev.set_noise(s)
    dev.set_mean(mu)
    _check(dev, desc, nr.kernel_of(o.KERNEL_MATERN52, VAR, il), x64, y64, tab, s64, mu64, dtype, f"hub table {np.dtype(dtype).name}")
    dev.free()


@pytest.mark.parametrize("fam", [o.KERNEL_SE, o.KERNEL_MATERN32])
def test_coincident_points_inside_a_block(ctx, fam):
    n, k, d = 40, 8, 2
    x, y = nr.synth(n, d, seed=11)
    x[:, 21] = x[:, 19]
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, F64)
    desc, keep = dev.desc(_kernel(fam, VAR, il), k, 1e-2, MC)
    err = _check(dev, desc, nr.kernel_of(fam, VAR, il), x, y, ns.window_table(n, k), None, None, F64, f"coincident fam {fam}", diag=1e-2)
    assert np.isfinite(err) and np.all(np.isfinite(dev.lml_grad_points(desc, wrt_inputs=True)[1]["x"]))
    dev.free()


def test_not_positive_definite_fills_nan_and_the_context_stays_healthy(ctx):
    n, k, d = 40, 8, 2
    x, y = nr.synth(n, d, seed=12)
    x[:, 21] = x[:, 19]   # a singular block without a diagonal term
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, F64)
    desc, keep = dev.desc(_kernel(o.KERNEL_SE, VAR, il), k, 0.0, MC)
    xt = torch.zeros((d, n), device="cuda", dtype=torch.float64)
    for out in (None, xt):
        with pytest.raises(_ffi.PosDefException) as e:
            dev.lml_grad_points(desc, wrt_inputs=True, x_grad_out=out)
        assert e.value.info in (22, 23)   # point 21 (F = 0), or the first block that holds both copies
        assert np.all(np.isnan(e.value.x_grad if out is None else xt.cpu().numpy()))
    desc2, keep2 = dev.desc(_kernel(o.KERNEL_SE, VAR, il), k, 1e-2, MC)
    assert np.all(np.isfinite(dev.lml_grad_points(desc2, wrt_inputs=True)[1]["x"]))
    dev.free()


def test_invalid_gx_arguments(ctx):
    n, k, d = 17, 3, 3
    (x, y, _, _), _ = inputs(n, k, d, F64)
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")   # torch features used in place
    data = _ffi.DeviceData.wrap(ctx, F64, d, n, n, xd.data_ptr(), yd.data_ptr())
    dev = DeviceNearestNeighbors(ctx, data=data)
    desc, keep = dev.desc(_kernel(o.KERNEL_SE, VAR, nr.invl_for(d, True)), k, DIAG, MC)
    lml, info, dv, dd, dm, dil = C.c_double(), _ffi.NNInfo(), C.c_double(), C.c_double(), C.c_double(), np.zeros(d)
    buf = np.zeros((d, n))
    xt = torch.zeros((d, n), device="cuda", dtype=torch.float64)
    sb = torch.zeros(n, device="cuda", dtype=torch.float64)
    gpn = _ffi.PointNoiseGrad(C.c_void_p(sb.data_ptr()), 1, 0)

    def call(gx, gpn=None):
        return ctx.lib.svgp_nn_lml_grad_inputs(ctx.h, dev.h, C.byref(desc), C.byref(lml), C.byref(info), C.byref(dv),
                                               dil.ctypes.data_as(C.POINTER(C.c_double)), C.byref(dd), C.byref(dm), None,
                                               None if gpn is None else C.byref(gpn), None if gx is None else C.byref(gx))

    bad = [None, _ffi.InputGrad(None, n, 0, 0), _ffi.InputGrad(_ffi._ptr(buf), n - 1, 0, 0), _ffi.InputGrad(_ffi._ptr(buf), n, 2, 0),
           _ffi.InputGrad(_ffi._ptr(buf), n, 0, 1), _ffi.InputGrad(C.c_void_p(xd.data_ptr() + 8 * n), n, 1, 0),
           _ffi.InputGrad(C.c_void_p(yd.data_ptr()), n, 1, 0)]
    for gx in bad:
        assert call(gx) == _ffi.INVALID_ARG
    assert call(_ffi.InputGrad(C.c_void_p(sb.data_ptr()), n, 1, 0), gpn) == _ffi.INVALID_ARG   # x_bar over the s_bar output
    assert call(_ffi.InputGrad(C.c_void_p(xt.data_ptr()), n, 1, 0), gpn) == _ffi.OK
    ref = nx.lml_and_xbar(nr.kernel_of(o.KERNEL_SE, VAR, nr.invl_for(d, True)), x, y, ns.window_table(n, k), DIAG, None, None, MC)[1]
    assert np.max(np.abs(xt.cpu().numpy() - ref)) <= 1e-6 * np.max(np.abs(ref))
    xd.mul_(0.5)   # an in-place update of the wrapped features is seen by the next call
    assert call(_ffi.InputGrad(C.c_void_p(xt.data_ptr()), n, 1, 0)) == _ffi.OK
    ref = nx.lml_and_xbar(nr.kernel_of(o.KERNEL_SE, VAR, nr.invl_for(d, True)), 0.5 * x, y, ns.window_table(n, k), DIAG, None, None, MC)[1]
    assert np.max(np.abs(xt.cpu().numpy() - ref)) <= 1e-6 * np.max(np.abs(ref))
    dev.free()
    data.free()


@pytest.mark.parametrize("shape", ["colvecs", "rowvecs", "vector"])
def test_approx_lml_and_gradient_returns_x_in_the_shape_of_fx(ctx, shape):
    n, k, d = 65, 16, 1 if shape == "vector" else 3
    (x, y, s, mu), (x64, y64, s64, mu64) = inputs(n, k, d, F64)
    il = nr.invl_for(d, True)
    gp = GP(MC, _kernel(o.KERNEL_SE, VAR, il))
    xa = x[0] if shape == "vector" else (x.T.copy() if shape == "rowvecs" else x)
    kw = dict(layout=_ffi.ROWVECS) if shape == "rowvecs" else {}
    lml, g = approx_lml_and_gradient(NearestNeighbors(k, include_noise=True, neighbors="nearest"), gp(xa, Diagonal(DIAG + s64)), y,
                                     ctx=ctx, mean_offsets=mu64, wrt_inputs=True, **kw)
    assert g["x"].shape == xa.shape
    _, ref = nx.lml_and_xbar(nr.kernel_of(o.KERNEL_SE, VAR, il), x64, y64, ns.nearest_table(x64, k, il), DIAG, s64, mu64, MC)
    got = g["x"][None, :] if shape == "vector" else (g["x"].T if shape == "rowvecs" else g["x"])
    assert np.max(np.abs(got - ref)) <= 1e-6 * np.max(np.abs(ref))
