"""GPU checks of the input gradient of the exact GP by conjugate gradients (csrc/cg_xgrad.hip; svgp_cg_lml_grad_inputs) against the
float64 restatement tests/cg_xgrad_ref.py (itself pinned to central differences of the oracle's exact GP in tests/test_cg_xgrad_cpu.py).
Inputs are seeded as in tests/test_gpu_cg.py: x ~ U[-3, 3]^d (divided by sqrt(d) from d = 9 on, so that K is not the identity),
lengthscale 0.7, variance 1.3.

Shapes: N in {48, 65, 300} (no multiples of 32; one to five workgroups of points), T in {8, 16} (17 and 33 columns: two and three column
blocks), d in {1, 2, 8, 9, 17, 33} (every feature-register width, the coordinate blocks of 8 and of 4, the by-differences path of fp32 up to
d = 8), the three kernel families, both dtypes.

Bounds.  x_bar against the restatement: the project's contract for a gradient block, 1e-8 of the block's largest entry in fp64 and 1e-4 in
fp32, at tol = 1e-12 / 1e-5 as in tests/test_gpu_cg.py.  Unit probes against central differences: 1e-6.  Shifted fp32 (d = 9, x + 30): at
most 4 x the float32 restatement's own error.  The identities: sum_i x_bar[c, i] = 0 to the contract times the block's largest entry (N
roundings of at most eps each stay far below it), sum_i x_ic x_bar[c, i] = il_c d_inv_lengthscale[c] of the same call to the contract
times the largest entry of that block.  test_report_observed_errors prints every measured figure (profiles/cg/accuracy_xgrad.md
records a run on an MI355X)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import cg_precond_ref as pr
import cg_ref as cr
import cg_xgrad_ref as xr
import svgp_oracle as o
from approxgp import (GP, ConjugateGradients, CustomMean, DeviceConjugateGradients, SEKernel, _ffi, approx_lml_and_gradient, draw_probes)
from approxgp.kernels import ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, TransformedKernel

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
SE, M32, M52 = o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52
FAMILIES = [SE, M32, M52]
BASES = {SE: SEKernel, M32: Matern32Kernel, M52: Matern52Kernel}
VAR, LS = 1.3, 0.7
OBSERVED = {}   # name -> text of the measured figures (printed by the last test)
SCALARS = ("variance", "diag", "mean_const")


def _kernel(family, d):
    return ScaledKernel(TransformedKernel(BASES[family](), ARDTransform(np.full(d, 1.0 / LS))), VAR)


def _okernel(family, d, dtype=F64):
    il = np.full(d, 1.0 / LS).astype(dtype).astype(F64)
    return o.Kernel(family, float(dtype(VAR)), il)


def _contract(dtype):
    return (1e-8, 1e-12) if dtype == F64 else (1e-4, 1e-5)   # (the gradient blocks' bound, the solver's tol)


def _name(dtype):
    return np.dtype(dtype).name


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _xy(N, d, seed=0, shift=0.0):
    rng = np.random.default_rng(1000 + 7 * N + 13 * d + seed)
    x = rng.uniform(-3, 3, size=(d, N))
    if d >= 9:
        x = x / np.sqrt(d)
    y = np.sin(x.sum(0)) + 0.1 * rng.standard_normal(N)
    x = x + shift
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _same_but_x(g, h):
    return all(g[k] == h[k] for k in SCALARS) and np.array_equal(g["inv_lengthscale"], h["inv_lengthscale"])


def _identities(x, g, dtype):
    """-> (translation, scaling) residuals relative to the largest entry of x_bar / of il o d_inv_lengthscale"""
    xb = g["x"].astype(F64)
    il = np.full(x.shape[0], 1.0 / LS).astype(dtype).astype(F64)
    rhs = il * g["inv_lengthscale"]
    return float(np.abs(xb.sum(1)).max() / np.abs(xb).max()), float(np.abs((x.astype(F64) * xb).sum(1) - rhs).max() / np.abs(rhs).max())


# ---- 1. against the restatement: every instantiation ------------------------------------------------------------------------------
CASES = [(48, 1, 8, SE, F64), (65, 2, 16, M32, F64), (300, 9, 8, M52, F64), (65, 17, 16, SE, F64), (65, 33, 8, M32, F64), (300, 2, 16, M52, F64),
         (48, 1, 16, M32, F32), (300, 2, 8, SE, F32), (65, 8, 16, M52, F32), (300, 9, 16, M32, F32), (65, 17, 8, M52, F32), (48, 33, 16, SE, F32)]


@pytest.mark.parametrize("N,d,T,family,dtype", [pytest.param(*c, id=f"N{c[0]}_d{c[1]}_T{c[2]}_k{c[3]}_{_name(c[4])}") for c in CASES])
def test_input_gradient_against_the_restatement(ctx, N, d, T, family, dtype):
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    z = draw_probes(N, T, 4)
    c, tol = _contract(dtype)
    dev = DeviceConjugateGradients(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, mean_const=0.25, tol=tol, maxiter=2000)
        lml0, g0, info0 = dev.lml_grad(desc, z)
        lml, g, info = dev.lml_grad(desc, z, wrt_inputs=True)
        lml2, g2, _ = dev.lml_grad(desc, z, wrt_inputs=True)
        xt = torch.full((d, N), 7.0, dtype=torch.float64 if dtype == F64 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        lml3, g3, _ = dev.lml_grad(desc, z, wrt_inputs=True, x_grad_out=xt)
        on_dev = g3["x"].cpu().numpy()
        lml4, g4, _ = dev.lml_grad(desc, z)
    finally:
        dev.free()
    assert g["x"].shape == (d, N) and g["x"].dtype == dtype and g3["x"] is xt
    # every other output is bitwise lml_grad's, before and after; repeated calls and device memory are bitwise equal
    assert lml == lml0 == lml2 == lml3 == lml4 and _same_but_x(g, g0) and _same_but_x(g3, g0) and _same_but_x(g4, g0) and "x" not in g0
    assert info.quad == info0.quad and info.logdet == info0.logdet and info.iterations == info0.iterations
    assert np.array_equal(g["x"], g2["x"]), "two calls differ"
    assert np.array_equal(g["x"], on_dev), "host and device-memory outputs differ"
    r = xr.estimate(_okernel(family, d, dtype), x.astype(F64), float(dtype(0.1)), y.astype(F64) - 0.25, z, tol, 2000)
    ref = r["grad"]["x"]
    err = float(np.abs(g["x"].astype(F64) - ref).max() / np.abs(ref).max())
    tr, sc = _identities(x, g, dtype)
    OBSERVED[f"x_bar N{N} d{d} T{T} k{family} {_name(dtype)}"] = f"restatement {err:.2e}, translation {tr:.2e}, scaling {sc:.2e}"
    print(N, d, T, family, _name(dtype), OBSERVED[f"x_bar N{N} d{d} T{T} k{family} {_name(dtype)}"])
    assert info.converged == 1 and np.isfinite(g["x"]).all()
    assert err <= c, (err, c)
    assert tr <= c and sc <= c, (tr, sc)


# ---- 2. unit probes: the exact gradient --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_unit_probe_input_gradient_against_central_differences(ctx, family):
    N, d = 48, 2
    x, y = _xy(N, d)
    dev = DeviceConjugateGradients(ctx, x, y, F64)
    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, tol=1e-12, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, cr.unit_probes(N), wrt_inputs=True)   # 97 columns: seven column blocks
    finally:
        dev.free()
    fd = xr.central_differences(_okernel(family, d), x, 0.1, y)
    err = float(np.abs(g["x"] - fd).max() / np.abs(fd).max())
    OBSERVED[f"x_bar vs central differences k{family}"] = f"{err:.2e}"
    print(family, err)
    assert err <= 1e-6, err


# ---- 3. fp32 far from the origin ----------------------------------------------------------------------------------------------------
def test_shifted_fp32_input_gradient(ctx):
    """d = 9 in fp32 with x shifted by +30 per coordinate: |xs| ~ 130 against differences of order one.  x_bar is bounded by 4 x the
    float32 restatement's own error against the float64 restatement, on the same float32-rounded inputs."""
    N, d, T = 300, 9, 8
    x, y = _xy(N, d, shift=30.0)
    x, y = x.astype(F32), y.astype(F32)
    z = draw_probes(N, T, 4)
    dev = DeviceConjugateGradients(ctx, x, y, F32)
    try:
        desc, keep = dev.desc(_kernel(SE, d), 0.1, tol=1e-5, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, z, wrt_inputs=True)
    finally:
        dev.free()
    ok = _okernel(SE, d, F32)
    r64 = xr.estimate(ok, x.astype(F64), float(F32(0.1)), y.astype(F64), z, 1e-5, 2000)["grad"]["x"]
    r32 = xr.estimate(ok, x.astype(F64), float(F32(0.1)), y.astype(F64), z, 1e-5, 2000, dtype=F32)["grad"]["x"]
    e_dev = float(np.abs(g["x"].astype(F64) - r64).max() / np.abs(r64).max())
    e_ref = float(np.abs(r32 - r64).max() / np.abs(r64).max())
    OBSERVED["shifted fp32 d9 x_bar"] = f"device {e_dev:.2e}, float32 restatement {e_ref:.2e}, ratio {e_dev / max(e_ref, 1e-300):.2f}"
    print(OBSERVED["shifted fp32 d9 x_bar"])
    assert e_dev <= 4.0 * e_ref, (e_dev, e_ref)


# ---- 4. with the Nystrom preconditioner --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
def test_preconditioned_input_gradient(ctx, family, dtype):
    N, d, k, T = 300, 2, 32, 16
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    eps, xi = draw_probes(N, T, 4), draw_probes(k, T, np.random.default_rng([4, 1]))
    zp = np.ascontiguousarray(x[:, np.random.default_rng(5).choice(N, size=k, replace=False)])
    c, tol = _contract(dtype)
    dev = DeviceConjugateGradients(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, mean_const=0.25, tol=tol, maxiter=2000)
        dev.set_preconditioner(zp, 1e-4)
        lml0, g0, info0 = dev.lml_grad(desc, eps, probes_k=xi)
        lml, g, info = dev.lml_grad(desc, eps, probes_k=xi, wrt_inputs=True)
        lml2, g2, _ = dev.lml_grad(desc, eps, probes_k=xi, wrt_inputs=True)
    finally:
        dev.free()
    assert lml == lml0 == lml2 and _same_but_x(g, g0) and info.logdet == info0.logdet and np.array_equal(g["x"], g2["x"])
    r = xr.estimate_precond(_okernel(family, d, dtype), x.astype(F64), zp.astype(F64), float(dtype(0.1)), y.astype(F64) - 0.25, eps, xi, tol, 2000)
    err = float(np.abs(g["x"].astype(F64) - r["x"]).max() / np.abs(r["x"]).max())
    tr, sc = _identities(x, g, dtype)
    OBSERVED[f"x_bar preconditioned k{family} {_name(dtype)}"] = f"restatement {err:.2e}, translation {tr:.2e}, scaling {sc:.2e}"
    print(family, _name(dtype), OBSERVED[f"x_bar preconditioned k{family} {_name(dtype)}"])
    assert info.converged == 1
    assert err <= c, (err, c)
    assert tr <= c and sc <= c, (tr, sc)


# ---- 5. duplicated points -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,dtype", [(SE, F64), (M32, F32), (M52, F64)])
def test_duplicated_points_have_finite_equal_gradients(ctx, family, dtype):
    """points 3 and 40 coincide (with equal y and equal probe rows): r^2 between them is 0 up to rounding, where 2 g is finite and the
    coordinate difference exactly 0; their columns of x_bar agree to the contract (the diagonal's exact-zero rule gives the two rows of
    K different roundings of one entry, so not bitwise)."""
    N, d, T = 65, 2, 8
    x, y = _xy(N, d)
    x, y = x.astype(dtype).copy(), y.astype(dtype).copy()
    z = draw_probes(N, T, 4).copy()
    x[:, 40], y[40], z[40] = x[:, 3], y[3], z[3]
    c, tol = _contract(dtype)
    dev = DeviceConjugateGradients(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, tol=tol, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, z, wrt_inputs=True)
    finally:
        dev.free()
    xb = g["x"].astype(F64)
    assert np.isfinite(xb).all() and np.abs(xb[:, 3]).max() > 0
    assert np.abs(xb[:, 3] - xb[:, 40]).max() <= c * np.abs(xb).max(), (xb[:, 3], xb[:, 40])


# ---- 6. device-resident features and the Python layer -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_wrapped_device_features_and_the_dispatcher(ctx, dtype):
    N, d = 65, 2
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    z = draw_probes(N, 8, 0)
    tdt = torch.float64 if dtype == F64 else torch.float32
    ft = torch.from_numpy(np.ascontiguousarray(x)).cuda()   # (d, N) contiguous: feature-major, ld N
    yt = torch.from_numpy(y.copy()).cuda()
    out = torch.zeros((d, N), dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    data = _ffi.DeviceData.wrap(ctx, dtype, d, N, N, ft.data_ptr(), yt.data_ptr())
    dev = DeviceConjugateGradients(ctx, data=data)
    up = DeviceConjugateGradients(ctx, x, y, dtype)
    try:
        tol = _contract(dtype)[1]
        desc, keep = dev.desc(_kernel(M52, d), 0.1, tol=tol, maxiter=2000)
        lml_w, g_w, _ = dev.lml_grad(desc, z, wrt_inputs=True, x_grad_out=out)
        lml_u, g_u, _ = up.lml_grad(desc, z, wrt_inputs=True)
    finally:
        dev.free()
        up.free()
    assert data.h is not None   # borrowed, not freed
    data.free()
    assert lml_w == lml_u and _same_but_x(g_w, g_u) and np.array_equal(out.cpu().numpy(), g_u["x"])
    # the dispatcher: the same seed gives the same probes, so the same numbers; a plain vector x gives a vector
    cg = ConjugateGradients(tol=tol, maxiter=2000, n_probes=8, seed=0)
    lml_a, g_a = approx_lml_and_gradient(cg, GP(_kernel(M52, d))(x, 0.1), y, ctx=ctx, dtype=dtype, wrt_inputs=True)
    assert lml_a == lml_u and np.array_equal(g_a["x"], g_u["x"]) and set(g_a) == {"variance", "inv_lengthscale", "diag", "mean_const", "x"}
    lml_b, g_b = approx_lml_and_gradient(cg, GP(_kernel(M52, d))(x, 0.1), y, ctx=ctx, dtype=dtype)
    assert lml_b == lml_a and "x" not in g_b and _same_but_x(g_a, g_b)
    x1, y1 = _xy(48, 1)
    trend = lambda xx: 0.5 * np.asarray(xx) - 0.2
    lml_v, g_v = approx_lml_and_gradient(cg, GP(CustomMean(trend), _kernel(SE, 1))(x1[0], 0.1), y1 + trend(x1[0]), ctx=ctx, dtype=dtype, wrt_inputs=True)
    lml_k, g_k = approx_lml_and_gradient(cg, GP(_kernel(SE, 1))(x1[0], 0.1), y1, ctx=ctx, dtype=dtype, wrt_inputs=True)
    assert g_v["x"].shape == (48,) and g_v["x"].dtype == dtype
    # a CustomMean prior: the gradient of the kernel part alone, so that of the zero-mean GP on y - mean(x).  (fp64 only: there the
    # two right-hand sides differ by eps64, which the solve's cond ~ 1e3 leaves far below the contract; in fp32 they differ by eps32)
    if dtype == F64:
        np.testing.assert_allclose(g_v["x"], g_k["x"], atol=1e-8 * np.abs(g_k["x"]).max())


# ---- 7. statuses, then a healthy call on the same context --------------------------------------------------------------------------
def test_statuses_leave_the_context_healthy(ctx):
    N, d = 65, 2
    x, y = _xy(N, d)
    lib, h = ctx.lib, ctx.h
    ft = torch.from_numpy(x.copy()).cuda()
    yt = torch.from_numpy(y.copy()).cuda()
    torch.cuda.synchronize()
    data = _ffi.DeviceData.wrap(ctx, F64, d, N, N, ft.data_ptr(), yt.data_ptr())
    dev = DeviceConjugateGradients(ctx, data=data)
    k = _kernel(M32, d)
    desc, keep = dev.desc(k, 0.01, tol=1e-10, maxiter=2000)
    z = draw_probes(N, 2, 0)
    dp = C.POINTER(C.c_double)
    out, info = C.c_double(), _ffi.CGInfo()
    dv, dil = C.c_double(), np.zeros(d)
    xg = np.full((d, N), 7.0)

    def call(gx, T=2, probes_k=None, handle=None):
        return lib.svgp_cg_lml_grad_inputs(h, (handle or dev).h, C.byref(desc), None, T, z.ctypes.data_as(dp) if T else None, probes_k, C.byref(out),
                                           C.byref(info), C.byref(dv), dil.ctypes.data_as(dp), None, None, gx)

    def gxs(ptr=None, ld=N, on=0, res=0):
        return C.byref(_ffi.InputGrad(_ffi._ptr(xg) if ptr is None else ptr, ld, on, res))

    INV = _ffi.INVALID_ARG
    try:
        lml_ok, g_ok, _ = dev.lml_grad(desc, z, wrt_inputs=True)
        assert call(None) == INV and call(C.byref(_ffi.InputGrad(None, N, 0, 0))) == INV
        assert call(gxs(ld=N - 1)) == INV and call(gxs(on=2)) == INV and call(gxs(on=-1)) == INV and call(gxs(res=1)) == INV
        assert call(gxs(ptr=C.c_void_p(ft.data_ptr()), on=1)) == INV                       # the data's x itself
        assert call(gxs(ptr=C.c_void_p(ft.data_ptr() + 8 * (N + 3)), on=1)) == INV          # inside it
        assert call(gxs(), probes_k=z.ctypes.data_as(dp)) == INV                            # probes_k without a preconditioner
        assert call(gxs(), T=-1) == INV
        assert np.all(xg == 7.0), "a rejected call wrote its output"
        # T = 0: SVGP_OK, the trace blocks and x_bar are NaN
        assert call(gxs(), T=0) == _ffi.OK and np.isnan(xg).all() and np.isnan(dil).all() and info.quad == info.quad
        xt = torch.zeros((d, N), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _, g0, _ = dev.lml_grad(desc, None, wrt_inputs=True, x_grad_out=xt)
        assert torch.isnan(xt).all().item()
        # a NaN coordinate: SVGP_NOT_POSDEF, NaN in host and in device output
        xn = x.copy()
        xn[1, 7] = np.nan
        bad = DeviceConjugateGradients(ctx, xn, y, F64)
        try:
            xg[:] = 7.0
            assert call(gxs(), handle=bad) == _ffi.NOT_POSDEF and np.isnan(xg).all() and np.isnan(out.value)
            xt.zero_()
            torch.cuda.synchronize()
            with pytest.raises(_ffi.PosDefException):
                bad.lml_grad(desc, z, wrt_inputs=True, x_grad_out=xt)
            assert torch.isnan(xt).all().item()
        finally:
            bad.free()
        # and a healthy call afterwards: bitwise the first
        lml_h, g_h, inf = dev.lml_grad(desc, z, wrt_inputs=True)
        assert inf.converged == 1 and lml_h == lml_ok and np.array_equal(g_h["x"], g_ok["x"]) and _same_but_x(g_h, g_ok)
    finally:
        dev.free()
        data.free()


def test_report_observed_errors():
    """Prints the table profiles/cg/accuracy_xgrad.md records (run the module with -s); SVGP_CG_XGRAD_ACCURACY_MD=path also writes it."""
    lines = ["| check | measured |", "|---|---|"] + [f"| {name} | {text} |" for name, text in OBSERVED.items()]
    print("\n".join(lines))
    path = os.environ.get("SVGP_CG_XGRAD_ACCURACY_MD")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
