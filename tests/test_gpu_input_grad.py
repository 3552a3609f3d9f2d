"""GPU checks of d elbo / d x (svgp_elbo_grad_inputs / svgp_elbo_grad_ext_inputs, csrc/grad.hip: xgrad_mfma_kernel) against the
float64 reference of tests/input_grad_ref.py (itself pinned by finite differences in tests/test_input_grad_cpu.py).
Tolerances, relative to the block's largest entry: fp64 1e-9, fp32 5e-4 (the header's z / lengthscale tolerance)."""
import ctypes as C

import numpy as np
import pytest

import svgp_oracle as o
from approxgp import _ffi
from helpers import context_with_env, device_model
from input_grad_ref import input_grad

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-9, np.float32: 5e-4}
LIKS = [(o.LIK_GAUSSIAN, 0), (o.LIK_BERNOULLI_LOGISTIC, 0), (o.LIK_BERNOULLI_NORMCDF, 0), (o.LIK_POISSON_EXP, 0),
        (o.LIK_EXPONENTIAL_EXP, 0), (o.LIK_GAMMA_EXP, 0), (o.LIK_GAUSSIAN, 9)]
LAYOUTS = (_ffi.COLVECS, _ffi.ROWVECS, _ffi.VEC)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= tol * scale, (np.abs(a - b).max(), scale)


def _upload(ctx, x, y, dtype, layout):
    """x (d, n) in the given layout -> (DeviceData, how to bring the returned x_bar back to (d, n))."""
    if layout == _ffi.VEC:
        assert x.shape[0] == 1
        return _ffi.DeviceData(ctx, x[0], y, dtype), lambda g: np.asarray(g)[None, :]
    if layout == _ffi.ROWVECS:
        return _ffi.DeviceData(ctx, np.ascontiguousarray(x.T), y, dtype, layout=_ffi.ROWVECS), lambda g: np.asarray(g).T
    return _ffi.DeviceData(ctx, x, y, dtype), lambda g: np.asarray(g)


def _problem(seed, N, M, d, family=o.KERNEL_SE, lik=o.LIK_GAUSSIAN, dtype=np.float64, centered=False):
    x, y, nc, s2 = o.synth_problem(seed, N, M, d, family=family, lik=lik, dtype=dtype)
    ils = np.linspace(0.8, 1.3, d) * np.asarray(nc.kernel.inv_lengthscale, dtype=np.float64)
    ils = ils.astype(dtype).astype(np.float64)
    k = o.Kernel(family, nc.kernel.variance, ils)
    sva = o.SVA(k, nc.z, nc.m, nc.Lq, jitter=nc.jitter, mean_const=0.15)
    if centered:   # the Centered form of a well-conditioned whitened posterior: m = c + Lk m~, Lq = Lk (0.8 B)
        Lk = np.linalg.cholesky(o.kuu(sva))
        rnd = lambda a: np.asarray(a).astype(dtype).astype(np.float64)
        sva = o.SVA(k, nc.z, rnd(0.15 + Lk @ nc.m), rnd(np.tril(Lk @ (0.8 * nc.Lq))), jitter=nc.jitter, mean_const=0.15, centered=True)
    return x, y, sva, s2


def _xbar(ctx, x, y, sva, s2, dtype, num_data):
    model = device_model(ctx, sva, dtype=dtype, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, dtype)
    try:
        return model.elbo_grad(data, 0, x.shape[1], num_data, inputs=True)[2]["x"]
    finally:
        model.free()
        data.free()


def _check(ctx, x, y, sva, s2, dtype, lik=o.LIK_GAUSSIAN, qn=0, layout=_ffi.COLVECS, off=0, n=None, num_data=None):
    d, N = x.shape
    n = N - off if n is None else n
    nd = float(num_data) if num_data is not None else 2.5 * N
    model = device_model(ctx, sva, dtype=dtype, lik=lik, sigma2=s2, quadrature_n=qn)
    data, back = _upload(ctx, x, y, dtype, layout)
    try:
        _, _, g = model.elbo_grad(data, off, n, nd, inputs=True)
        ref = input_grad(sva, x[:, off:off + n], y[off:off + n], lik=lik, sigma2=s2, num_data=nd, quadrature_n=qn)
        got = back(g["x"])
        assert got.shape == ref.shape
        _close(got, ref, TOL[dtype])
        return g
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
@pytest.mark.parametrize("lik,qn", LIKS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_parity_family_likelihood(ctx, family, lik, qn, dtype):
    i = 3 * LIKS.index((lik, qn)) + family
    layout = LAYOUTS[i % 3]
    d = 1 if layout == _ffi.VEC else 3
    x, y, sva, s2 = _problem(500 + i, 901, 64, d, family=family, lik=lik, dtype=dtype, centered=bool(i % 2))
    _check(ctx, x, y, sva, s2, dtype, lik, qn, layout, off=37, n=801)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("centered", [False, True])
def test_parity_layout_parametrization(ctx, layout, centered):
    d = 1 if layout == _ffi.VEC else 5
    for dtype in (np.float64, np.float32):
        x, y, sva, s2 = _problem(540 + d, 700, 40, d, family=o.KERNEL_MATERN52, lik=o.LIK_POISSON_EXP, dtype=dtype, centered=centered)
        _check(ctx, x, y, sva, s2, dtype, o.LIK_POISSON_EXP, 0, layout)


@pytest.mark.parametrize("d", [1, 2, 3, 8, 9, 16, 17, 32, 64])
@pytest.mark.parametrize("M", [1, 15, 64, 129, 640])
def test_parity_shapes(ctx, d, M):
    for dtype in (np.float64, np.float32):
        if dtype == np.float32 and M == 640 and d < 8:
            continue   # 640 inducing points on few input dimensions: Kuu is beyond fp32's Cholesky at the default jitter
        fam = (o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52)[(d + M) % 3]
        x, y, sva, s2 = _problem(600 + d + M, 1000 + 3 * d, M, d, family=fam, dtype=dtype)
        _check(ctx, x, y, sva, s2, dtype, off=5, n=1000 + 3 * d - 11)


def test_two_chunks_and_window(ctx):
    """N > 131 072 points: the gradient runs in 65 536-point chunks (x_bar of each chunk behind its own kernel-gradient reduction)."""
    N, M, d = 140_000, 128, 3
    x, y, sva, s2 = _problem(77, N, M, d, family=o.KERNEL_MATERN32)
    _check(ctx, x, y, sva, s2, np.float64, num_data=float(N))
    _check(ctx, x, y, sva, s2, np.float64, off=70_001, n=66_000, num_data=float(N))


def test_other_outputs_bitwise_and_repeatable(ctx):
    for dtype, lik in ((np.float64, o.LIK_GAUSSIAN), (np.float32, o.LIK_BERNOULLI_LOGISTIC), (np.float64, o.LIK_GAMMA_EXP)):
        x, y, sva, s2 = _problem(81, 3000, 200, 6, lik=lik, dtype=dtype)
        model = device_model(ctx, sva, dtype=dtype, lik=lik, sigma2=s2)
        data = _ffi.DeviceData(ctx, x, y, dtype)
        v0, t0, g0 = model.elbo_grad(data, 10, 2900, 9000.0)
        runs = [model.elbo_grad(data, 10, 2900, 9000.0, inputs=True) for _ in range(3)]
        for v, t, g in runs:
            assert v == v0
            assert bytes(t) == bytes(t0)
            for k in ("variance", "lik_sigma2", "mean_const"):
                assert g[k] == g0[k], k
            for k in ("inv_lengthscale", "z", "m", "Lq"):
                assert np.array_equal(g[k], g0[k]), k
            assert np.array_equal(g["x"], runs[0][2]["x"])
        model.free()
        data.free()


def test_far_from_origin(ctx):
    """x and z shifted together by 1e3 lengthscales: x_bar does not change (the kernel centres the points)."""
    N, M, d = 2000, 100, 4
    x, y, sva, s2 = _problem(88, N, M, d, family=o.KERNEL_MATERN52)
    shift = (1e3 / sva.kernel.inv_lengthscale)[:, None]
    g0 = _check(ctx, x, y, sva, s2, np.float64)["x"]
    xs, zs = x + shift, sva.z + shift
    moved = o.SVA(sva.kernel, zs, sva.m, sva.Lq, jitter=sva.jitter, mean_const=sva.mean_const)
    _close(_xbar(ctx, xs, y, moved, s2, np.float64, 2.5 * N), g0, 1e-8)
    # fp32, against the fp64 reference of the shifted problem rounded through fp32.  At 1e3 lengthscales the fp32 FORWARD path (Kuu, the
    # strips' Kuf, whose distances are not centred) has lost the posterior before x_bar is formed, so fp32 is held to its
    # tolerance at 10 lengthscales from the origin
    xs, zs = x + 1e-2 * shift, sva.z + 1e-2 * shift
    x32, z32 = xs.astype(np.float32).astype(np.float64), zs.astype(np.float32).astype(np.float64)
    m32 = o.SVA(sva.kernel, z32, sva.m.astype(np.float32).astype(np.float64), sva.Lq.astype(np.float32).astype(np.float64),
                jitter=1e-3, mean_const=sva.mean_const)
    _check(ctx, x32, y, m32, s2, np.float32)


def test_device_output_into_torch(ctx):
    import torch
    N, M, d = 5000, 128, 4
    x, y, sva, s2 = _problem(90, N, M, d, family=o.KERNEL_MATERN32)
    stream = torch.cuda.current_stream()
    tctx = _ffi.Context(0, stream.cuda_stream)
    try:
        xt = torch.tensor(x, dtype=torch.float64, device="cuda")              # (d, n): feature-major, ldx = n
        yt = torch.tensor(y, dtype=torch.float64, device="cuda")
        model = device_model(tctx, sva, sigma2=s2)
        data = _ffi.DeviceData.wrap(tctx, np.float64, d, N, N, xt.data_ptr(), yt.data_ptr())
        ld = N + 37
        out = torch.full((d, ld), -7.25, dtype=torch.float64, device="cuda")
        v_dev, _, g_dev = model.elbo_grad(data, 0, N, 2.0 * N, inputs=(out.data_ptr(), ld))
        assert "x" not in g_dev
        _, _, g_host = model.elbo_grad(data, 0, N, 2.0 * N, inputs=True)
        assert g_host["x"].shape == (N, d)                                   # wrapped device data: RowVecs layout
        torch.cuda.synchronize()
        o_np = out.cpu().numpy()
        assert np.array_equal(o_np[:, :N], g_host["x"].T)
        assert np.all(o_np[:, N:] == -7.25)
        _close(o_np[:, :N], input_grad(sva, x, y, sigma2=s2, num_data=2.0 * N), 1e-9)
        model.free()
        data.free()
    finally:
        tctx.close()


def test_caller_likelihood_matches_builtin(ctx):
    N, M, d = 2500, 90, 3
    x, y, sva, s2 = _problem(93, N, M, d, lik=o.LIK_POISSON_EXP)
    model = device_model(ctx, sva, lik=o.LIK_POISSON_EXP, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    _, _, g_in = model.elbo_grad(data, 100, 2000, 7000.0, inputs=True)
    mu, var = model.marginals(data, 100, 2000)
    yb = y[100:2100]
    e_host = o.expected_loglik(o.LIK_POISSON_EXP, mu, np.sqrt(var), yb, s2)
    gmu, gv, _ = o.expected_loglik_grads(o.LIK_POISSON_EXP, mu, var, yb, s2)
    _, _, g_ext = model.elbo_grad(data, 100, 2000, 7000.0, ext=(e_host, gmu, gv), inputs=True)
    _close(g_ext["x"], g_in["x"], 1e-12)
    _close(g_ext["x"], input_grad(sva, x[:, 100:2100], None, num_data=7000.0, point_grads=(e_host, gmu, gv)), 1e-9)
    model.free()
    data.free()


def test_overlap_setting_gives_identical_bits():
    x, y, sva, s2 = _problem(95, 6000, 256, 8)
    res = []
    for ov in (0, 1):
        with context_with_env(SVGP_OVERLAP=ov) as c:
            model = device_model(c, sva, sigma2=s2)
            data = _ffi.DeviceData(c, x, y, np.float64)
            res.append(model.elbo_grad(data, 0, 6000, 6000.0, inputs=True)[2]["x"])
            model.free()
            data.free()
    assert np.array_equal(res[0], res[1])


def test_collective_world_of_one():
    x, y, sva, s2 = _problem(97, 3001, 96, 3, family=o.KERNEL_MATERN52)
    c = _ffi.Context(0)
    try:
        model = device_model(c, sva, sigma2=s2)
        data = _ffi.DeviceData(c, x, y, np.float64)
        lv, _, lg = model.elbo_grad(data, 100, 1500, 9000.0, inputs=True)
        c.attach_comm(_ffi.comm_unique_id(), 1, 0)
        gv, _, gg = model.elbo_grad(data, 100, 1500, 9000.0, inputs=True)
        assert abs(gv - lv) <= 1e-12 * abs(lv)
        np.testing.assert_allclose(gg["x"], lg["x"], rtol=1e-12, atol=1e-13 * np.abs(lg["x"]).max())
        with pytest.raises(ValueError):   # an argument error goes through the opening handshake and comes back as itself
            model.elbo_grad(data, 100, 1500, 9000.0, inputs=(0, 1500))
        g2 = model.elbo_grad(data, 100, 1500, 9000.0, inputs=True)[2]
        assert np.array_equal(g2["x"], gg["x"])
        model.free()
        data.free()
    finally:
        c.close()


def test_nan_point_stays_in_its_column(ctx):
    N, M, d = 1200, 64, 3
    x, y, sva, s2 = _problem(99, N, M, d)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    g_fin = model.elbo_grad(data, 0, N, 0.0, inputs=True)[2]["x"]
    data.free()
    xn = x.copy()
    xn[1, 417] = np.nan
    data = _ffi.DeviceData(ctx, xn, y, np.float64)
    _, _, g = model.elbo_grad(data, 0, N, 0.0, inputs=True)
    assert np.isnan(g["x"][:, 417]).all()
    keep = np.ones(N, dtype=bool)
    keep[417] = False
    assert np.isfinite(g["x"][:, keep]).all()
    _close(g["x"][:, keep], g_fin[:, keep], 1e-12)
    model.free()
    data.free()


def test_bad_arguments(ctx):
    import torch
    N, M, d = 800, 32, 2
    x, y, sva, s2 = _problem(101, N, M, d)
    model = device_model(ctx, sva, sigma2=s2)
    xt = torch.tensor(x, dtype=torch.float64, device="cuda")
    yt = torch.tensor(y, dtype=torch.float64, device="cuda")
    data = _ffi.DeviceData.wrap(ctx, np.float64, d, N, N, xt.data_ptr(), yt.data_ptr())
    lib = ctx.lib
    buf = np.zeros((d, N))
    dev = torch.zeros((d, N), dtype=torch.float64, device="cuda")
    bad = [None,
           _ffi.InputGrad(None, N, 0, 0),                                    # NULL x
           _ffi.InputGrad(buf.ctypes.data_as(C.c_void_p), N - 1, 0, 0),      # ld < batch_len
           _ffi.InputGrad(buf.ctypes.data_as(C.c_void_p), N, 2, 0),          # on_device not 0 / 1
           _ffi.InputGrad(buf.ctypes.data_as(C.c_void_p), N, 0, 1),          # reserved != 0
           _ffi.InputGrad(C.c_void_p(xt.data_ptr() + 8 * 100), N, 1, 0),     # device output overlapping x
           _ffi.InputGrad(C.c_void_p(dev.data_ptr()), N, 1, 7)]
    gmu = np.zeros(N)
    for gx in bad:
        out, terms = C.c_double(), _ffi.Terms()
        il, zb, mb, Lb = np.zeros(d), np.zeros((d, M)), np.zeros(M), np.zeros((M, M))
        g = _ffi.Grads(0, 0, 0, il.ctypes.data_as(C.POINTER(C.c_double)), zb.ctypes.data_as(C.c_void_p), mb.ctypes.data_as(C.c_void_p),
                       Lb.ctypes.data_as(C.c_void_p))
        p = C.byref(gx) if gx is not None else None
        assert lib.svgp_elbo_grad_inputs(ctx.h, model.h, data.h, 0, N, 0.0, C.byref(out), C.byref(terms), C.byref(g), p) == _ffi.INVALID_ARG
        assert lib.svgp_elbo_grad_ext_inputs(ctx.h, model.h, data.h, 0, N, 0.0, 0.0, gmu.ctypes.data_as(C.c_void_p),
                                             gmu.ctypes.data_as(C.c_void_p), C.byref(out), C.byref(terms), C.byref(g), p) == _ffi.INVALID_ARG
    torch.cuda.synchronize()
    assert np.array_equal(xt.cpu().numpy(), x)                                # nothing was written into the data
    _, _, g = model.elbo_grad(data, 0, N, 0.0, inputs=True)                  # the context is healthy afterwards
    _close(g["x"].T, input_grad(sva, x, y, sigma2=s2), 1e-9)
    model.free()
    data.free()


def test_python_api_wrt_inputs(ctx):
    import approxgp as ag

    rng = np.random.default_rng(11)
    N, M = 1500, 40
    for d in (3, 1, 0):   # ColVecs (d, n), a 1 x n ColVecs, a plain vector
        dd = max(d, 1)
        xr = rng.uniform(-2, 2, (dd, N))
        x = xr if d > 0 else xr[0]
        y = np.sin(xr.sum(0)) + 0.1 * rng.standard_normal(N)
        z = xr[:, :M].copy() if d > 0 else xr[0, :M].copy()
        A = np.eye(M) + 0.01 * np.tril(rng.standard_normal((M, M)))
        mvec = 0.1 * rng.standard_normal(M)
        f = ag.GP(1.3 * ag.with_lengthscale(ag.Matern32Kernel(), 0.7))
        sva = ag.SparseVariationalApproximation(f(z, 1e-5), ag.MvNormal.from_cholesky(mvec, A))
        val, g = ag.elbo_and_gradient(sva, f(x, 0.3), y, num_data=3 * N, ctx=ctx, wrt_inputs=True)
        assert g["x"].shape == np.shape(x)
        osva = o.SVA(o.Kernel(o.KERNEL_MATERN32, 1.3, np.full(dd, 1 / 0.7)), np.reshape(z, (dd, M)), mvec, A, jitter=1e-5)
        _close(np.reshape(g["x"], (dd, N)), input_grad(osva, np.reshape(x, (dd, N)), y, sigma2=0.3, num_data=3 * N), 1e-9)
        _, g0 = ag.elbo_and_gradient(sva, f(x, 0.3), y, num_data=3 * N, ctx=ctx)
        assert "x" not in g0 and np.array_equal(g0["z"], g["z"])
