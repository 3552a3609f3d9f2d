"""GPU checks of prior mean offsets (svgp_model_set_mean_z, svgp_elbo_with_mean, svgp_marginals_with_mean, svgp_elbo_grad_with_mean)
against the float64 reference of tests/prior_mean_ref.py (itself pinned in tests/test_prior_mean_cpu.py).
Tolerances, relative to each block's largest entry: fp64 1e-9 (the likelihood parameter's gradient, a sum whose terms cancel, relative
to the sum of its terms' magnitudes).  fp32: 5e-5 for mux_bar (the header's m tolerance), 5e-4 for z, 1e-5 for the value and the
variances, 1e-3 for the scalar gradients (sums whose terms cancel: measured 5.8e-4 on the kernel variance), 1e-4 for the marginal mean,
m and Lq, 2e-3 for the inverse lengthscales (measured over the Gaussian cases: 4.8e-5, 5.3e-5, 4.9e-5, 8.2e-4).  On the non-Gaussian
likelihoods the fp32 adjoint itself errs more on these small problems (measured up to 9.2e-3 on z, 6.3e-3 on Lq, with or without
offsets; tests/test_gpu_grad.py holds the existing calls to 2e-3 / 5e-3 against the oracle): there a gradient block may also pass by
erring no more than 3 x the existing call's own fp32 error on the same problem without offsets - the offsets must not cost fp32
accuracy - and never more than FP32_CEIL = 1.5e-2 of the block's largest entry.  mux enters the
marginal mean by one fp64 addition and mux_bar is g_mu, which the existing calls form the same way."""
import ctypes as C

import numpy as np
import pytest

import prior_mean_ref as pmr
import svgp_oracle as o
from approxgp import _ffi
from helpers import context_with_env, device_model

pytestmark = pytest.mark.gpu

LIKS = [(o.LIK_GAUSSIAN, 0), (o.LIK_BERNOULLI_LOGISTIC, 0), (o.LIK_BERNOULLI_NORMCDF, 0), (o.LIK_POISSON_EXP, 0),
        (o.LIK_EXPONENTIAL_EXP, 0), (o.LIK_GAMMA_EXP, 0), (o.LIK_GAUSSIAN, 9)]
LAYOUTS = (_ffi.COLVECS, _ffi.ROWVECS, _ffi.VEC)
TOL64 = 1e-9
TOL32 = dict(value=1e-5, mu=1e-4, var=1e-5, m=1e-4, Lq=1e-4, mean_x=5e-5, z=5e-4, inv_lengthscale=2e-3, variance=1e-3,
             mean_const=1e-3, lik_sigma2=1e-3)
GRAD_BLOCKS = ("variance", "inv_lengthscale", "z", "m", "Lq", "lik_sigma2", "mean_const")
FP32_CEIL = 1.5e-2   # the fixed bound of the fp32 "no worse than the existing call" clause (measured worst: 9.2e-3, z)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _close(a, b, tol, what=""):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    scale = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= tol * scale, (what, np.abs(a - b).max(), scale)


def _tol(dtype, block):
    return TOL64 if dtype == np.float64 else TOL32[block]


def _rnd(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def _problem(seed, N, M, d, family=o.KERNEL_SE, lik=o.LIK_GAUSSIAN, dtype=np.float64, centered=False):
    """-> x, y, sva, s2, mux (N), muz (M): every array exactly representable in `dtype`."""
    x, y, nc, s2 = o.synth_problem(seed, N, M, d, family=family, lik=lik, dtype=dtype)
    ils = _rnd(np.linspace(0.8, 1.3, d) * np.asarray(nc.kernel.inv_lengthscale, dtype=np.float64), dtype)
    k = o.Kernel(family, nc.kernel.variance, ils)
    sva = o.SVA(k, nc.z, nc.m, nc.Lq, jitter=nc.jitter, mean_const=0.15)
    if centered:   # the Centered form of a well-conditioned whitened posterior: m = c + Lk m~, Lq = Lk (0.8 B)
        Lk = np.linalg.cholesky(o.kuu(sva))
        sva = o.SVA(k, nc.z, _rnd(0.15 + Lk @ nc.m, dtype), _rnd(np.tril(Lk @ (0.8 * nc.Lq)), dtype), jitter=nc.jitter, mean_const=0.15,
                    centered=True)
    rng = np.random.default_rng(seed)
    xs = np.asarray(x, dtype=np.float64).reshape(d, -1)
    amp = 0.25 if lik in (o.LIK_POISSON_EXP, o.LIK_EXPONENTIAL_EXP, o.LIK_GAMMA_EXP) else 0.6
    mux = _rnd(amp * np.sin(1.7 * xs[0]) + 0.1 * rng.standard_normal(N), dtype)   # a trend the kernel does not carry, plus noise
    muz = _rnd(amp * np.sin(1.7 * np.asarray(sva.z, dtype=np.float64).reshape(d, -1)[0]), dtype)
    return x, y, sva, s2, mux, muz


def _upload(ctx, x, y, dtype, layout):
    if layout == _ffi.VEC:
        return _ffi.DeviceData(ctx, np.reshape(x, -1), y, dtype)
    if layout == _ffi.ROWVECS:
        return _ffi.DeviceData(ctx, np.ascontiguousarray(np.reshape(x, (x.shape[0], -1)).T), y, dtype, layout=_ffi.ROWVECS)
    return _ffi.DeviceData(ctx, x, y, dtype)


def _zgrad(g, d, M):
    return np.reshape(np.asarray(g["z"], dtype=np.float64), (d, M)) if np.ndim(g["z"]) == 2 else np.reshape(g["z"], (1, M))


def _check(ctx, x, y, sva, s2, mux, muz, dtype, lik=o.LIK_GAUSSIAN, qn=0, layout=_ffi.COLVECS, off=0, n=None, num_data=None):
    d, N = np.reshape(x, (sva.z.shape[0], -1)).shape
    n = N - off if n is None else n
    nd = float(num_data) if num_data is not None else 2.5 * N
    xs = np.reshape(np.asarray(x, dtype=np.float64), (d, N))[:, off:off + n]
    model = device_model(ctx, sva, dtype=dtype, lik=lik, sigma2=s2, quadrature_n=qn)
    model.set_mean_z(muz)
    data = _upload(ctx, x, y, dtype, layout)
    errs = {}
    try:
        pmb = mux[off:off + n]
        v, _, g = model.elbo_grad(data, off, n, nd, prior_mean=pmb, mean_grad=True)
        rv, rg = pmr.elbo_grad(sva, xs, y[off:off + n], pmb, muz, lik=lik, sigma2=s2, num_data=nd, quadrature_n=qn)
        mu, var = model.marginals(data, off, n, prior_mean=pmb)
        rmu, rvar = pmr.marginals(sva, xs, pmb, muz)
        fv, _ = model.elbo(data, off, n, nd, prior_mean=pmb)
        got = dict(value=[v], mu=mu, var=var, mean_x=g["mean_x"], z=_zgrad(g, d, sva.z.shape[1]),
                   **{b: g[b] for b in GRAD_BLOCKS if b != "z"})
        ref = dict(value=[rv], mu=rmu, var=rvar, mean_x=rg["mean_x"], **{b: rg[b] for b in GRAD_BLOCKS})
        scales = {}
        if lik not in (o.LIK_GAUSSIAN, o.LIK_GAMMA_EXP):
            got.pop("lik_sigma2"), ref.pop("lik_sigma2")
        else:   # sum of the magnitudes of the per-point terms of d E / d (likelihood parameter)
            from scipy.special import digamma
            yb = np.asarray(y[off:off + n], dtype=np.float64)
            terms = (-0.5 / s2 + 0.5 * ((yb - rmu) ** 2 + rvar) / s2 ** 2) if lik == o.LIK_GAUSSIAN else (np.log(yb) - rmu - digamma(s2))
            scales["lik_sigma2"] = nd / n * np.abs(terms).sum()
        bad = []
        for b in got:
            a, r = np.asarray(got[b], dtype=np.float64).ravel(), np.asarray(ref[b], dtype=np.float64).ravel()
            errs[b] = float(np.abs(a - r).max() / max(np.abs(r).max(), scales.get(b, 0.0), 1e-300))
            if errs[b] > _tol(dtype, b):
                bad.append((b, errs[b]))
        if bad and dtype == np.float32:   # the existing call's own fp32 error, same problem without offsets (see the module docstring)
            model.set_mean_z(None)
            _, _, g0 = model.elbo_grad(data, off, n, nd)
            _, rg0 = pmr.elbo_grad(sva, xs, y[off:off + n], None, None, lik=lik, sigma2=s2, num_data=nd, quadrature_n=qn)
            g0 = dict(g0, z=_zgrad(g0, d, sva.z.shape[1]))
            base = {b: float(np.abs(np.asarray(g0[b], dtype=np.float64).ravel() - np.asarray(rg0[b], dtype=np.float64).ravel()).max()
                             / max(np.abs(np.asarray(rg0[b])).max(), scales.get(b, 0.0), 1e-300)) for b, _ in bad if b in GRAD_BLOCKS}
            print("fp32 errors with offsets", bad, "existing call without", base)
            bad = [(b, e) for b, e in bad if not (b in base and e <= 3.0 * base[b] and e <= FP32_CEIL)]
        assert not bad, bad
        _close([fv], [rv], _tol(dtype, "value"), "forward value")
        assert g["mean_x"].dtype == np.dtype(dtype)
        return g, errs
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
    x, y, sva, s2, mux, muz = _problem(700 + i, 901, 64, d, family=family, lik=lik, dtype=dtype, centered=bool(i % 2))
    _, errs = _check(ctx, x, y, sva, s2, mux, muz, dtype, lik, qn, layout, off=37, n=801)
    print("errs", dtype.__name__, family, lik, qn, errs)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("centered", [False, True])
def test_parity_layout_parametrization(ctx, layout, centered):
    d = 1 if layout == _ffi.VEC else 5
    for dtype in (np.float64, np.float32):
        x, y, sva, s2, mux, muz = _problem(760 + d, 700, 40, d, family=o.KERNEL_MATERN52, lik=o.LIK_POISSON_EXP, dtype=dtype,
                                           centered=centered)
        _check(ctx, x, y, sva, s2, mux, muz, dtype, o.LIK_POISSON_EXP, 0, layout)


def test_several_chunks_and_window(ctx):
    """A gradient batch of more than 131 072 points runs in 65 536-point chunks: each chunk's strips read mux from the chunk's offset."""
    N, M, d = 140_000, 128, 3
    x, y, sva, s2, mux, muz = _problem(771, N, M, d, family=o.KERNEL_MATERN32, centered=True)
    _check(ctx, x, y, sva, s2, mux, muz, np.float64, num_data=float(N))
    _check(ctx, x, y, sva, s2, mux, muz, np.float64, off=3_001, n=136_000, num_data=float(N))


@pytest.mark.parametrize("overlap", [0, 1])
def test_small_batch_split_and_overlap_paths(overlap):
    """1 024 points at M = 1024 (NonCentered): with SVGP_OVERLAP=1 the strips run segmented beside the factorisation and their closing
    launch takes the several-workgroups-per-strip split; SVGP_OVERLAP=0 the plain path.  Both against the reference.  The path taken is
    asserted from the timing record of the last (forward) call of _check: segmented = one launch per panel + the pre-generation + the
    split closing launch, with a non-zero overlap; plain = at most two strip launches, no overlap.  The value-and-gradient call before it
    plans its strips with the same overlap_plan / seg_split_factor on the same batch."""
    N, M, d = 4096, 1024, 8
    nP = M // 128
    x, y, sva, s2, mux, muz = _problem(781, N, M, d, family=o.KERNEL_SE)
    with context_with_env(SVGP_OVERLAP=overlap, SVGP_SEG_SPLIT=1, SVGP_TIMING=1) as c:
        _check(c, x, y, sva, s2, mux, muz, np.float64, off=1000, n=1024, num_data=float(N))
        t = c.timing()
        if overlap:
            assert t.strip_launches == nP + 2 and t.ms_overlap > 0.0, (t.strip_launches, t.ms_overlap)
        else:
            assert t.strip_launches <= 2 and t.ms_overlap == 0.0, (t.strip_launches, t.ms_overlap)


def _grads_equal(g, g0, keys=("variance", "lik_sigma2", "mean_const", "inv_lengthscale", "z", "m", "Lq")):
    for k in keys:
        assert np.array_equal(np.asarray(g[k]), np.asarray(g0[k])), k


def test_null_offsets_are_the_existing_calls_bitwise(ctx):
    for dtype, lik, centered in ((np.float64, o.LIK_GAUSSIAN, False), (np.float32, o.LIK_BERNOULLI_LOGISTIC, True),
                                 (np.float64, o.LIK_GAMMA_EXP, True)):
        x, y, sva, s2, _, _ = _problem(791, 3000, 200, 6, lik=lik, dtype=dtype, centered=centered)
        model = device_model(ctx, sva, dtype=dtype, lik=lik, sigma2=s2)
        data = _ffi.DeviceData(ctx, x, y, dtype)
        lib = ctx.lib
        v0, t0 = model.elbo(data, 10, 2900, 9000.0)
        out, terms = C.c_double(), _ffi.Terms()
        ctx.check(lib.svgp_elbo_with_mean(ctx.h, model.h, data.h, 10, 2900, 9000.0, None, C.byref(out), C.byref(terms)), terms)
        assert out.value == v0 and bytes(terms) == bytes(t0)
        mu0, var0 = model.marginals(data, 10, 2900)
        mu, var = np.zeros(2900), np.zeros(2900)
        ctx.check(lib.svgp_marginals_with_mean(ctx.h, model.h, data.h, 10, 2900, None, mu.ctypes.data_as(C.c_void_p),
                                               var.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(mu, mu0) and np.array_equal(var, var0)
        gv0, gt0, g0 = model.elbo_grad(data, 10, 2900, 9000.0)
        il, zb, mb, Lb = np.zeros(6), np.zeros((6, 200), dtype=dtype, order="F"), np.zeros(200, dtype=dtype), np.zeros((200, 200), dtype=dtype, order="F")
        g = _ffi.Grads(0, 0, 0, il.ctypes.data_as(C.POINTER(C.c_double)), zb.ctypes.data_as(C.c_void_p), mb.ctypes.data_as(C.c_void_p),
                       Lb.ctypes.data_as(C.c_void_p))
        ctx.check(lib.svgp_elbo_grad_with_mean(ctx.h, model.h, data.h, 10, 2900, 9000.0, None, 0.0, None, None, C.byref(out),
                                               C.byref(terms), C.byref(g), None, None), terms)
        assert out.value == gv0 and bytes(terms) == bytes(gt0)
        _grads_equal(dict(variance=g.variance, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const, inv_lengthscale=il, z=zb, m=mb, Lq=Lb), g0)
        model.free()
        data.free()


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_offsets_bitwise(ctx, centered, dtype):
    """mux = 0 and muz = 0: every output of the four routes (built-in / caller likelihood, with / without x_bar) is the existing call's."""
    x, y, sva, s2, _, _ = _problem(801, 2500, 150, 4, lik=o.LIK_POISSON_EXP, dtype=dtype, centered=centered)
    model = device_model(ctx, sva, dtype=dtype, lik=o.LIK_POISSON_EXP, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, dtype)
    zx = np.zeros(2000, dtype=dtype)
    ref_v, ref_t = model.elbo(data, 300, 2000, 7000.0)
    ref_m = model.marginals(data, 300, 2000)
    ref_g = model.elbo_grad(data, 300, 2000, 7000.0, inputs=True)
    mu, var = ref_m
    yb = y[300:2300]
    e = o.expected_loglik(o.LIK_POISSON_EXP, mu, np.sqrt(var), yb, s2)
    gmu, gv, _ = o.expected_loglik_grads(o.LIK_POISSON_EXP, mu, var, yb, s2)
    ref_ext = model.elbo_grad(data, 300, 2000, 7000.0, ext=(e, gmu, gv))
    ref_ext_in = model.elbo_grad(data, 300, 2000, 7000.0, ext=(e, gmu, gv), inputs=True)
    ref_plain = model.elbo_grad(data, 300, 2000, 7000.0)
    model.set_mean_z(np.zeros(150))
    v, t = model.elbo(data, 300, 2000, 7000.0, prior_mean=zx)
    assert v == ref_v and bytes(t) == bytes(ref_t)
    m2 = model.marginals(data, 300, 2000, prior_mean=zx)
    assert np.array_equal(m2[0], ref_m[0]) and np.array_equal(m2[1], ref_m[1])
    for kw, ref in ((dict(inputs=True), ref_g), (dict(ext=(e, gmu, gv)), ref_ext), (dict(ext=(e, gmu, gv), inputs=True), ref_ext_in),
                    ({}, ref_plain)):
        gv_, gt_, gg = model.elbo_grad(data, 300, 2000, 7000.0, prior_mean=zx, mean_grad=True, **kw)
        assert gv_ == ref[0] and bytes(gt_) == bytes(ref[1])
        _grads_equal(gg, ref[2])
        if "inputs" in kw:
            assert np.array_equal(gg["x"], ref[2]["x"])
    model.free()
    data.free()


def test_noncentered_ignores_mean_z(ctx):
    x, y, sva, s2, mux, muz = _problem(811, 2000, 120, 3)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    a = model.elbo_grad(data, 0, 2000, 5000.0, prior_mean=mux, mean_grad=True)
    pa = model.posterior()
    model.set_mean_z(muz)
    b = model.elbo_grad(data, 0, 2000, 5000.0, prior_mean=mux, mean_grad=True)
    pb = model.posterior()
    assert a[0] == b[0] and bytes(a[1]) == bytes(b[1])
    _grads_equal(b[2], a[2], keys=("variance", "lik_sigma2", "mean_const", "inv_lengthscale", "z", "m", "Lq", "mean_x"))
    assert all(np.array_equal(p, q) for p, q in zip(pa, pb))
    model.free()
    data.free()


def test_mean_z_persists_and_moves_alpha(ctx):
    """Centered: muz changes alpha (svgp_posterior) as Kuu \\ (m - c - muz); it survives svgp_model_update and NULL removes it."""
    x, y, sva, s2, mux, muz = _problem(821, 1500, 90, 3, centered=True)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    base = model.posterior()[1]
    model.set_mean_z(muz)
    Kuu = o.kuu(sva)
    _close(model.posterior()[1], np.linalg.solve(Kuu, sva.m - sva.mean_const - muz), 1e-9, "alpha")
    desc, keep = __import__("helpers").desc_from_oracle(sva, sigma2=s2)
    model.update(desc, keep)                       # a training step: the offsets stay
    v, _, g = model.elbo_grad(data, 0, 1500, 3000.0, prior_mean=mux, mean_grad=True)
    rv, rg = pmr.elbo_grad(sva, x, y, mux, muz, sigma2=s2, num_data=3000.0)
    _close([v], [rv], 1e-9, "value after update")
    _close(g["m"], rg["m"], 1e-9, "m")
    model.set_mean_z(None)
    assert np.array_equal(model.posterior()[1], base)
    model.free()
    data.free()


def test_mean_const_identity(ctx):
    x, y, sva, s2, mux, muz = _problem(831, 3000, 100, 2, lik=o.LIK_BERNOULLI_LOGISTIC, centered=True)
    model = device_model(ctx, sva, lik=o.LIK_BERNOULLI_LOGISTIC, sigma2=s2)
    model.set_mean_z(muz)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    _, _, g = model.elbo_grad(data, 0, 3000, 6000.0, prior_mean=mux, mean_grad=True)
    muz_bar = -np.asarray(g["m"])          # Centered: the library's documented identity
    total = g["mean_x"].sum() + muz_bar.sum()
    assert abs(g["mean_const"] - total) <= 1e-10 * (np.abs(g["mean_x"]).sum() + np.abs(muz_bar).sum())
    model.free()
    data.free()


def test_device_offsets_and_gradient_into_torch(ctx):
    import torch
    N, M, d = 5000, 128, 4
    for dtype, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        x, y, sva, s2, mux, muz = _problem(841, N, M, d, family=o.KERNEL_MATERN32, dtype=dtype, centered=True)
        stream = torch.cuda.current_stream()
        tctx = _ffi.Context(0, stream.cuda_stream)
        try:
            xt = torch.tensor(np.asarray(x, dtype=dtype), device="cuda")
            yt = torch.tensor(np.asarray(y, dtype=dtype), device="cuda")
            model = device_model(tctx, sva, dtype=dtype, sigma2=s2)
            model.set_mean_z(muz)
            data = _ffi.DeviceData.wrap(tctx, dtype, d, N, N, xt.data_ptr(), yt.data_ptr())
            mt = torch.tensor(mux[500:4500].astype(dtype), device="cuda")
            out = torch.full((4000 + 16,), -7.25, dtype=tdt, device="cuda")
            v_dev, t_dev, g_dev = model.elbo_grad(data, 500, 4000, 2.0 * N, prior_mean=mt, mean_grad=out)
            assert "mean_x" not in g_dev
            v_h, t_h, g_h = model.elbo_grad(data, 500, 4000, 2.0 * N, prior_mean=mux[500:4500], mean_grad=True)
            torch.cuda.synchronize()
            o_np = out.cpu().numpy()
            assert v_dev == v_h and bytes(t_dev) == bytes(t_h)
            _grads_equal(g_dev, g_h)
            assert np.array_equal(o_np[:4000], g_h["mean_x"]) and np.all(o_np[4000:] == -7.25)
            assert np.array_equal(model.marginals(data, 500, 4000, prior_mean=mt)[0], model.marginals(data, 500, 4000, prior_mean=mux[500:4500])[0])
            assert model.elbo(data, 500, 4000, 2.0 * N, prior_mean=mt)[0] == model.elbo(data, 500, 4000, 2.0 * N, prior_mean=mux[500:4500])[0]
            model.free()
            data.free()
        finally:
            tctx.close()


def test_caller_likelihood_matches_builtin(ctx):
    N, M, d = 2500, 90, 3
    x, y, sva, s2, mux, muz = _problem(851, N, M, d, centered=True)
    model = device_model(ctx, sva, sigma2=s2)
    model.set_mean_z(muz)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    pmb = mux[100:2100]
    v_in, _, g_in = model.elbo_grad(data, 100, 2000, 7000.0, prior_mean=pmb, mean_grad=True, inputs=True)
    mu, var = model.marginals(data, 100, 2000, prior_mean=pmb)
    yb = y[100:2100]
    e_host = o.expected_loglik(o.LIK_GAUSSIAN, mu, np.sqrt(var), yb, s2)
    gmu, gv, _ = o.expected_loglik_grads(o.LIK_GAUSSIAN, mu, var, yb, s2)
    v_ext, _, g_ext = model.elbo_grad(data, 100, 2000, 7000.0, prior_mean=pmb, mean_grad=True, inputs=True, ext=(e_host, gmu, gv))
    # (1e-10 for the gradient blocks: svgp_marginals takes the variance as k - sum A^2 + sum (B'A)^2, the gradient strips as k_j' (R A)_j -
    # the header's two paths - so the host's point gradients differ from the built-in ones in the last bits; measured 7.6e-12 on the
    # kernel variance's gradient)
    _close([v_ext], [v_in], 1e-12, "value")
    for b in ("variance", "mean_const", "inv_lengthscale", "z", "m", "Lq", "mean_x", "x"):
        _close(g_ext[b], g_in[b], 1e-10, b)
    model.free()
    data.free()


def test_nan_offset_stays_at_its_point(ctx):
    N, M, d = 1200, 64, 3
    x, y, sva, s2, mux, muz = _problem(861, N, M, d)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    mu0, _ = model.marginals(data, 0, N, prior_mean=mux)
    bad = mux.copy()
    bad[417] = np.nan
    mu, var = model.marginals(data, 0, N, prior_mean=bad)
    assert np.isnan(mu[417]) and np.isfinite(np.delete(mu, 417)).all() and np.isfinite(var).all()
    assert np.array_equal(np.delete(mu, 417), np.delete(mu0, 417))
    v, t = model.elbo(data, 0, N, 0.0, prior_mean=bad)    # status OK: the numbers say it
    assert np.isnan(v)
    gv, _, g = model.elbo_grad(data, 0, N, 0.0, prior_mean=bad, mean_grad=True)
    assert np.isnan(gv) and np.isnan(g["mean_x"][417])
    model.free()
    data.free()


def test_bad_arguments(ctx):
    import torch
    N, M, d = 800, 32, 2
    x, y, sva, s2, mux, muz = _problem(871, N, M, d)
    model = device_model(ctx, sva, sigma2=s2)
    xt = torch.tensor(x, dtype=torch.float64, device="cuda")
    yt = torch.tensor(y, dtype=torch.float64, device="cuda")
    data = _ffi.DeviceData.wrap(ctx, np.float64, d, N, N, xt.data_ptr(), yt.data_ptr())
    lib = ctx.lib
    hbuf = np.zeros(N)
    dev = torch.zeros(N, dtype=torch.float64, device="cuda")
    xg_dev = torch.zeros((d, N), dtype=torch.float64, device="cuda")
    good_pm = _ffi.PointMean(mux.ctypes.data_as(C.c_void_p), 0, 0)
    bad_pm = [_ffi.PointMean(None, 0, 0), _ffi.PointMean(mux.ctypes.data_as(C.c_void_p), 2, 0),
              _ffi.PointMean(mux.ctypes.data_as(C.c_void_p), 0, 1)]
    bad_gpm = [_ffi.PointMeanGrad(None, 0, 0), _ffi.PointMeanGrad(hbuf.ctypes.data_as(C.c_void_p), 3, 0),
               _ffi.PointMeanGrad(hbuf.ctypes.data_as(C.c_void_p), 0, 5),
               _ffi.PointMeanGrad(C.c_void_p(xt.data_ptr() + 8 * 100), 1, 0),     # overlaps x
               _ffi.PointMeanGrad(C.c_void_p(yt.data_ptr() + 8 * 10), 1, 0)]      # overlaps y
    gx_dev = _ffi.InputGrad(C.c_void_p(xg_dev.data_ptr()), N, 1, 0)
    gmu = np.zeros(N)
    il, zb, mb, Lb = np.zeros(d), np.zeros((d, M)), np.zeros(M), np.zeros((M, M))
    g = _ffi.Grads(0, 0, 0, il.ctypes.data_as(C.POINTER(C.c_double)), zb.ctypes.data_as(C.c_void_p), mb.ctypes.data_as(C.c_void_p),
                   Lb.ctypes.data_as(C.c_void_p))
    out, terms = C.c_double(), _ffi.Terms()
    gp = lambda p: gmu.ctypes.data_as(C.c_void_p) if p else None

    def grad(pm, gpm, gx=None, a=False, b=False):
        return lib.svgp_elbo_grad_with_mean(ctx.h, model.h, data.h, 0, N, 0.0, C.byref(pm) if pm is not None else None, 0.0, gp(a), gp(b),
                                            C.byref(out), C.byref(terms), C.byref(g), C.byref(gx) if gx is not None else None,
                                            C.byref(gpm) if gpm is not None else None)

    for pm in bad_pm:
        assert lib.svgp_elbo_with_mean(ctx.h, model.h, data.h, 0, N, 0.0, C.byref(pm), C.byref(out), C.byref(terms)) == _ffi.INVALID_ARG
        assert lib.svgp_marginals_with_mean(ctx.h, model.h, data.h, 0, N, C.byref(pm), hbuf.ctypes.data_as(C.c_void_p),
                                            hbuf.ctypes.data_as(C.c_void_p)) == _ffi.INVALID_ARG
        assert grad(pm, None) == _ffi.INVALID_ARG
    for gpm in bad_gpm:
        assert grad(good_pm, gpm) == _ffi.INVALID_ARG
    assert grad(good_pm, _ffi.PointMeanGrad(C.c_void_p(xg_dev.data_ptr() + 8 * 5), 1, 0), gx_dev) == _ffi.INVALID_ARG   # overlaps x_bar
    assert grad(good_pm, None, a=True) == _ffi.INVALID_ARG and grad(good_pm, None, b=True) == _ffi.INVALID_ARG          # one of g_mu / g_v
    # the mirror checks a device tensor given as the destination before the library could write batch_len elements into it
    guard = torch.full((N + 8,), -3.5, dtype=torch.float64, device="cuda")
    for badt in (torch.zeros(N, dtype=torch.float32, device="cuda"),     # fp32 for fp64 data: half the bytes
                 guard[:N - 1],                                           # one element short
                 guard[::2],                                              # not contiguous
                 torch.zeros(N, dtype=torch.float64)):                    # host tensor
        with pytest.raises(ValueError):
            model.elbo_grad(data, 0, N, 0.0, prior_mean=mux, mean_grad=badt)
    torch.cuda.synchronize()
    assert torch.all(guard == -3.5)
    assert np.array_equal(xt.cpu().numpy(), x) and np.array_equal(yt.cpu().numpy(), y)
    assert grad(good_pm, _ffi.PointMeanGrad(C.c_void_p(dev.data_ptr()), 1, 0)) == _ffi.OK   # healthy afterwards
    torch.cuda.synchronize()
    _, rg = pmr.elbo_grad(sva, x, y, mux, None, sigma2=s2)
    _close(dev.cpu().numpy(), rg["mean_x"], 1e-9, "mean_x")
    model.free()
    data.free()


def test_collective_world_of_one():
    x, y, sva, s2, mux, muz = _problem(881, 3001, 96, 3, family=o.KERNEL_MATERN52, centered=True)
    c = _ffi.Context(0)
    try:
        model = device_model(c, sva, sigma2=s2)
        model.set_mean_z(muz)
        data = _ffi.DeviceData(c, x, y, np.float64)
        pmb = mux[100:1600]
        lv, _, lg = model.elbo_grad(data, 100, 1500, 9000.0, prior_mean=pmb, mean_grad=True)
        le = model.elbo(data, 100, 1500, 9000.0, prior_mean=pmb)[0]
        c.attach_comm(_ffi.comm_unique_id(), 1, 0)
        gv, _, gg = model.elbo_grad(data, 100, 1500, 9000.0, prior_mean=pmb, mean_grad=True)
        assert abs(gv - lv) <= 1e-12 * abs(lv)
        assert model.elbo(data, 100, 1500, 9000.0, prior_mean=pmb)[0] == le
        np.testing.assert_allclose(gg["mean_x"], lg["mean_x"], rtol=1e-12, atol=1e-13 * np.abs(lg["mean_x"]).max())
        np.testing.assert_allclose(gg["m"], lg["m"], rtol=1e-12, atol=1e-13 * np.abs(lg["m"]).max())
        with pytest.raises(ValueError):   # an argument error goes through the opening handshake and comes back as itself
            model.elbo_grad(data, 100, 1500, 9000.0, prior_mean=pmb, mean_grad=0)
        g2 = model.elbo_grad(data, 100, 1500, 9000.0, prior_mean=pmb, mean_grad=True)[2]
        assert np.array_equal(g2["mean_x"], gg["mean_x"])
        model.free()
        data.free()
    finally:
        c.close()


def test_python_mirror_custom_mean(ctx):
    """GP(CustomMean(fn), k): the posterior's mean_and_var and the ELBO gradient, end to end through the mirror."""
    import approxgp as ag

    rng = np.random.default_rng(13)
    N, M = 1500, 40
    xr = rng.uniform(-3, 3, (2, N))
    fn = lambda x: 0.8 * np.asarray(x)[0] - 0.3 * np.asarray(x)[1] ** 2
    y = fn(xr) + np.sin(xr.sum(0)) + 0.1 * rng.standard_normal(N)
    z = xr[:, :M].copy()
    A = np.eye(M) + 0.01 * np.tril(rng.standard_normal((M, M)))
    mvec = 0.1 * rng.standard_normal(M)
    k = 1.3 * ag.with_lengthscale(ag.Matern32Kernel(), 0.7)
    f = ag.GP(ag.CustomMean(fn), k)
    for centered in (False, True):
        q = ag.MvNormal.from_cholesky(mvec + (fn(z) if centered else 0.0), A)
        sva = ag.SparseVariationalApproximation(ag.Centered(), f(z, 1e-5), q) if centered else ag.SparseVariationalApproximation(f(z, 1e-5), q)
        osva = o.SVA(o.Kernel(o.KERNEL_MATERN32, 1.3, np.full(2, 1 / 0.7)), z, q.m, A, jitter=1e-5, centered=centered)
        xs = rng.uniform(-3, 3, (2, 300))
        post = ag.posterior(sva, ctx=ctx)
        mu, var = post.mean_and_var(xs)
        rmu, rvar = pmr.marginals(osva, xs, fn(xs), fn(z))
        _close(mu, rmu, 1e-9, "mean")
        _close(var, rvar - o.DEFAULT_SIGMA2, 1e-9, "var")
        val, g = ag.elbo_and_gradient(sva, f(xr, 0.3), y, num_data=3 * N, ctx=ctx)
        rv, rg = pmr.elbo_grad(osva, xr, y, fn(xr), fn(z), sigma2=0.3, num_data=3 * N)
        _close([val], [rv], 1e-9, "value")
        _close(g["mean_x"], rg["mean_x"], 1e-9, "mean_x")
        _close(g["mean_z"], rg["mean_z"], 1e-9, "mean_z")
        _close(g["m"], rg["m"], 1e-9, "m")
        _close([ag.elbo(sva, f(xr, 0.3), y, num_data=3 * N, ctx=ctx)], [rv], 1e-9, "elbo")
