"""GPU checks of the collapsed (Titsias) bound and the optimal q(u) (svgp_collapsed_bound / _q / _grad) against the float64
restatement tests/collapsed_ref.py.

Shapes: the smallest that cross every boundary of the phase-1 kernel and of the tail - M below, at and above one 128-row panel; d in
the three kernel families (d <= 16, 16 < d <= 32, 32 < d <= 64); n that is no multiple of a strip; two gradient chunks (70 001 points).
fp32: measured against the fp64 restatement on fp32-rounded inputs, asserted at 4x the worst measured value (see F32_MEASURED)."""
import functools

import numpy as np
import pytest

import collapsed_ref as cr
import input_grad_ref
import svgp_oracle as o
from approxgp import _ffi
from helpers import device_model

pytestmark = pytest.mark.gpu
JITTER = 1e-5
JITTER_F32 = 1e-3     # the project's fp32 problems carry the larger jitter (approxgp/synthetic.py): an fp32 cholesky(Kuu) needs it


def _jitter(name):
    return JITTER_F32 if name.startswith("f32") else JITTER

# (n, M, d, family, ard, layout, centered, mean_const, batch_off)
CASES = {
    "n20_M5_d1": (20, 5, 1, o.KERNEL_SE, False, _ffi.VEC, False, 0.0, 0),
    "n300_M20_d1": (300, 20, 1, o.KERNEL_MATERN52, False, _ffi.VEC, True, 0.7, 0),
    "n777_M200_d3": (777, 200, 3, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0),
    "n1000_M130_d8": (1000, 130, 8, o.KERNEL_MATERN32, True, _ffi.ROWVECS, True, -0.4, 0),
    "n640_M129_d17": (640, 129, 17, o.KERNEL_SE, False, _ffi.COLVECS, False, 0.3, 37),
    "n513_M64_d64": (513, 64, 64, o.KERNEL_MATERN52, True, _ffi.ROWVECS, False, 0.0, 0),
    "n70001_M64_d2": (70001, 64, 2, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0),
}
F32_CASES = {
    "f32_n1000_M256_d4": (1000, 256, 4, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0),
    "f32_n70001_M64_d2": (70001, 64, 2, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0),   # 65 536-point chunk: the 128-point strips
    "f32_n640_M129_d17": (640, 129, 17, o.KERNEL_MATERN32, False, _ffi.COLVECS, True, 0.3, 37),
}
# fp32 against the fp64 restatement on fp32-rounded inputs, worst value over F32_CASES as measured on an MI355X (relative to the
# bound / to each gradient block's largest entry); the asserts below take 4x these (box-to-box reduction-order differences)
F32_MEASURED = {"bound": 7.4e-6, "variance": 2.1e-4, "lik_sigma2": 5.7e-5, "mean_const": 6.3e-4, "inv_lengthscale": 1.0e-5, "z": 1.1e-3}


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(kernel, z, x, y, s2, spec, reference over the window, oracle SVA at the optimal q, gradient reference) - computed once."""
    spec = {**CASES, **F32_CASES}[name]
    n, M, d, family, ard, layout, centered, mc, off = spec
    dtype = np.float32 if name.startswith("f32") else np.float64
    kernel, z, x, y, s2 = cr.problem(n + off + (11 if off else 0), M, d, family=family, ard=ard, dtype=dtype, mean_const=mc)
    xw, yw = x[:, off:off + n], y[off:off + n]
    sva, ref = cr.optimal_sva(kernel, z, _jitter(name), xw, s2, yw, mean_const=mc, centered=centered)
    for a in (z, x, y, xw, yw):
        a.setflags(write=False)
    return kernel, z, x, y, s2, spec, ref, sva, (xw, yw)


@functools.lru_cache(maxsize=None)
def _grad_ref(name):
    kernel, z, x, y, s2, spec, ref, sva, (xw, yw) = _problem(name)
    return o.elbo_grad(sva, xw, yw, lik=o.LIK_GAUSSIAN, sigma2=s2)[1]


def _device(ctx, name, sva_q=None):
    """model (unit q unless sva_q is given) and data of a case on the device, in the case's layouts."""
    kernel, z, x, y, s2, spec, ref, sva, _ = _problem(name)
    n, M, d, family, ard, layout, centered, mc, off = spec
    dtype = np.float32 if name.startswith("f32") else np.float64
    q = sva_q if sva_q is not None else o.SVA(kernel, z, np.zeros(M), np.eye(M), jitter=_jitter(name), mean_const=mc, centered=centered)
    if d == 1:
        xd = x[0]
        q = o.SVA(q.kernel, q.z, q.m, q.Lq, jitter=q.jitter, mean_const=q.mean_const, centered=q.centered)
    else:
        xd = x if layout == _ffi.COLVECS else np.ascontiguousarray(x.T)
    data = _ffi.DeviceData(ctx, xd, y, dtype, layout=layout if d > 1 else _ffi.VEC)
    model = device_model(ctx, q, dtype=dtype, sigma2=s2)
    return model, data


def _rel(a, b):
    return abs(a - b) / abs(b)


def _block_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _z_like(gz, zref, d):
    return gz.reshape(zref.shape, order="F") if d > 1 else gz


@pytest.mark.parametrize("name", list(CASES))
def test_bound_and_terms_match_the_restatement(ctx, name):
    kernel, z, x, y, s2, spec, ref, sva, _ = _problem(name)
    n, off = spec[0], spec[8]
    model, data = _device(ctx, name)
    try:
        val, t = model.collapsed_bound(data, off, n)
        print(f"{name}: bound {val:.12g} ref {ref.bound:.12g} rel {_rel(val, ref.bound):.2e}")
        assert _rel(val, ref.bound) < 1e-8                      # the project's fp64 contract
        assert t.bound == val and t.n_points == n and t.chol_info == 0 and t.chol_info_b == 0 and t.reserved == 0
        assert _rel(t.fit, ref.fit) < 1e-8 and abs(t.trace - ref.trace) < 1e-8 * abs(ref.bound)
        assert _rel(t.logdet_B, ref.logdet_B) < 1e-8 and abs(t.logdet_kuu - ref.logdet_kuu) < 1e-8 * abs(ref.logdet_kuu)
        val2, _ = model.collapsed_bound(data, off, n)
        assert val2 == val                                      # bitwise repeatable
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("name", list(CASES))
def test_optimal_q_on_the_device(ctx, name):
    """After svgp_collapsed_q the model carries the optimal q: svgp_elbo on the same window is the bound, svgp_predict is the
    restatement's posterior, and a fresh model built from the returned host arrays gives the same ELBO bitwise."""
    kernel, z, x, y, s2, spec, ref, sva, (xw, yw) = _problem(name)
    n, M, d, family, ard, layout, centered, mc, off = spec
    model, data = _device(ctx, name)
    try:
        bound, m, Lq = model.collapsed_q(data, off, n)
        assert _rel(bound, ref.bound) < 1e-8
        assert np.all(np.triu(Lq, 1) == 0) and np.all(np.diag(Lq) > 0)
        el, _ = model.elbo(data, off, n, float(n))
        print(f"{name}: elbo at q {el:.12g} bound {bound:.12g} rel {_rel(el, bound):.2e}")
        assert _rel(el, bound) < 1e-9
        bound2, m2, Lq2 = model.collapsed_q(data, off, n)
        assert bound2 == bound and np.array_equal(m2, m) and np.array_equal(Lq2, Lq)   # bitwise repeatable
        # predictions at 50 points against the restatement's posterior
        rng = np.random.default_rng(3)
        xs = rng.random((d, 50))
        mean_ref, cov_ref = cr.posterior_at(kernel, z, JITTER, xw, s2, yw, xs, mean_const=mc)
        mean, var, cov = model.predict(xs[0] if d == 1 else xs, True, True, True)
        assert np.abs(mean - mean_ref).max() <= 1e-9 * np.abs(mean_ref).max()
        assert np.abs(var - np.diag(cov_ref)).max() <= 1e-9 * kernel.variance
        assert np.abs(cov - cov_ref).max() <= 1e-9 * kernel.variance
        # the returned host arrays describe the same q
        fresh = o.SVA(kernel, z, m, Lq, jitter=JITTER, mean_const=mc, centered=centered)
        model2 = device_model(ctx, fresh, dtype=np.float64, sigma2=s2)
        try:
            el2, _ = model2.elbo(data, off, n, float(n))
        finally:
            model2.free()
        assert el2 == el
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_matches_the_envelope_reference(ctx, name):
    kernel, z, x, y, s2, spec, ref, sva, (xw, yw) = _problem(name)
    n, M, d, off = spec[0], spec[1], spec[2], spec[8]
    g_ref = _grad_ref(name)
    model, data = _device(ctx, name)
    try:
        want_x = name == "n640_M129_d17"
        val, t, g = model.collapsed_grad(data, off, n, inputs=True if want_x else None)
        assert _rel(val, ref.bound) < 1e-8 and t.bound == val
        errs = {k: _block_err([g[k]], [g_ref[k]]) for k in ("variance", "lik_sigma2", "mean_const")}
        errs["inv_lengthscale"] = _block_err(g["inv_lengthscale"], g_ref["inv_lengthscale"])
        zr = g_ref["z"] if d > 1 else g_ref["z"][0]
        errs["z"] = _block_err(_z_like(g["z"], zr, d), zr)
        print(name, {k: f"{v:.2e}" for k, v in errs.items()})
        for k, v in errs.items():
            assert v <= 1e-6, (k, v)                                 # the tolerances of tests/test_gpu_grad.py
        if want_x:
            xbar = input_grad_ref.input_grad(sva, xw, yw, sigma2=s2)
            assert _block_err(g["x"], xbar) <= 1e-6
        val2, _, g2 = model.collapsed_grad(data, off, n)
        assert val2 == val and g2["variance"] == g["variance"] and g2["lik_sigma2"] == g["lik_sigma2"]
        assert np.array_equal(g2["z"], g["z"]) and np.array_equal(g2["inv_lengthscale"], g["inv_lengthscale"])
    finally:
        model.free()
        data.free()


def test_fp32_accuracy(ctx):
    """fp32 models (data pass in fp32, M-sized tail in fp64) against the fp64 restatement on fp32-rounded inputs, jitter 1e-3.  Measured on
    an MI355X, relative to the bound / to each gradient block's largest entry (bound, variance, lik_sigma2, mean_const, inv_lengthscale, z):
        f32_n1000_M256_d4   4.2e-6  3.1e-5  9.9e-6  2.3e-5  8.3e-6  1.1e-3
        f32_n70001_M64_d2   7.4e-6  2.1e-4  5.7e-5  6.3e-4  1.0e-5  6.7e-5     (two chunks; the 128-point strips)
        f32_n640_M129_d17   3.7e-8  2.5e-8  6.0e-8  2.7e-5  5.5e-6  2.8e-5     (Centered, wide inputs)
    F32_MEASURED holds the worst of each column; asserted at 4x.  The bound must also stay inside the project's fp32 contract of 1e-4."""
    worst = {k: 0.0 for k in F32_MEASURED}
    for name in F32_CASES:
        kernel, z, x, y, s2, spec, ref, sva, _ = _problem(name)
        n, M, d, off = spec[0], spec[1], spec[2], spec[8]
        g_ref = _grad_ref(name)
        model, data = _device(ctx, name)
        try:
            val, _, g = model.collapsed_grad(data, off, n)
            vb, _ = model.collapsed_bound(data, off, n)
        finally:
            model.free()
            data.free()
        assert vb == val
        e = {"bound": _rel(val, ref.bound)}
        for k in ("variance", "lik_sigma2", "mean_const"):
            e[k] = _block_err([g[k]], [g_ref[k]])
        e["inv_lengthscale"] = _block_err(g["inv_lengthscale"], g_ref["inv_lengthscale"])
        zr = g_ref["z"] if d > 1 else g_ref["z"][0]
        e["z"] = _block_err(_z_like(g["z"], zr, d), zr)
        print(name, {k: f"{v:.2e}" for k, v in e.items()})
        for k, v in e.items():
            worst[k] = max(worst[k], v)
    print("fp32 worst", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["bound"] < 1e-4
    for k, v in worst.items():
        assert F32_MEASURED[k] is not None, "fp32 figures have not been recorded"
        assert v <= 4 * F32_MEASURED[k], (k, v, F32_MEASURED[k])


def test_errors_leave_the_context_usable(ctx):
    name = "n300_M20_d1"
    kernel, z, x, y, s2, spec, ref, sva, _ = _problem(name)
    n, M = spec[0], spec[1]
    model, data = _device(ctx, name)
    try:
        # a Bernoulli model: SVGP_INVALID_ARG
        bern = device_model(ctx, o.SVA(kernel, z, np.zeros(M), np.eye(M), jitter=JITTER), lik=o.LIK_BERNOULLI_LOGISTIC)
        try:
            for call in (bern.collapsed_bound, bern.collapsed_q, bern.collapsed_grad):
                with pytest.raises(ValueError, match="Gaussian"):
                    call(data, 0, n)
        finally:
            bern.free()
        assert _rel(model.collapsed_bound(data, 0, n)[0], ref.bound) < 1e-8
        # a window outside the data, data without y
        with pytest.raises(ValueError, match="batch range"):
            model.collapsed_bound(data, 200, n)
        noy = _ffi.DeviceData(ctx, x[0], None, np.float64)
        try:
            with pytest.raises(ValueError, match="no observations"):
                model.collapsed_bound(noy, 0, n)
        finally:
            noy.free()
        # non-NULL m / Lq gradient outputs
        import ctypes as C
        buf = np.zeros(M)
        il, zb = np.zeros(1), np.zeros(M)
        g = _ffi.Grads(0.0, 0.0, 0.0, il.ctypes.data_as(C.POINTER(C.c_double)), zb.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), None)
        out, t = C.c_double(), _ffi.CollapsedTerms()
        assert ctx.lib.svgp_collapsed_grad(ctx.h, model.h, data.h, 0, n, C.byref(out), C.byref(t), C.byref(g), None) == _ffi.INVALID_ARG
        # a model with muz: SVGP_UNSUPPORTED
        model.set_mean_z(np.zeros(M))
        with pytest.raises(_ffi.UnsupportedError):
            model.collapsed_bound(data, 0, n)
        model.set_mean_z(None)
        assert _rel(model.collapsed_bound(data, 0, n)[0], ref.bound) < 1e-8
        # a duplicated inducing point at jitter 0: SVGP_NOT_POSDEF with chol_info set, and the model keeps its q
        zd = z.copy()
        zd[:, 7] = zd[:, 3]
        dup = device_model(ctx, o.SVA(kernel, zd, np.zeros(M), np.eye(M), jitter=0.0, mean_const=spec[7], centered=spec[6]), sigma2=s2)
        try:
            with pytest.raises(_ffi.PosDefException) as ei:
                dup.collapsed_bound(data, 0, n)
            assert 1 <= ei.value.info <= M
            with pytest.raises(_ffi.PosDefException):
                dup.collapsed_grad(data, 0, n)
        finally:
            dup.free()
        assert _rel(model.collapsed_bound(data, 0, n)[0], ref.bound) < 1e-8
    finally:
        model.free()
        data.free()


def test_nan_coordinate_gives_nan_not_an_error(ctx):
    name = "n777_M200_d3"
    kernel, z, x, y, s2, spec, ref, sva, _ = _problem(name)
    n, M = spec[0], spec[1]
    xn = x.copy()
    xn[1, 500] = np.nan
    data = _ffi.DeviceData(ctx, xn, y, np.float64)
    model = device_model(ctx, o.SVA(kernel, z, np.zeros(M), np.eye(M), jitter=JITTER), sigma2=s2)
    try:
        val, t = model.collapsed_bound(data, 0, n)
        assert np.isnan(val) and t.chol_info == 0 and t.chol_info_b == 0
        # the window that leaves the point out is healthy
        val2, _ = model.collapsed_bound(data, 0, 500)
        assert np.isfinite(val2)
    finally:
        model.free()
        data.free()


def test_python_mirror(ctx):
    """approxgp.VFE: elbo / approx_lml / elbo_and_gradient / posterior / optimal_variational_posterior end to end."""
    import approxgp as ag
    name = "n777_M200_d3"
    kernel, z, x, y, s2, spec, ref, sva, _ = _problem(name)
    k = kernel.variance * (ag.SqExponentialKernel() @ ag.ARDTransform(list(kernel.inv_lengthscale)))
    f = ag.GP(k)
    fz, fx = f(z, JITTER), f(x, s2)
    assert _rel(ag.elbo(ag.VFE(fz), fx, y, ctx=ctx), ref.bound) < 1e-8
    assert _rel(ag.approx_lml(ag.VFE(fz), fx, y, ctx=ctx), ref.bound) < 1e-8
    val, g = ag.elbo_and_gradient(ag.VFE(fz), fx, y, ctx=ctx)
    assert _rel(val, ref.bound) < 1e-8 and _block_err(g["z"], _grad_ref(name)["z"]) <= 1e-6
    q = ag.optimal_variational_posterior(fz, fx, y, ctx=ctx)
    assert isinstance(q, ag.SparseVariationalApproximation) and not q.is_centered
    assert _rel(ag.elbo(q, fx, y, ctx=ctx), ref.bound) < 1e-9
    post = ag.posterior(ag.VFE(fz), fx, y, ctx=ctx)
    assert isinstance(post, ag.ApproxPosteriorGP)
    xs = np.random.default_rng(3).random((3, 50))
    mean_ref, cov_ref = cr.posterior_at(kernel, z, JITTER, x, s2, y, xs)
    m, v = post.mean_and_var(xs)
    assert np.abs(m - mean_ref).max() <= 1e-9 * np.abs(mean_ref).max() and np.abs(v - np.diag(cov_ref)).max() <= 1e-9 * kernel.variance
