"""GPU checks of the Laplace entry points (csrc/laplace.hip) at the enumerated shapes of tests/laplace_edge_cases.py, each chosen
because one kernel can go wrong there: the gradient reduction beyond its first feature chunk and at tile edges, g and W of a single
Newton step from an uploaded start at odd panel counts, predictions at the output-tile edges in both dtypes and every layout, the
warm start's corner cases, and non-finite inputs.  tests/test_laplace_edges_cpu.py shows that the reference alone is well inside
every tolerance used here; profiles/laplace/edge_parity.md holds the measured fp32 figures (each test prints its own: run with -s).
"""
import ctypes as C

import numpy as np
import pytest

import laplace_edge_cases as ec
import laplace_ref as lr
import test_gpu_laplace as base
from approxgp import DeviceLaplace, _ffi

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- A. the gradient across feature chunks and tile edges ---------------------------------------------------------

def _device_gradient(ctx, row, dtype, layout):
    lik, fam, d, n = row
    x, y, il, s2 = ec.grad_problem(row)
    dev = base._dev(ctx, x.astype(dtype), y.astype(dtype), dtype, layout)
    desc, keep = dev.desc(base._kernel(fam, ec.VARIANCE, il), base._lik(lik, s2), ec.JITTER, maxiter=ec.GRAD_MAXITER)
    lml, gv, gil, info = dev.lml_grad(desc)
    dev.free()
    return lml, np.concatenate([[gv], gil])


_GRAD_REF = {}


def _reference_gradient(row):
    if row not in _GRAD_REF:
        lik, fam, d, n = row
        x, y, il, s2 = ec.grad_problem(row)
        lml, rv, ril = lr.lml_grad(lr.kernel_of(fam, ec.VARIANCE, il), x, y, lik, s2, jitter=ec.JITTER, maxiter=ec.GRAD_MAXITER)
        _GRAD_REF[row] = (lml, np.concatenate([[rv], ril]))
    return _GRAD_REF[row]


def _assert_every_slot(g, ref, tol, scale, what):
    err = np.abs(g - ref)
    assert np.all(np.isfinite(g)), (what, g)
    assert np.max(err) <= tol * scale, (what, int(np.argmax(err)), float(np.max(err) / scale))
    for slot in range(ref.size):   # each slot on its own: slot 0 the variance, 1 + f feature f
        assert err[slot] <= tol * scale, (what, slot, g[slot], ref[slot])


# fp32 gradient against the fp64 device gradient, relative to the largest slot: the contract of test_gradient.  Every row was
# measured (profiles/laplace/edge_parity.md); all are below a quarter of it, so none needs the one-rounding model's bound.
FP32_GRAD_TOL = 1e-3


@pytest.mark.parametrize("row", ec.GRAD_ROWS, ids=ec.grad_id)
def test_gradient_rows(ctx, row):
    lik, fam, d, n = row
    layout = _ffi.VEC if d == 1 else _ffi.COLVECS
    ref_lml, ref = _reference_gradient(row)
    scale = np.max(np.abs(ref))
    lml, g = _device_gradient(ctx, row, F64, layout)
    print(f"EDGE grad64 {ec.grad_id(row)} lml {abs(lml - ref_lml) / abs(ref_lml):.2e} grad {np.max(np.abs(g - ref)) / scale:.2e}")
    assert abs(lml - ref_lml) <= 1e-10 * abs(ref_lml), (lml, ref_lml)
    _assert_every_slot(g, ref, 1e-6, scale, "fp64")
    if n == 1:
        assert np.all(g[1:] == 0.0) and g[0] != 0.0
    _, g32 = _device_gradient(ctx, row, F32, layout)
    print(f"EDGE grad32 {ec.grad_id(row)} grad {np.max(np.abs(g32 - g)) / scale:.2e}")
    _assert_every_slot(g32, g, FP32_GRAD_TOL, scale, "fp32")
    if n == 1:
        assert np.all(g32[1:] == 0.0) and g32[0] != 0.0


@pytest.mark.parametrize("dtype", [F64, F32])
def test_gradient_through_a_rowvecs_upload(ctx, dtype):
    row = ec.GRAD_ROWVECS_ROW
    ref_lml, ref = _reference_gradient(row)
    scale = np.max(np.abs(ref))
    lml, g = _device_gradient(ctx, row, dtype, _ffi.ROWVECS)
    lml_c, g_c = _device_gradient(ctx, row, dtype, _ffi.COLVECS)
    assert lml == lml_c and _bits(g) == _bits(g_c)   # both uploads end feature-major: the same numbers in the same order
    if dtype == F64:
        assert abs(lml - ref_lml) <= 1e-10 * abs(ref_lml)
        _assert_every_slot(g, ref, 1e-6, scale, "fp64 ROWVECS")
    else:
        _assert_every_slot(g, ref, FP32_GRAD_TOL, scale, "fp32 ROWVECS")


# ---- B. one Newton step from a given start ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("row", ec.STEP_ROWS, ids=ec.step_id)
def test_one_newton_step_from_f_init(ctx, row, dtype):
    lik, fam, n = row
    x, y, il, s2, f_init = ec.step_problem(row, dtype)
    ref, cache, it_ref, conv_ref = lr.fit(lr.kernel_of(fam, ec.VARIANCE, il), x, y, lik, s2, jitter=ec.JITTER, f_init=f_init,
                                          maxiter=1, eps=np.finfo(dtype).eps)
    dev = base._dev(ctx, x.astype(dtype), y.astype(dtype), dtype, _ffi.COLVECS)
    desc, keep = dev.desc(base._kernel(fam, ec.VARIANCE, il), base._lik(lik, s2), ec.JITTER, maxiter=1)
    lml, info = dev.fit(desc, f_init)
    vecs = dict(zip(("f", "g", "W"), dev.mode()))
    dev.free()
    tol_lml, tol_vec = ec.step_tolerances(dtype)
    errs = {k: float(np.max(np.abs(v - cache[k])) / np.max(np.abs(cache[k]))) for k, v in vecs.items()}
    print(f"EDGE step {ec.step_id(row)} {np.dtype(dtype).name} lml {abs(lml - ref) / abs(ref):.2e} " +
          " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert info.iterations == 1 and it_ref == 1
    assert bool(info.converged) == bool(conv_ref)
    assert abs(lml - ref) <= tol_lml * abs(ref), (lml, ref)
    for k in ("f", "g", "W"):
        assert vecs[k].dtype == dtype and np.all(np.isfinite(vecs[k]))
        assert errs[k] <= tol_vec, (k, errs[k])


# ---- C. predictions -----------------------------------------------------------------------------------------------

class _Fitted:
    """a fitted handle of the prediction problem and the reference's cache at the same (dtype-rounded) inputs"""

    def __init__(self, ctx, d, dtype, layout, grad=False):
        self.d, self.dtype = d, dtype
        self.x, y, il = ec.pred_problem(d, dtype)
        self.kernel = lr.kernel_of(ec.PRED_FAMILY, ec.VARIANCE, il)
        self.dev = base._dev(ctx, self.x.astype(dtype), y.astype(dtype), dtype, layout)
        desc, keep = self.dev.desc(base._kernel(ec.PRED_FAMILY, ec.VARIANCE, il), base._lik(ec.PRED_LIK, 1.0), ec.JITTER)
        out = self.dev.lml_grad(desc) if grad else self.dev.fit(desc)
        self.lml, self.info = out[0], out[-1]
        self.y = y
        self._cache = None
        self._model = None

    @property
    def cache(self):
        if self._cache is None:
            _, self._cache, self.it_ref, _ = lr.fit(self.kernel, self.x, self.y, ec.PRED_LIK, jitter=ec.JITTER,
                                                    eps=np.finfo(self.dtype).eps)
        return self._cache

    @property
    def model_cache(self):
        if self._model is None:
            self._model, _ = lr.fit_one_rounding(self.kernel, self.x, self.y, ec.PRED_LIK, jitter=ec.JITTER)
        return self._model

    def points(self, n, seed):
        xs = ec.pred_points(self.d, n, seed, self.dtype)
        return xs[0] if self.d == 1 else xs   # d = 1: a plain vector, the VEC layout of the test inputs too


@pytest.fixture(scope="module")
def fitted(ctx):
    made = {}

    def get(d, dtype, layout=None, grad=False):
        key = (d, np.dtype(dtype).name, layout, grad)
        if key not in made:
            made[key] = _Fitted(ctx, d, dtype, (_ffi.VEC if d == 1 else _ffi.COLVECS) if layout is None else layout, grad)
        return made[key]

    yield get
    for f in made.values():
        f.dev.free()


def _pred_tolerances(dtype, ref_mean):
    """fp64: those of test_predictions; fp32: the fp32 value contract, 1e-4 of the largest mean and 1e-4 of the prior variance"""
    if dtype == F64:
        return 1e-9 * np.max(np.abs(ref_mean)), 1e-9
    return 1e-4 * np.max(np.abs(ref_mean)), 1e-4 * ec.VARIANCE


# the fp32 mean cases measured above a quarter of the 1e-4 contract: they assert 8 x the one-rounding model's error instead
FP32_MEAN_BY_MODEL = {(F32, 1, 1)}


@pytest.mark.parametrize("nstar", ec.PRED_NSTAR)
@pytest.mark.parametrize("d", [2, 1], ids=["colvecs-d2", "vec-d1"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_predictions_at_tile_edges(fitted, dtype, d, nstar):
    """Mean, variance and covariance at n* on both sides of lp_gemm_kernel's 64 x 64 output tile.

    fp32 mean: measured 4.6e-6 ... 5.7e-6 of max |mean| at d = 2 and 1.6e-5 ... 1.7e-5 at d = 1, n* >= 63 - below a quarter
    of the 1e-4 contract, which is what they assert.  The single point of d = 1, n* = 1 measures 2.7e-5, above a quarter: it
    asserts 8 x the one-rounding model of the whole fp32 pipeline instead (lr.fit_one_rounding + lr.predict(one_rounding=True):
    4.2e-6 there, so 3.3e-5), the tighter bound.  The mean is a cancelling sum of g (sum |k* g| / |mean| = 150 at that point),
    so it shows the fp32 mode's error magnified; profiles/laplace/edge_parity.md has the account."""
    h = fitted(d, dtype)
    xs = h.points(nstar, nstar)
    m, v, c = h.dev.predict(xs, cov=True)
    rm, rv, rc = lr.predict(h.cache, h.kernel, h.x, np.atleast_2d(xs))
    tol_m, tol_v = _pred_tolerances(dtype, rm)
    print(f"EDGE pred {np.dtype(dtype).name} d{d} n*{nstar} iters {h.info.iterations}/{h.it_ref} mean {np.max(np.abs(m - rm)) / np.max(np.abs(rm)):.2e} "
          f"var {np.max(np.abs(v - rv)):.2e} cov {np.max(np.abs(c - rc)):.2e}")
    assert m.shape == (nstar,) and v.shape == (nstar,) and c.shape == (nstar, nstar)
    if (dtype, d, nstar) in FP32_MEAN_BY_MODEL:
        mm = lr.predict(h.model_cache, h.kernel, h.x, np.atleast_2d(xs), one_rounding=True)[0]
        model = np.max(np.abs(mm - rm))
        print(f"EDGE pred model mean {model / np.max(np.abs(rm)):.2e}")
        assert 8.0 * model <= tol_m
        tol_m = 8.0 * model
    np.testing.assert_allclose(m, rm, rtol=0, atol=tol_m)
    np.testing.assert_allclose(v, rv, rtol=0, atol=tol_v)
    np.testing.assert_allclose(c, rc, rtol=0, atol=tol_v)
    if dtype == F64:
        np.testing.assert_allclose(np.diag(c), v, rtol=0, atol=1e-12)
        assert np.max(np.abs(c - c.T)) <= 1e-12


@pytest.mark.parametrize("nx,ny", ec.PRED_CROSS)
@pytest.mark.parametrize("d", [2, 1], ids=["colvecs-d2", "vec-d1"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_cross_covariance_shapes(fitted, dtype, d, nx, ny):
    h = fitted(d, dtype)
    xs, ys = h.points(nx, 10 + nx), h.points(ny, 20 + ny)
    c = h.dev.cross_cov(xs, ys)
    rm, _, rc = lr.predict(h.cache, h.kernel, h.x, np.atleast_2d(xs), np.atleast_2d(ys))
    print(f"EDGE cross {np.dtype(dtype).name} d{d} {nx}x{ny} cov {np.max(np.abs(c - rc)):.2e}")
    assert c.shape == (nx, ny)
    np.testing.assert_allclose(c, rc, rtol=0, atol=_pred_tolerances(dtype, rm)[1])
    ct = h.dev.cross_cov(ys, xs)   # the other side of the tile edge: cov(y*, x*) = cov(x*, y*)'
    np.testing.assert_allclose(ct, rc.T, rtol=0, atol=_pred_tolerances(dtype, rm)[1])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_rowvecs_predictions_through_the_c_abi(ctx, fitted, dtype):
    """RowVecs test inputs are reachable through the C ABI only: on a handle made from RowVecs data they give the ColVecs
    handle's numbers bit for bit (both uploads end in the same feature-major storage)."""
    col, row = fitted(2, dtype), fitted(2, dtype, _ffi.ROWVECS)
    assert row.lml == col.lml and row.info.iterations == col.info.iterations
    nx, ny = 65, 130
    xs, ys = col.points(nx, 31), col.points(ny, 32)
    m, v, c = col.dev.predict(xs, cov=True)
    cx = col.dev.cross_cov(xs, ys)
    xr, yr = (np.asfortranarray(a.T.astype(dtype)) for a in (xs, ys))   # (n*, d) column-major: feature-contiguous
    m2, v2 = np.zeros(nx, dtype=dtype), np.zeros(nx, dtype=dtype)
    c2, cx2 = np.zeros((nx, nx), dtype=dtype, order="F"), np.zeros((nx, ny), dtype=dtype, order="F")
    lib = ctx.lib
    assert lib.svgp_laplace_predict(ctx.h, row.dev.h, _ffi.ROWVECS, nx, _ffi._ptr(xr), _ffi._ptr(m2), _ffi._ptr(v2),
                                    _ffi._ptr(c2)) == _ffi.OK
    assert lib.svgp_laplace_predict_cross_cov(ctx.h, row.dev.h, _ffi.ROWVECS, nx, _ffi._ptr(xr), ny, _ffi._ptr(yr),
                                              _ffi._ptr(cx2)) == _ffi.OK
    assert np.any(m != 0) and np.any(cx != 0)
    assert np.array_equal(m2, m) and np.array_equal(v2, v) and np.array_equal(c2, c) and np.array_equal(cx2, cx)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_predictions_after_lml_grad(fitted, dtype):
    """svgp_laplace_lml_grad reuses t1..t3 and allocates R and K R after its fit: the predictions that follow are those of a
    plain fit with the same descriptor from a cold start, bit for bit."""
    plain, grad = fitted(2, dtype), fitted(2, dtype, grad=True)
    assert grad.lml == plain.lml
    xs, ys = plain.points(65, 41), plain.points(64, 42)
    for a, b in zip(plain.dev.predict(xs, cov=True), grad.dev.predict(xs, cov=True)):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    assert np.array_equal(plain.dev.cross_cov(xs, ys), grad.dev.cross_cov(xs, ys))
    for a, b in zip(plain.dev.mode(), grad.dev.mode()):
        assert np.array_equal(a, b)


# ---- D. warm start ------------------------------------------------------------------------------------------------

def _warm_dev(ctx, dtype):
    x, y = ec.warm_problem(dtype)
    return x, y, DeviceLaplace(ctx, x.astype(dtype), y.astype(dtype), dtype)


def _warm_desc(dev, theta, **kw):
    return dev.desc(base._kernel(ec.WARM_FAMILY, theta[0], theta[1]), base._lik(ec.WARM_LIK, 1.0), ec.JITTER, **kw)


def _result(dev, lml, info):
    return (lml, info.iterations, info.converged) + tuple(_bits(v) for v in dev.mode())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_warm_start_at_a_changed_theta(ctx, dtype):
    x, y, dev = _warm_dev(ctx, dtype)
    d1, k1 = _warm_desc(dev, ec.WARM_THETA1)
    _, info1 = dev.fit(d1)
    assert info1.converged
    f1 = dev.mode()[0]
    d2, k2 = _warm_desc(dev, ec.WARM_THETA2, maxiter=1, warm_start=True)
    lml, info = dev.fit(d2)
    vecs = dict(zip(("f", "g", "W"), dev.mode()))
    dev.free()
    ref, cache, it_ref, conv_ref = lr.fit(lr.kernel_of(ec.WARM_FAMILY, *ec.WARM_THETA2), x, y, ec.WARM_LIK, jitter=ec.JITTER,
                                          f_init=f1.astype(np.float64), maxiter=1, eps=np.finfo(dtype).eps)
    tol_lml, tol_vec = ec.step_tolerances(dtype)
    assert info.iterations == 1 and bool(info.converged) == bool(conv_ref) and not conv_ref
    assert abs(lml - ref) <= tol_lml * abs(ref), (lml, ref)
    for k, v in vecs.items():
        assert np.max(np.abs(v - cache[k])) <= tol_vec * np.max(np.abs(cache[k])), k
    # and the step did start at f1, not at zero: from zero the reference lands elsewhere by far more than the tolerance
    cold = lr.fit(lr.kernel_of(ec.WARM_FAMILY, *ec.WARM_THETA2), x, y, ec.WARM_LIK, jitter=ec.JITTER, maxiter=1)[1]["f"]
    assert np.max(np.abs(cold - cache["f"])) > 100 * tol_vec * np.max(np.abs(cache["f"]))


def test_explicit_f_init_wins_over_warm_start(ctx):
    x, y, dev = _warm_dev(ctx, F64)
    f_init = 0.5 * np.cos(2.0 * x[1])
    d1, k1 = _warm_desc(dev, ec.WARM_THETA1)
    dev.fit(d1)   # the handle now holds a mode a warm start would use
    dw, kw = _warm_desc(dev, ec.WARM_THETA2, maxiter=2, warm_start=True)
    warm = _result(dev, *dev.fit(dw, f_init))
    dc, kc = _warm_desc(dev, ec.WARM_THETA2, maxiter=2, warm_start=False)
    cold = _result(dev, *dev.fit(dc, f_init))
    from_mode = _result(dev, *dev.fit(dw))
    dev.free()
    assert warm == cold
    assert from_mode[3] != cold[3]   # the same descriptor without f_init does start elsewhere (from the previous mode)


def test_warm_start_after_a_failed_call_is_a_cold_start(ctx):
    x, y, dev = _warm_dev(ctx, F64)
    d1, k1 = _warm_desc(dev, ec.WARM_THETA1)
    dev.fit(d1)
    bad, kb = _warm_desc(dev, ec.WARM_THETA2, warm_start=True)
    bad.variance = 0.0
    lml, info = C.c_double(), _ffi.LaplaceInfo()
    assert ctx.lib.svgp_laplace_fit(ctx.h, dev.h, C.byref(bad), None, C.byref(lml), C.byref(info)) == _ffi.INVALID_ARG
    assert ctx.lib.svgp_laplace_mode(ctx.h, dev.h, None, None, None) == _ffi.INVALID_ARG   # the failed call left no mode
    d2, k2 = _warm_desc(dev, ec.WARM_THETA2, maxiter=2, warm_start=True)
    after = _result(dev, *dev.fit(d2))
    dev.free()
    x, y, fresh = _warm_dev(ctx, F64)
    d3, k3 = _warm_desc(fresh, ec.WARM_THETA2, maxiter=2, warm_start=True)
    first = _result(fresh, *fresh.fit(d3))
    fresh.free()
    assert after == first


# ---- E. non-finite inputs -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["y", "x", "f_init"])
def test_a_nan_never_gives_a_finite_lml(ctx, where):
    """An ordinary call with one bad number.  lp_point_kernel's sqrt(fmax(W, 0)) turns a NaN W into sW = 0, which keeps B
    finite: the NaN has to reach the lml through b = W f + g and the log-likelihood sum, as the reference's arithmetic has it."""
    lik = 3 if where == "y" else 1
    n = 64
    x, y = lr.synth(lik, n, 2, seed=23)
    il = np.array([0.8, 1.1])
    xb, yb, f_init = x.copy(), y.copy(), None
    if where == "y":
        yb[17] = np.nan
    elif where == "x":
        xb[1, 40] = np.nan
    else:
        f_init = np.zeros(n)
        f_init[5] = np.nan
    dev = DeviceLaplace(ctx, xb, yb, F64)
    desc, keep = dev.desc(base._kernel(ec.SE, ec.VARIANCE, il), base._lik(lik, 1.0), ec.JITTER, maxiter=3)
    lml, info = C.c_double(1.25), _ffi.LaplaceInfo()
    rc = ctx.lib.svgp_laplace_fit(ctx.h, dev.h, C.byref(desc), None if f_init is None else _ffi._ptr(f_init), C.byref(lml),
                                  C.byref(info))
    assert rc in (_ffi.OK, _ffi.NOT_POSDEF), rc
    assert np.isnan(lml.value), (rc, lml.value)
    f = np.zeros(n)
    rc_mode = ctx.lib.svgp_laplace_mode(ctx.h, dev.h, _ffi._ptr(f), None, None)
    if rc != _ffi.OK:
        assert rc_mode == _ffi.INVALID_ARG   # no mode after a failure
    else:
        assert rc_mode == _ffi.INVALID_ARG or not np.all(np.isfinite(f))   # never a finite "mode" beside a NaN lml
    dev.free()
    # a healthy fit on a fresh handle of the same context
    good = DeviceLaplace(ctx, x, y, F64)
    desc, keep = good.desc(base._kernel(ec.SE, ec.VARIANCE, il), base._lik(lik, 1.0), ec.JITTER)
    val, _ = good.fit(desc)
    good.free()
    ref = lr.fit(lr.kernel_of(ec.SE, ec.VARIANCE, il), x, y, lik, jitter=ec.JITTER)[0]
    assert abs(val - ref) <= 1e-9 * abs(ref), (val, ref)
