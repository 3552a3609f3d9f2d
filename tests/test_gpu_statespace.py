"""GPU tests of the exact one-dimensional Matern GP in O(N) (svgp_ss_*, approxgp.StateSpace): the parallel-scan Kalman filter and RTS
smoother against the dense float64 exact GP of tests/statespace_ref.py.  Tolerances: 10 x the larger of the device's and the sequential
float64 reference's measured distance to the dense GP (profiles/statespace/accuracy.md), below the fp64 contract of 1e-8."""
import ctypes as C
import functools

import numpy as np
import pytest

import approxgp
import statespace_ref as R
from approxgp import _ffi
from approxgp.statespace import DeviceStateSpace

pytestmark = pytest.mark.gpu

# (relative for the lml, in units of the prior variance for the moments) per group of cases; float32 handles round the moments once more
LML_RTOL = {"regular": 5.6e-14, "long": 1.4e-12}
MEAN_ATOL = {"regular": 7.6e-13, "long": 2.8e-12}
VAR_ATOL = {"regular": 1.7e-13, "long": 4.2e-14}
F32_EPS = 2.0 ** -24

CASES = [(N, "plain") for N in R.SIZES + (R.RECURSIVE_N,)] + [(2 * R.TILE + 1, k) for k in R.KINDS[1:]]


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def reference(family, N, kind):
    p = R.problem(N, kind)
    return p, R.dense(family, p["variance"], p["inv_lengthscale"], p["t"], p["y"] - p["mean_const"], p["sig2"], p["ts"])


def kernel_of(family, p):
    base = approxgp.Matern32Kernel() if family == 1 else approxgp.Matern52Kernel()
    return p["variance"] * approxgp.with_lengthscale(base, 1.0 / p["inv_lengthscale"])


def run(ctx, family, dtype, p):
    dev = DeviceStateSpace(ctx, p["t"], p["y"], dtype)
    try:
        if np.ndim(p["sig2"]):
            dev.set_noise(p["sig2"] - 0.125)
        desc = dev.desc(kernel_of(family, p), 0.125, p["mean_const"])
        out = []
        for _ in range(2):
            lml, info = dev.fit(desc)
            out.append((lml,) + dev.predict(p["ts"]))
        return out, info
    finally:
        dev.free()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("N,kind", CASES)
def test_lml_and_marginals_match_the_dense_gp(ctx, family, dtype, N, kind):
    p, (lml_d, mean_d, var_d) = reference(family, N, kind)
    (first, second), info = run(ctx, family, dtype, p)
    assert info.state_dim == family + 1 and info.n_tiles == -(-N // R.TILE) and info.levels == (1 if N <= R.TILE else 3 if N > R.TILE ** 2 else 2)
    lml, mean, var = first
    v, g = p["variance"], "long" if kind == "long" else "regular"
    e_lml = abs(lml - lml_d) / abs(lml_d)
    e_mean = np.abs(mean - p["mean_const"] - mean_d).max() / v
    e_var = np.abs(var - var_d).max() / v
    print(f"ss accuracy family={family} {np.dtype(dtype).name} N={N} {kind}: lml {e_lml:.2e} mean {e_mean:.2e} var {e_var:.2e}")
    r32 = F32_EPS * (np.abs(mean_d).max() + abs(p["mean_const"]) + v) / v if dtype == np.float32 else 0.0
    assert e_lml <= LML_RTOL[g]
    assert e_mean <= MEAN_ATOL[g] + r32 and e_var <= VAR_ATOL[g] + r32
    assert mean.dtype == dtype and var.dtype == dtype
    # a repeated call returns the same bits
    assert second[0] == lml and np.array_equal(second[1], mean) and np.array_equal(second[2], var)


def test_unsorted_inputs_come_back_in_the_callers_order(ctx):
    p, (lml_d, mean_d, var_d) = reference(2, 2 * R.TILE + 1, "noise")
    rng = np.random.default_rng(1)
    pd, pt = rng.permutation(p["t"].shape[0]), rng.permutation(p["ts"].shape[0])
    f = approxgp.GP(p["mean_const"], kernel_of(2, p))
    fx = f(p["t"][pd], approxgp.Diagonal(p["sig2"][pd]))
    assert abs(approxgp.approx_lml(approxgp.StateSpace(), fx, p["y"][pd], ctx=ctx) - lml_d) <= LML_RTOL["regular"] * abs(lml_d)
    post = approxgp.posterior(approxgp.StateSpace(), fx, p["y"][pd], ctx=ctx)
    try:
        m, v = post.mean_and_var(p["ts"][pt])
        np.testing.assert_allclose(m - p["mean_const"], mean_d[pt], rtol=0, atol=MEAN_ATOL["regular"] * p["variance"])
        np.testing.assert_allclose(v, var_d[pt], rtol=0, atol=VAR_ATOL["regular"] * p["variance"])
        ym, yv = post.predict_y(p["ts"][pt], noise=0.25)
        np.testing.assert_allclose(yv, v + 0.25, rtol=1e-14)
        lpd = post.log_predictive_density(p["ts"][pt], np.zeros(pt.shape[0]), noise=0.25)
        np.testing.assert_allclose(lpd, -0.5 * (np.log(2 * np.pi * yv) + ym ** 2 / yv), rtol=1e-12)
    finally:
        post.free()
    # any other prior mean, as offsets: the same lml as the dense GP of y - offsets
    off = 0.1 * p["t"]
    lml_o = approxgp.approx_lml(approxgp.StateSpace(), fx, p["y"][pd], ctx=ctx, mean_offsets=off[pd])
    ref_o = R.dense(2, p["variance"], p["inv_lengthscale"], p["t"], p["y"] - p["mean_const"] - off, p["sig2"], p["ts"][:1])[0]
    assert abs(lml_o - ref_o) <= LML_RTOL["regular"] * abs(ref_o)


def test_status_codes(ctx):
    lib, t = ctx.lib, np.linspace(0.0, 1.0, 9)
    h = C.c_void_p()
    d2 = _ffi.DeviceData(ctx, np.zeros((2, 9)), np.zeros(9), np.float64)
    assert lib.svgp_ss_create(ctx.h, d2.h, C.byref(h)) == _ffi.UNSUPPORTED          # d = 2
    d2.free()
    du = _ffi.DeviceData(ctx, t[::-1].copy(), np.zeros(9), np.float64, _ffi.VEC)
    assert lib.svgp_ss_create(ctx.h, du.h, C.byref(h)) == _ffi.INVALID_ARG           # unsorted at the C level
    du.free()
    dev = DeviceStateSpace(ctx, t, np.zeros(9), np.float64)
    try:
        lml = C.c_double()
        fit = lambda ds: lib.svgp_ss_fit(ctx.h, dev.h, C.byref(ds), None, C.byref(lml), None)
        assert fit(dev.desc(approxgp.SqExponentialKernel(), 0.1)) == _ffi.UNSUPPORTED   # SE has no finite state
        assert fit(dev.desc(approxgp.Matern32Kernel(), 0.0)) == _ffi.INVALID_ARG        # diag = 0
        m = np.zeros(2)
        assert lib.svgp_ss_predict(ctx.h, dev.h, 2, _ffi._ptr(np.array([0.1, 0.2])), _ffi._ptr(m), None) == _ffi.INVALID_ARG   # no fit yet
        assert fit(dev.desc(approxgp.Matern32Kernel(), 0.1)) == _ffi.OK
        assert lib.svgp_ss_predict(ctx.h, dev.h, 2, _ffi._ptr(np.array([0.2, 0.1])), _ffi._ptr(m), None) == _ffi.INVALID_ARG   # unsorted test times
    finally:
        dev.free()
