"""GPU checks of the compile-time buffer rotation of the asynchronous k-loop (csrc/device_common.hpp: TileGemm::rstep,
loop_tri_async_w), at the smallest shapes at which the rotation can go wrong.

A loop of n regular steps runs n % 3 left-over steps first (tiles displaced by (3 - n % 3) % 3 LDS buffers), then trips of three
steps; phase 1 of the strips appends eight triangular steps, phase 2 starts with eight and ends with its left-over steps.  So:
  * 1, 2, 3 and 5 panels (M = 100, 200, 300, 640): phase-1 loops of 0, 8, 16, 24, 32 regular steps - every left-over count, a loop
    without any trip, loops of one and several trips; phase-2 loops of 0 .. 32 regular steps behind the head likewise;
  * every strip width: f64 32 / 64 points (strip_plan: the 64-point kernel above 16 384 points), fp32 64 / 128 points (above 32 768);
  * the segmented strips beside the factorisation (5 panels, SVGP_OVERLAP unset) against the single launch (SVGP_OVERLAP=0);
  * the SYRK of the value-and-gradient evaluation (TRI = 0), loops of 1, 2, 3, 4 and 5 steps, unweighted (Gaussian) and weighted
    (Bernoulli); phase 3 of its strips (TRI = 0, 8 / 24 steps);
  * phase 1 alone (the collapsed bound).

The slicing rule of the SYRK (csrc/api_grad.hip: syrk_slices, grad_chunk_points; csrc/grad.hip: syrk_async_kernel), restated: a call
of N <= 65 536 points is one chunk of ncp = ceil128(N) points; it is cut into ns = min(64, ncp / 512) slices (at least 1; for M <= 384
on a device of >= 64 CUs) of sl = ceil16(ceil(ncp / ns)) points, the last slice takes what is left.  A slice of L points is a loop of
ceil(L / 16) steps.
  Gaussian (uniform weights): the kernel covers n16 = ceil16(N) points, so N <= 80 is ONE slice of ceil(N / 16) steps:
    N = 16, 32, 48, 64, 80 -> 1, 2, 3, 4, 5 steps.
  Bernoulli (weighted): the kernel covers ncp points, a single slice has >= 8 steps; with ns slices of 528 points (33 steps) the last
    one is short:  ncp = 18 560 (ns 36) -> 80 points = 5 steps, 19 072 (37) -> 4, 19 584 (38) -> 3, 20 096 (39) -> 2,
    20 608 (40) -> 1.  N is taken 5 below ncp."""
import contextlib
import functools
import os

import numpy as np
import pytest

import collapsed_ref as cr
import svgp_oracle as o
from approxgp import _ffi
from helpers import context_with_env, device_model, rel

pytestmark = pytest.mark.gpu

F64_RTOL, F32_RTOL = 1e-8, 1e-4     # the suite's tolerances (tests/test_gpu_parity.py)
MS = (100, 200, 300, 640)           # 1, 2, 3, 5 panels
D = 3


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _forward_problem(N, M, f32):
    """(x, y, sva, sigma2, oracle ELBO) - computed once, arrays read-only."""
    x, y, sva, s2 = o.synth_problem(700 + M, N, M, D, dtype=np.float32 if f32 else np.float64)
    ref = o.elbo(sva, x, y, sigma2=s2, num_data=2.0 * N)
    for a in (x, y):
        a.setflags(write=False)
    return x, y, sva, s2, ref


def _elbo(c, N, M, f32, calls=1):
    x, y, sva, s2, ref = _forward_problem(N, M, f32)
    dtype = np.float32 if f32 else np.float64
    model = device_model(c, sva, dtype=dtype, sigma2=s2)
    data = _ffi.DeviceData(c, x, y, dtype)
    try:
        return [model.elbo(data, 0, N, 2.0 * N)[0] for _ in range(calls)], ref
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("N", [200, 16_400])     # the half-width 32-point kernel; the full-width 64-point kernel (the flagship's)
@pytest.mark.parametrize("M", MS)
def test_forward_f64(ctx, N, M):
    vals, ref = _elbo(ctx, N, M, False, calls=3)
    print(f"N {N} M {M}: elbo {vals[0]:.15g} oracle {ref:.15g} rel {rel(vals[0], ref):.2e}")
    assert rel(vals[0], ref) <= F64_RTOL
    assert vals[1] == vals[0] and vals[2] == vals[0]      # identical bits


@pytest.mark.parametrize("N", [200, 32_900])     # 64- and 128-point strips
@pytest.mark.parametrize("M", MS)
def test_forward_f32(ctx, N, M):
    vals, ref = _elbo(ctx, N, M, True)
    print(f"N {N} M {M}: elbo {vals[0]:.9g} oracle {ref:.9g} rel {rel(vals[0], ref):.2e}")
    assert rel(vals[0], ref) <= F32_RTOL


@contextlib.contextmanager
def _context_without(name):
    """A fresh context created with `name` absent from the environment; the ambient value is restored."""
    old = os.environ.pop(name, None)
    try:
        c = _ffi.Context(0)
    finally:
        if old is not None:
            os.environ[name] = old
    try:
        yield c
    finally:
        c.close()


def test_segmented_strips_equal_the_single_launch():
    with _context_without("SVGP_OVERLAP") as c_on, context_with_env(SVGP_OVERLAP="0") as c_off:
        (v_on,), ref = _elbo(c_on, 200, 640, False)
        (v_off,), _ = _elbo(c_off, 200, 640, False)
    assert rel(v_on, ref) <= F64_RTOL
    assert v_on == v_off                                  # bitwise


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-12)
    assert np.abs(a - b).max() <= tol * scale, (np.abs(a - b).max(), scale)


GRAD_N = {o.LIK_GAUSSIAN: (16, 32, 48, 64, 80),                                          # 1 .. 5 steps (see the module's docstring)
          o.LIK_BERNOULLI_LOGISTIC: (20_603, 20_091, 19_579, 19_067, 18_555)}            # last slice of 1 .. 5 steps


@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("lik", [o.LIK_GAUSSIAN, o.LIK_BERNOULLI_LOGISTIC])
@pytest.mark.parametrize("M", [100, 300])
def test_value_and_gradient_f64(ctx, M, lik, steps):
    """The route and the tolerances of tests/test_gpu_grad.py::test_gradient_matches_oracle (fp64: value 1e-8, gradient blocks 1e-6 of
    their max-norm)."""
    N, tol = GRAD_N[lik][steps - 1], 1e-6
    x, y, sva, s2 = o.synth_problem(300 + N, N, M, D, lik=lik)
    sva.mean_const = 0.1
    val_ref, g_ref = o.elbo_grad(sva, x, y, lik=lik, sigma2=s2, num_data=2.5 * N)
    model = device_model(ctx, sva, dtype=np.float64, lik=lik, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    try:
        val, terms, g = model.elbo_grad(data, 0, N, 2.5 * N)
        print(f"M {M} lik {lik} N {N}: value rel {rel(val, val_ref):.2e}")
        assert rel(val, val_ref) < 1e-8
        _close(g["m"], g_ref["m"], tol)
        _close(g["Lq"], g_ref["Lq"], tol)
        _close(g["z"].reshape(g_ref["z"].shape, order="F"), g_ref["z"], tol)
        _close(g["inv_lengthscale"], g_ref["inv_lengthscale"], tol)
        _close([g["variance"]], [g_ref["variance"]], tol)
        _close([g["mean_const"]], [g_ref["mean_const"]], tol)
        if lik == o.LIK_GAUSSIAN:
            _close([g["lik_sigma2"]], [g_ref["lik_sigma2"]], tol)
    finally:
        model.free()
        data.free()


def test_collapsed_bound_phase_one_alone(ctx):
    n, M = 16_400, 300
    kernel, z, x, y, s2 = cr.problem(n, M, D, family=o.KERNEL_SE, ard=True)
    ref = cr.collapsed(kernel, z, 1e-5, x, s2, y)
    q = o.SVA(kernel, z, np.zeros(M), np.eye(M), jitter=1e-5)
    model = device_model(ctx, q, dtype=np.float64, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    try:
        val, t = model.collapsed_bound(data, 0, n)
        print(f"bound {val:.12g} ref {ref.bound:.12g} rel {rel(val, ref.bound):.2e}")
        assert rel(val, ref.bound) < 1e-8                 # tests/test_gpu_collapsed.py's fp64 tolerance
        assert model.collapsed_bound(data, 0, n)[0] == val
    finally:
        model.free()
        data.free()
