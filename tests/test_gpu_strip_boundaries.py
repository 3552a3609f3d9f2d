"""The forward strips outside their k-loops (csrc/strip.hip): the pre-generation of Kuf (pregen_mfma; the f64 SE register body is
software-pipelined: z rows prefetched a block ahead, the distance MFMAs of all column tiles ahead of the exponentials, the
exponentials stage by stage) and the panel epilogues (a call without optional outputs runs one straight block per panel, addresses
as scalar base + per-lane offset + immediate).  Neither may change a result, so every case here is a parity check against the CPU
oracle (oracle/svgp_oracle.py) at the suite's tolerances (tests/test_gpu_parity.py), on the smallest shapes at which that code takes
another path:

  M = 128 ... 640      one to five 128-row panels (every remainder of the k-loop's three-buffer rotation, the single-panel model, the
                       hand-over from phase 1 to phase 2)
  M = 200, 130         the 16-row block that straddles M (masked store form) and a padded panel
  N = 1 ... 64 * 7 + 5 a single point, one short / exact / just over one strip, several strips with a ragged end
  N = 512 * 64 + 3 * 64 + 5 at M = 256: more strips than workgroups, so some workgroups run a second strip (the z prefetch and the
                       per-lane offsets live across the strip loop)
  d = 3, 8, 9, 16, 17  the 8- and 16-feature register bodies and the wide-input body
  SE / Matern-3/2 / Matern-5/2, f64 and f32
  a NaN coordinate     must still reach the results of its point, and of that point only
  4 096 points on their own and inside a 40 000-point batch: equal bits (the small batch runs as half-width strips and, from five
                       panels on, beside the factorisation as segmented launches, which keep the block-at-a-time pre-generation)."""
import functools

import numpy as np
import pytest

import svgp_oracle as o
from approxgp import _ffi
from helpers import device_model, rel

pytestmark = pytest.mark.gpu

F64_RTOL, F32_RTOL = 1e-8, 1e-4   # the suite's: tests/test_gpu_parity.py
# The fp32 problems take the jitter the suite's fp32 sweeps take (test_randomized_shapes_and_models, tests/fuzz_families.py).  The
# marginal MEAN is A'm with A = Lk \ Kuf in fp32: its error grows with cond(Kuu), and at the recipe's default jitter the 512-inducing-
# point problem is at 1.2e-4 of the largest mean - with the parent's library too, bit for bit - which says nothing about the strips.
F32_JITTER = 1e-2

DTYPES = [(np.float64, F64_RTOL), (np.float32, F32_RTOL)]
N_RAGGED = 64 * 7 + 5


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _reference(N, M, d, family, f32):
    """Problem and oracle results, computed once per shape and shared; nothing modifies them."""
    dtype = np.float32 if f32 else np.float64
    x, y, sva, s2 = o.synth_problem(8000 + M + d, N, M, d, family=family, dtype=dtype, jitter=F32_JITTER if f32 else None)
    ref = o.elbo_terms(sva, x, y, sigma2=s2, num_data=2.0 * N)
    mu, var = o.mean_and_var(o.posterior(sva), x)
    for a in (x, y, mu, var):
        a.setflags(write=False)
    return x, y, sva, s2, ref, mu, var


def _block_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _check(ctx, N, M, d, family, dtype, tol):
    x, y, sva, s2, ref, mu_ref, var_ref = _reference(N, M, d, family, dtype == np.float32)
    model = device_model(ctx, sva, dtype=dtype, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, dtype)
    try:
        val, t = model.elbo(data, 0, N, 2.0 * N)
        mu, var = model.marginals(data)
    finally:
        model.free()
        data.free()
    errs = (rel(val, ref.elbo), rel(t.expectation, ref.expectation), _block_err(mu, mu_ref), _block_err(var, var_ref))
    print(f"N={N} M={M} d={d} family={family} {np.dtype(dtype).name}: elbo {errs[0]:.2e} expectation {errs[1]:.2e} "
          f"mean {errs[2]:.2e} var {errs[3]:.2e} (tol {tol:g})")
    assert t.n_points == N and t.n_neg_var == 0
    assert max(errs) < tol, errs


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("M", [128, 256, 384, 512, 640, 200, 130])
def test_panel_counts_and_padded_panels(ctx, M, dtype, tol):
    _check(ctx, N_RAGGED, M, 8, o.KERNEL_SE, dtype, tol)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_batch_sizes_around_one_strip(ctx, N, dtype, tol):
    _check(ctx, N, 256, 8, o.KERNEL_SE, dtype, tol)


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_workgroups_take_a_second_strip(ctx, dtype, tol):
    _check(ctx, 512 * 64 + 3 * 64 + 5, 256, 8, o.KERNEL_SE, dtype, tol)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
@pytest.mark.parametrize("d", [3, 8, 9, 16, 17])
def test_input_dimensions_and_families(ctx, d, family, dtype, tol):
    _check(ctx, N_RAGGED, 200, d, family, dtype, tol)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_nan_coordinate_still_gives_nan(ctx, dtype):
    """The clamp in front of the staged exponentials must let a NaN through exactly as the block-at-a-time body does."""
    N, M, bad = N_RAGGED, 256, 77
    x, y, sva, s2 = _reference(N, M, 8, o.KERNEL_SE, dtype == np.float32)[:4]
    xb = x.copy()
    xb[5, bad] = np.nan
    model = device_model(ctx, sva, dtype=dtype, sigma2=s2)
    clean, dirty = _ffi.DeviceData(ctx, x, y, dtype), _ffi.DeviceData(ctx, xb, y, dtype)
    try:
        mu0, v0 = model.marginals(clean)
        mu1, v1 = model.marginals(dirty)
        elbo_dirty = model.elbo(dirty, 0, N, float(N))[0]
    finally:
        for h in (model, clean, dirty):
            h.free()
    keep = np.arange(N) != bad
    assert np.isnan(mu1[bad]) and np.isnan(v1[bad])
    assert np.array_equal(mu0[keep], mu1[keep]) and np.array_equal(v0[keep], v1[keep])
    assert not np.isfinite(elbo_dirty)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [256, 640])
def test_a_small_batch_has_the_bits_of_the_large_one(ctx, M, dtype):
    """4 096 points evaluated on their own - first, on a fresh model: half-width strips, and at five panels segmented launches beside
    the factorisation - and as part of a 39 900-point batch (full-width strips, one launch)."""
    x, y, sva, s2 = o.synth_problem(8100 + M, 40000, M, 8, dtype=dtype)
    model = device_model(ctx, sva, dtype=dtype, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, dtype)
    try:
        mu_s, var_s = model.marginals(data, 100, 4096)
        mu_l, var_l = model.marginals(data, 100, 39900)
    finally:
        model.free()
        data.free()
    assert np.isfinite(mu_l).all() and np.isfinite(var_l).all()
    assert np.array_equal(mu_s, mu_l[:4096]) and np.array_equal(var_s, var_l[:4096])
