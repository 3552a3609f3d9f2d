#!/usr/bin/env python
"""Function samples from a fitted SVGP, evaluated anywhere on the device (pathwise conditioning, svgp_sampler_*): the last step of the
reference's examples - `rand(post(x), 20)` - as FUNCTIONS that can be evaluated on a plot grid, then on a finer one, then at the
candidates of a Thompson-sampling step, always the same functions.

  * the model of examples/a_regression.py (SE kernel, M = 20) with the optimal q(u) for its training data (svgp_collapsed_q);
  * 16 functions on a grid of 10^6 points: one data pass, linear in the grid, nothing n x n;
  * the same functions again on a 500-point subset: bitwise the grid's values;
  * moments of 512 functions on that subset against svgp_predict's mean and variance.

    python examples/k_function_samples.py      # needs an MI355X
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402
from approxgp import _ffi  # noqa: E402


def main(n_grid=1_000_000, n_features=2048, seed=7):
    rng = np.random.default_rng(seed)
    N, M, noise, jitter = 10_000, 20, 0.3, 1e-5
    x = rng.uniform(-1, 1, N)
    y = np.sin(3 * np.pi * x) + 0.3 * np.cos(9 * np.pi * x) + 0.5 * np.sin(7 * np.pi * x) + np.sqrt(noise) * rng.standard_normal(N)
    var, ell = 1.3, 0.12
    z = np.linspace(-1, 1, M)
    ctx = _ffi.default_context()
    # "training": the optimal q(u) of the collapsed bound at fixed hyperparameters, computed on the device
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    model = _ffi.DeviceModel(ctx, *_ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, [1.0 / ell], z, np.zeros(M), np.eye(M), jitter,
                                                  lik_sigma2=noise))
    bound, m, Lq = model.collapsed_q(data)
    model.free()
    data.free()
    f = ag.GP(var * ag.with_lengthscale(ag.SqExponentialKernel(), ell))
    post = ag.posterior(ag.SparseVariationalApproximation(f(z, jitter), ag.MvNormal.from_cholesky(m, Lq)), ctx=ctx)

    fs = post.function_samples(16, n_features=n_features, rng=rng)
    grid = np.linspace(-1, 1, n_grid)
    fs(grid[:1000])                                  # warm-up
    t0 = time.perf_counter()
    F = fs(grid)                                     # (n_grid, 16)
    dt = time.perf_counter() - t0
    print(f"collapsed bound {bound:.2f}; 16 functions on {n_grid} points in {1e3 * dt:.1f} ms (upload, one data pass, download)")
    idx = np.linspace(0, n_grid - 1, 500).astype(int)
    again = fs(grid[idx])
    assert np.array_equal(again, F[idx]), "a sample is a function: the same values wherever it is evaluated again"
    print("the same 16 functions on a 500-point subset: bitwise the grid's values")
    fs.free()

    many = post.function_samples(512, n_features=n_features, rng=rng)
    G = many(grid[idx])                              # (500, 512)
    many.free()
    mean, v = post.mean_and_var(grid[idx])
    zmean = np.abs(G.mean(axis=1) - mean) / (G.std(axis=1, ddof=1) / np.sqrt(512))   # in the samples' own standard errors
    verr = np.abs(G.var(axis=1, ddof=1) - v)
    print(f"512 functions against svgp_predict on the subset: |sample mean - mean| = {zmean.mean():.2f} standard errors on average "
          f"(max {zmean.max():.2f}); |sample variance - variance| <= {verr.max():.4f} (variance {v.min():.4f} .. {v.max():.4f}, "
          f"kernel variance {var}; the Fourier part's error is O(kernel variance / sqrt(L)) = {var / np.sqrt(n_features):.3f})")
    assert zmean.max() < 6.0 and verr.max() < 0.1 * var
    return F, G


if __name__ == "__main__":
    main()
