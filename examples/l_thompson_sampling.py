#!/usr/bin/env python
"""Thompson sampling with pathwise function samples: the maximiser of each sampled function, climbed with the device gradient
(svgp_sampler_eval_grad).  A posterior sample drawn by pathwise conditioning is a FUNCTION; one acquisition step of Thompson sampling
(Wilson et al. 2020, section 5) maximises each drawn function and proposes its maximiser.

  * the model of examples/k_function_samples.py (SE kernel, M = 20, the optimal q(u) of its training data) and 8 functions from it;
  * 48 starts per function on [-1, 1], climbed by gradient ascent; the points, the values and the gradients stay in device memory
    (torch tensors, wrapped without a copy as in examples/d_input_gradients.py), one svgp_sampler_eval_grad call per step;
  * each function's maximiser, checked against that function's maximum on a dense grid of fs(x).

The call evaluates EVERY function at EVERY point: the example lays the starts of all functions out in one row of points and takes, of
the (S, d, points) gradient, the block of each function's own starts.  A per-point choice of the sample (evaluating only function s at
the starts of function s) is out of the call's scope: with S = 8 it would save 7/8 of the products, not of the tile generation, which is
the larger share of the kernel's time.

    python examples/l_thompson_sampling.py      # needs an MI355X
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402
from approxgp import _ffi  # noqa: E402


def main(n_functions=8, n_starts=48, n_features=2048, n_steps=400, n_grid=20_001, seed=7):
    rng = np.random.default_rng(seed)
    N, M, noise, jitter = 10_000, 20, 0.3, 1e-5
    x = rng.uniform(-1, 1, N)
    y = np.sin(3 * np.pi * x) + 0.3 * np.cos(9 * np.pi * x) + 0.5 * np.sin(7 * np.pi * x) + np.sqrt(noise) * rng.standard_normal(N)
    var, ell = 1.3, 0.12
    z = np.linspace(-1, 1, M)
    ctx = _ffi.Context(0, torch.cuda.current_stream().cuda_stream)   # the library's work is ordered with torch's on one stream
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    model = _ffi.DeviceModel(ctx, *_ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, [1.0 / ell], z, np.zeros(M), np.eye(M), jitter,
                                                  lik_sigma2=noise))
    bound, m, Lq = model.collapsed_q(data)
    model.free()
    data.free()
    f = ag.GP(var * ag.with_lengthscale(ag.SqExponentialKernel(), ell))
    post = ag.posterior(ag.SparseVariationalApproximation(f(z, jitter), ag.MvNormal.from_cholesky(m, Lq)), ctx=ctx)
    fs = post.function_samples(n_functions, n_features=n_features, rng=rng)
    S, K = n_functions, n_starts
    P = S * K

    # the starts of function s are the points s K .. (s + 1) K - 1; everything below lives in device memory
    xt = torch.linspace(-1.0, 1.0, K, dtype=torch.float64, device="cuda").repeat(S).reshape(1, P).contiguous()
    F = torch.empty((S, P), dtype=torch.float64, device="cuda")
    G = torch.empty((S, 1, P), dtype=torch.float64, device="cuda")
    pts = _ffi.DeviceData.wrap(ctx, np.float64, 1, P, P, xt.data_ptr(), None)   # no copy: the call reads xt where torch updates it
    own = torch.arange(S, device="cuda").repeat_interleave(K)                   # the function each point belongs to
    col = torch.arange(P, device="cuda")
    step = 0.25 * ell * ell / var     # the curvature of a sample is of order variance / lengthscale^2
    for _ in range(n_steps):
        fs.sampler.eval_grad(pts, out=F, grad_out=G)
        xt.add_(step * G[own, 0, col]).clamp_(-1.0, 1.0)
    fs.sampler.eval_grad(pts, out=F, grad_out=G)
    torch.cuda.synchronize()
    val = F[own, col].reshape(S, K)                      # function s at its own starts
    grd = G[own, 0, col].reshape(S, K)
    best = val.argmax(dim=1)
    rows = torch.arange(S, device="cuda")
    x_best = xt.reshape(S, K)[rows, best].cpu().numpy()
    f_best = val[rows, best].cpu().numpy()
    g_best = grd[rows, best].cpu().numpy()
    pts.free()

    grid = np.linspace(-1, 1, n_grid)
    Fg = fs(grid)                                        # (n_grid, S): the same functions on a dense grid
    fs.free()
    print(f"collapsed bound {bound:.2f}; {S} functions, {K} starts each, {n_steps} ascent steps of one svgp_sampler_eval_grad call on {P} points")
    worst = -np.inf
    for s in range(S):
        j = int(Fg[:, s].argmax())
        gap = Fg[j, s] - f_best[s]
        worst = max(worst, gap)
        print(f"function {s}: maximiser {x_best[s]:+.5f}  f = {f_best[s]:+.6f}  |f'| = {abs(g_best[s]):.1e}    "
              f"grid: {grid[j]:+.5f}  f = {Fg[j, s]:+.6f}  (grid - climbed: {gap:+.1e})")
        interior = abs(x_best[s]) < 1.0
        assert gap <= 1e-5, "the climb found a lower maximum than the dense grid"
        assert abs(x_best[s] - grid[j]) <= 2e-3, "the maximiser is not the grid's"
        assert not interior or abs(g_best[s]) <= 1e-2, "the gradient does not vanish at an interior maximiser"
    print(f"every maximiser agrees with the dense grid (largest grid - climbed value {worst:+.1e}; negative: the climb is finer than the grid)")
    return x_best, f_best


if __name__ == "__main__":
    main()
