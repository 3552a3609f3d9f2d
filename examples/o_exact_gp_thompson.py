#!/usr/bin/env python
"""Thompson sampling on an EXACT GP: examples/l_thompson_sampling.py's loop with the posterior of ConjugateGradients in place of the
sparse one.  The function samples come from pathwise conditioning with the CG solve (svgp_cg_sampler_*): S draws cost one batched solve
with S right-hand sides, after which every evaluation - here the steps of a gradient ascent - is one data-sized pass over the N rows.

  * N = 4000 noisy observations of the objective of example l, the exact GP with an SE kernel (no inducing points);
  * 8 functions from its posterior, 48 starts per function on [-1, 1], climbed by ascent on fs.value_and_grad;
  * each function's maximiser, checked against that function's maximum on a dense grid of fs(x).

    python examples/o_exact_gp_thompson.py      # needs an MI355X
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402


def main(N=4000, n_functions=8, n_starts=48, n_features=2048, n_steps=300, n_grid=20_001, seed=7):
    rng = np.random.default_rng(seed)
    noise, var, ell = 0.3, 1.3, 0.12
    x = rng.uniform(-1, 1, N)
    y = np.sin(3 * np.pi * x) + 0.3 * np.cos(9 * np.pi * x) + 0.5 * np.sin(7 * np.pi * x) + np.sqrt(noise) * rng.standard_normal(N)
    f = ag.GP(var * ag.with_lengthscale(ag.SqExponentialKernel(), ell))
    post = ag.posterior(ag.ConjugateGradients(tol=1e-8, maxiter=2000, n_probes=0, precond_size=64), f(x, noise), y)
    fs = post.function_samples(n_functions, n_features=n_features, rng=rng)
    V, iters, rel = fs.state()
    S, K = n_functions, n_starts
    own, col = np.repeat(np.arange(S), K), np.arange(S * K)   # the function each point belongs to
    xt = np.tile(np.linspace(-1.0, 1.0, K), S)                # the starts of function s are the points s K .. (s + 1) K - 1
    step = 0.25 * ell * ell / var                             # the curvature of a sample is of order variance / lengthscale^2
    for _ in range(n_steps):
        F, G = fs.value_and_grad(xt)                          # (S K, S), (S K, S, 1): every function at every point
        xt = np.clip(xt + step * G[col, own, 0], -1.0, 1.0)
    F, G = fs.value_and_grad(xt)
    val, grd = F[col, own].reshape(S, K), G[col, own, 0].reshape(S, K)
    best = val.argmax(1)
    x_best, f_best, g_best = xt.reshape(S, K)[np.arange(S), best], val[np.arange(S), best], grd[np.arange(S), best]

    grid = np.linspace(-1, 1, n_grid)
    Fg = fs(grid)                                             # (n_grid, S): the same functions on a dense grid
    m = post.mean(grid)
    fs.free()
    post.dev.free()
    print(f"exact GP on N = {N}: {S} functions from one solve of {S} columns ({iters.max()} iterations, residual {rel.max():.1e}); "
          f"{K} starts each, {n_steps} ascent steps on {S * K} points")
    for s in range(S):
        j = int(Fg[:, s].argmax())
        gap = Fg[j, s] - f_best[s]
        print(f"function {s}: maximiser {x_best[s]:+.5f}  f = {f_best[s]:+.6f}  |f'| = {abs(g_best[s]):.1e}    "
              f"grid: {grid[j]:+.5f}  f = {Fg[j, s]:+.6f}  (grid - climbed: {gap:+.1e})")
        assert gap <= 1e-5, "the climb found a lower maximum than the dense grid"
        assert abs(x_best[s] - grid[j]) <= 2e-3, "the maximiser is not the grid's"
        assert abs(x_best[s]) >= 1.0 or abs(g_best[s]) <= 1e-2, "the gradient does not vanish at an interior maximiser"
    print(f"the proposals {np.round(np.sort(x_best), 3)} gather around the posterior mean's maximiser {grid[int(m.argmax())]:+.3f}")
    return x_best, f_best


if __name__ == "__main__":
    main()
