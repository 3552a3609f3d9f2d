#!/usr/bin/env python
"""Upper-confidence-bound acquisition on a fitted SVGP, climbed with the device gradient of the predictive distribution
(svgp_predictor_eval).  UCB(x) = mu(x) + kappa sqrt(v(x)) and d UCB / dx = d mu / dx + kappa d v / dx / (2 sqrt(v)): one call per step
returns mu, v and both gradients for every start.

  * the model of examples/l_thompson_sampling.py (SE kernel, M = 20, the optimal q(u) of its training data);
  * 64 starts on [-1, 1], climbed by gradient ascent with the gradient of this call;
  * beside it the same ascent on central differences of svgp_marginals (2 d more data passes per step), and the maximum of UCB on a
    dense grid of marginals(x) to check both against.

    python examples/s_ucb_acquisition.py      # needs an MI355X
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402
from approxgp import _ffi  # noqa: E402


def main(n_starts=64, n_steps=300, kappa=2.0, n_grid=20_001, seed=7):
    rng = np.random.default_rng(seed)
    N, M, noise, jitter = 2_000, 20, 0.3, 1e-5
    x = rng.uniform(-1, 1, N) * np.abs(rng.uniform(-1, 1, N))   # denser near 0: the variance matters at the edges
    y = np.sin(3 * np.pi * x) + 0.3 * np.cos(9 * np.pi * x) + np.sqrt(noise) * rng.standard_normal(N)
    var, ell = 1.3, 0.12
    z = np.linspace(-1, 1, M)
    ctx = _ffi.Context(0)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    model = _ffi.DeviceModel(ctx, *_ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, [1.0 / ell], z, np.zeros(M), np.eye(M), jitter,
                                                  lik_sigma2=noise))
    model.collapsed_q(data)
    data.free()
    pred = model.predictor()   # a snapshot of the fitted model

    def ucb_and_grad(xs):
        pts = _ffi.DeviceData(ctx, xs, None, np.float64)
        try:
            mu, v, dmu, dv = pred.eval(pts)
        finally:
            pts.free()
        s = np.sqrt(v)
        return mu + kappa * s, dmu[0] + kappa * dv[0] / (2 * s)

    def ucb_marginals(xs):
        pts = _ffi.DeviceData(ctx, xs, None, np.float64)
        try:
            mu, v = model.marginals(pts)
        finally:
            pts.free()
        return mu + kappa * np.sqrt(v)

    step, h = 0.1 * ell * ell / var, 1e-4
    xa = np.linspace(-1.0, 1.0, n_starts)
    xf = xa.copy()
    for _ in range(n_steps):
        xa = np.clip(xa + step * ucb_and_grad(xa)[1], -1.0, 1.0)
        xf = np.clip(xf + step * (ucb_marginals(xf + h) - ucb_marginals(xf - h)) / (2 * h), -1.0, 1.0)
    grid = np.linspace(-1.0, 1.0, n_grid)
    best = ucb_marginals(grid).max()
    ua, uf = ucb_and_grad(xa)[0], ucb_marginals(xf)
    print(f"max UCB on a grid of {n_grid}: {best:.6f}")
    print(f"ascent with svgp_predictor_eval:        best {ua.max():.6f} at x = {xa[ua.argmax()]:+.5f}  ({n_steps} data passes)")
    print(f"ascent with differences of marginals:   best {uf.max():.6f} at x = {xf[uf.argmax()]:+.5f}  ({2 * n_steps} data passes)")
    print(f"largest distance between the two ascents' end points: {np.abs(xa - xf).max():.2e}")
    assert ua.max() >= best - 1e-6 * abs(best)
    pred.free()
    model.free()
    ctx.close()


if __name__ == "__main__":
    main()
