#!/usr/bin/env python
"""Noisy regression with the NearestNeighbors (Vecchia) approximation through the MI355X library: N = 50 000 points in d = 2,
k = 32 neighbours.  Every point is conditioned on its 32 nearest predecessors (neighbors="nearest": the search runs on the device,
with the kernel's inverse lengthscales as the metric, once per evaluation of the objective); the points are still ordered along a
Morton (Z-order) curve, which keeps the gathers local.  The reference's rule - the 32 points before a point in that order - is
printed beside it.  Variance, lengthscale and noise are trained with L-BFGS on the device's -approx_lml and its gradient (svgp_nn_lml_grad; log
parametrisation, chained here by hand), then the posterior is fitted once and predicts on a grid.  The noise enters as the
diagonal term (NearestNeighbors(k, include_noise=True)): the objective is the Vecchia approximation of logpdf(fx, y).

    python examples/g_nearest_neighbors.py [N]     # needs an MI355X
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402

K = 32


def morton_order(x, bits=16):
    """argsort of the interleaved bits of the two coordinates, each quantised to `bits` bits"""
    lo, hi = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    q = ((x - lo) / (hi - lo) * (2 ** bits - 1)).astype(np.uint64)
    code = np.zeros(x.shape[1], dtype=np.uint64)
    for b in range(bits):
        code |= ((q[0] >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b)
        code |= ((q[1] >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b + 1)
    return np.argsort(code, kind="stable")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000   # the search is brute force: N^2 / 2 distances
    rng = np.random.default_rng(0)
    x = rng.uniform(-3.0, 3.0, size=(2, n))
    truth = lambda p: np.sin(2.0 * p[0]) * np.cos(1.5 * p[1])
    y = truth(x) + 0.2 * rng.standard_normal(n)
    order = morton_order(x)
    x, y = x[:, order], y[order]

    dev = ag.DeviceNearestNeighbors(ag.default_context(), x, y, np.float64)

    def value_and_grad(theta):   # theta = log (variance, lengthscale, noise)
        variance, lengthscale, noise = np.exp(theta)
        desc, keep = dev.desc(variance * ag.with_lengthscale(ag.SqExponentialKernel(), lengthscale), K, diag=noise)
        lml, dv, dil, dd, _ = dev.lml_grad(desc)   # at the fixed table: an isotropic metric selects the same sets at every lengthscale
        # the kernel's parameter is 1 / lengthscale: d / d log l = sum(d / d invl) * (-1 / l)
        return -lml / n, -np.array([dv * variance, float(np.sum(dil)) * (-1.0 / lengthscale), dd * noise]) / n

    dev.build_neighbors(K)   # unit metric
    res = minimize(value_and_grad, np.log([1.0, 1.0, 0.1]), jac=True, method="L-BFGS-B")
    variance, lengthscale, noise = np.exp(res.x)
    print(f"{res.nfev} evaluations: variance {variance:.4f} lengthscale {lengthscale:.4f} noise sd {np.sqrt(noise):.4f} "
          f"(data: 0.2)  -approx_lml / N = {res.fun:.6f}")
    desc, keep = dev.desc(variance * ag.with_lengthscale(ag.SqExponentialKernel(), lengthscale), K, diag=noise)
    near = dev.lml(desc)[0]
    dev.clear_neighbors()
    print(f"approx_lml / N at these parameters: {near / n:.6f} (32 nearest predecessors)  {dev.lml(desc)[0] / n:.6f} (window of the previous 32)")
    dev.free()

    f = ag.GP(variance * ag.with_lengthscale(ag.SqExponentialKernel(), lengthscale))
    g = np.linspace(-3.0, 3.0, 40)
    grid = np.stack([a.ravel() for a in np.meshgrid(g, g)])
    for name, neighbors in (("nearest", "nearest"), ("window", None)):
        post = ag.posterior(ag.NearestNeighbors(K, include_noise=True, neighbors=neighbors), f(x, noise), y)
        mean, var = post.mean_and_var(grid)
        print(f"{name}: grid of {grid.shape[1]} points: rmse against the noise-free function {np.sqrt(np.mean((mean - truth(grid)) ** 2)):.4f}, "
              f"mean latent sd {np.mean(np.sqrt(np.maximum(var, 0.0))):.4f}")
        if neighbors == "nearest":
            # the same model predicted locally: every grid point conditioned on its K nearest observed points (svgp_nn_predict_local),
            # N distances and one K x K block per grid point in place of N kernel evaluations through the global U
            lmean, lvar = post.local_mean_and_var(grid)
            print(f"local:   grid of {grid.shape[1]} points: rmse against the noise-free function {np.sqrt(np.mean((lmean - truth(grid)) ** 2)):.4f}, "
                  f"mean latent sd {np.mean(np.sqrt(np.maximum(lvar, 0.0))):.4f}")
        post.dev.free()


if __name__ == "__main__":
    main()
