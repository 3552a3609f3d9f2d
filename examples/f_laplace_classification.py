#!/usr/bin/env python
"""The reference's Laplace comparison (examples/c-comparisons) through the MI355X library: the 48-point binary data set of
src/TestUtils.jl:13-37, a latent GP with softplus-parametrised variance and lengthscale (SE kernel, Bernoulli-logistic
likelihood, jitter 1e-8), theta0 = invsoftplus([1, 5]), L-BFGS on the device's -approx_lml and its gradient (the chain through
softplus done here by hand), then the posterior warm-started from the objective's last mode and its predictions on the plotting grid.

    python examples/f_laplace_classification.py      # needs an MI355X
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402

X = np.linspace(0.0, 23.5, 48)
Y = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1,
              1, 0, 0, 0, 0, 0, 0, 0], dtype=np.float64)


def softplus(t):
    return np.log1p(np.exp(-abs(t))) + max(t, 0.0)


def invsoftplus(v):
    return float(np.log(np.expm1(v)))


def build_latent_gp(theta):
    variance, lengthscale = softplus(theta[0]), softplus(theta[1])
    return ag.LatentGP(ag.GP(variance * ag.with_lengthscale(ag.SqExponentialKernel(), lengthscale)), ag.BernoulliLikelihood(), 1e-8)


def main():
    objective = ag.build_laplace_objective(build_latent_gp, X, Y)   # newton_warmstart = True

    def value_and_grad(theta):
        v, g = objective.value_and_gradient(theta)
        lengthscale = softplus(theta[1])
        dsp = 1.0 / (1.0 + np.exp(-np.asarray(theta)))                 # d softplus / d t
        # variance: d/d t0; lengthscale: the kernel's parameter is 1 / lengthscale (ScaleTransform)
        return v, np.array([g["variance"] * dsp[0], float(np.sum(g["inv_lengthscale"])) * (-1.0 / lengthscale ** 2) * dsp[1]])

    theta0 = np.array([invsoftplus(1.0), invsoftplus(5.0)])
    res = minimize(value_and_grad, theta0, jac=True, method="L-BFGS-B")
    print(f"theta_opt = {res.x}  -approx_lml = {res.fun:.10g}  (Newton steps of the last call: {objective.last_info.iterations})")
    lf = build_latent_gp(res.x)
    # warm start: the Newton loop of the posterior begins at the objective's last mode
    post = ag.posterior(ag.LaplaceApproximation(f_init=objective.mode()), lf(X), Y)
    print(f"posterior Newton steps from the warm start: {post.info.iterations}")
    grid = np.linspace(-1.0, 25.0, 200)
    mean, var = post.mean_and_var(grid)
    prob = 1.0 / (1.0 + np.exp(-mean))
    print("p(y = 1) on the grid, every 20th point:", np.round(prob[::20], 3))
    print("latent sd, every 20th point:", np.round(np.sqrt(np.maximum(var, 0.0))[::20], 3))
    objective.free()


if __name__ == "__main__":
    main()
