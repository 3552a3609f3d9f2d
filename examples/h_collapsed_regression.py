#!/usr/bin/env python
"""The regression problem of examples/a_regression.py without a q(u) to learn: for a Gaussian likelihood the optimal q(u) has a closed
form (Titsias 2009), so only the kernel's variance and lengthscale and the M = 20 inducing inputs are optimised - by Adam on the
gradient of the collapsed bound over all N = 10 000 points, which svgp_collapsed_grad returns from one data pass plus the existing
value-and-gradient at the optimal q.  Prints the final bound next to the full-data ELBO the SVGP example reaches.

    python examples/h_collapsed_regression.py          # needs an MI355X
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approxgp as ag  # noqa: E402
from approxgp import _ffi  # noqa: E402


def softplus(v):
    return np.log1p(np.exp(-abs(v))) + max(v, 0.0)


def invsoftplus(v):
    return v + np.log(-np.expm1(-v))


def main(steps=200, lr=0.02, seed=1234, compare=True):
    rng = np.random.default_rng(seed)
    N, M = 10_000, 20
    x = rng.uniform(-1, 1, N)
    y = np.sin(3 * np.pi * x) + 0.3 * np.cos(9 * np.pi * x) + 0.5 * np.sin(7 * np.pi * x) + 0.3 * rng.standard_normal(N)
    lik_noise, jitter = 0.3, 1e-5
    theta = {"k": np.array([invsoftplus(1.3), invsoftplus(0.3)]), "z": x[:M].copy()}
    ctx = _ffi.default_context()
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    adam = {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in theta.items()}

    def desc():
        var, ell = softplus(theta["k"][0]), softplus(theta["k"][1])
        return _ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, [1.0 / ell], theta["z"], np.zeros(M), np.eye(M), jitter,
                              likelihood=_ffi.LIK_GAUSSIAN, lik_sigma2=lik_noise), var, ell

    (d0, keep), _, _ = desc()
    model = _ffi.DeviceModel(ctx, d0, keep)
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))                # d softplus / dt
    for step in range(1, steps + 1):
        (d, keep), var, ell = desc()
        model.update(d, keep)
        val, _, g = model.collapsed_grad(data, 0, N, z_shape=(M,))
        grads = {"k": -np.array([g["variance"] * sig(theta["k"][0]), g["inv_lengthscale"][0] * (-1.0 / ell**2) * sig(theta["k"][1])]),
                 "z": -np.asarray(g["z"])}
        for k in theta:
            m1, m2 = adam[k]
            m1[...] = 0.9 * m1 + 0.1 * grads[k]
            m2[...] = 0.999 * m2 + 0.001 * grads[k] ** 2
            theta[k] = theta[k] - lr * (m1 / (1 - 0.9**step)) / (np.sqrt(m2 / (1 - 0.999**step)) + 1e-8)
        if step % 50 == 0 or step == 1:
            print(f"step {step:4d}  collapsed bound {val:12.3f}")
    (d, keep), var, ell = desc()
    model.update(d, keep)
    bound, m, Lq = model.collapsed_q(data, 0, N)            # the model now carries the optimal q
    elbo_at_q, _ = model.elbo(data, 0, N, float(N))
    print(f"final: variance {var:.3f}, lengthscale {ell:.3f}, collapsed bound {bound:.2f} (svgp_elbo at the optimal q: {elbo_at_q:.2f})")
    mu, v, _ = model.predict(np.linspace(-1, 1, 5))
    print("posterior mean at -1, -0.5, 0, 0.5, 1:", np.round(mu, 3), " var:", np.round(v, 4))
    model.free()
    data.free()
    if compare:
        import a_regression
        full = a_regression.main()
        print(f"collapsed bound {bound:.2f}  vs  SVGP full-data ELBO after its 300 minibatch Adam steps {full:.2f}")
    return bound


if __name__ == "__main__":
    main()
