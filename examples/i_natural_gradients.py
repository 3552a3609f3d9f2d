#!/usr/bin/env python
"""Natural gradients for q(u), Adam for the rest - the split GPflow's NaturalGradient and GPyTorch's NGD make - on two problems:

  classification   the reference's examples/b-classification/script.jl: labels from a latent GP, Bernoulli-logistic likelihood
                   (20-point Gauss-Hermite), N = 30, M = 15, jitter 1e-3, full batch
  regression       a minibatched sparse GP regression: N = 4000 noisy points of a smooth function, M = 64, batches of 500

Each is trained twice for the same number of steps from the same start: (a) svgp_natgrad_step moves q on the device while Adam takes
the kernel parameters and z from the gradient the same call returns, the new hyperparameters going up with svgp_model_update_keep_q
(no m / Lq upload); (b) Adam on everything from svgp_elbo_grad, the way examples/a_regression.py and b_classification.py train.  The
full-data ELBO is printed after equal numbers of steps.

    python examples/i_natural_gradients.py      # needs an MI355X
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
from approxgp import _ffi  # noqa: E402


class Adam:
    def __init__(self, n, lr):
        self.m, self.v, self.t, self.lr = np.zeros(n), np.zeros(n), 0, lr

    def step(self, theta, grad):   # ascent
        self.t += 1
        self.m = 0.9 * self.m + 0.1 * grad
        self.v = 0.999 * self.v + 0.001 * grad * grad
        return theta + self.lr * (self.m / (1 - 0.9 ** self.t)) / (np.sqrt(self.v / (1 - 0.999 ** self.t)) + 1e-8)


def train(ctx, data, N, M, batch, lik, sigma2, z0, steps, natgrad, gamma=0.5, lr=0.02, seed=0):
    """-> the full-data ELBO after every `steps // 5` steps.  Hyperparameters: log variance, log precision, z (d = 1), [log sigma2]."""
    jitter = 1e-3
    gaussian = lik == _ffi.LIK_GAUSSIAN
    hyp = np.concatenate([[0.0, 0.0], z0, [np.log(sigma2)] if gaussian else []])
    m, A = np.zeros(M), np.eye(M)

    def desc(h, m, A):
        return _ffi.make_desc(np.float64, _ffi.KERNEL_SE, np.exp(h[0]), [np.exp(h[1])], h[2:2 + M], m, A, jitter, likelihood=lik,
                              lik_sigma2=float(np.exp(h[-1])) if gaussian else 1.0)

    def hyp_grad(h, g):
        head = [g["variance"] * np.exp(h[0]), g["inv_lengthscale"][0] * np.exp(h[1])]
        return np.concatenate([head, np.asarray(g["z"]), [g["lik_sigma2"] * np.exp(h[-1])] if gaussian else []])

    model = _ffi.DeviceModel(ctx, *desc(hyp, m, A))
    rng = np.random.default_rng(seed)
    opt_h, opt_q = Adam(hyp.size, lr), Adam(M + M * M, lr)
    trace = []
    for it in range(steps):
        off = 0 if batch == N else int(rng.integers(0, N - batch + 1))
        if natgrad:
            _, _, g, _, _ = model.natgrad_step(data, off, batch, float(N), gamma=gamma, want_grads=True, fetch=False, z_shape=(M,))
            hyp = opt_h.step(hyp, hyp_grad(hyp, g))
            model.update_keep_q(*desc(hyp, m, A))         # m, A are ignored: q stays on the device
        else:
            _, _, g = model.elbo_grad(data, off, batch, float(N), z_shape=(M,))
            hyp = opt_h.step(hyp, hyp_grad(hyp, g))
            q = opt_q.step(np.concatenate([m, A.ravel()]), np.concatenate([np.asarray(g["m"]), np.tril(np.asarray(g["Lq"])).ravel()]))
            m, A = q[:M], np.tril(q[M:].reshape(M, M))
            model.update(*desc(hyp, m, A))
        if (it + 1) % max(1, steps // 5) == 0:
            trace.append(model.elbo(data, 0, N, float(N))[0])
    model.free()
    return trace


def main(seed=1):
    rng = np.random.default_rng(seed)
    ctx = _ffi.default_context()
    # ---- the reference's Bernoulli example (script.jl:57-86) ----
    x_true = np.arange(0.0, 6.0 + 1e-9, 0.02)
    k_true = lambda a, b: 10.0 * np.exp(-0.5 * (0.9 * (a[:, None] - b[None, :])) ** 2)
    f_true = np.linalg.cholesky(k_true(x_true, x_true) + 1e-6 * np.eye(x_true.size)) @ rng.standard_normal(x_true.size)
    y_true = (rng.random(x_true.size) < 1.0 / (1.0 + np.exp(-f_true))).astype(np.float64)
    N, M = 30, 15
    mask = np.sort(rng.choice(x_true.size, N, replace=False))
    data = _ffi.DeviceData(ctx, x_true[mask], y_true[mask], np.float64)
    z0 = rng.uniform(0, 6, M)
    results = {}
    for natgrad in (True, False):
        results["classification", natgrad] = train(ctx, data, N, M, N, _ffi.LIK_BERNOULLI_LOGISTIC, 1.0, z0, 200, natgrad)
    data.free()
    # ---- minibatched regression ----
    N, M, batch = 4000, 64, 500
    x = rng.uniform(0, 6, N)
    y = np.sin(2.0 * x) + 0.5 * np.cos(5.0 * x) + 0.3 * rng.standard_normal(N)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    z0 = np.linspace(0.1, 5.9, M)
    for natgrad in (True, False):
        results["regression", natgrad] = train(ctx, data, N, M, batch, _ffi.LIK_GAUSSIAN, 0.5, z0, 200, natgrad)
    data.free()
    for prob in ("classification", "regression"):
        print(f"{prob}: full-data ELBO after 40, 80, 120, 160, 200 steps")
        print("  natural gradients on q + Adam on the rest:", " ".join(f"{v:10.3f}" for v in results[prob, True]))
        print("  Adam on everything                       :", " ".join(f"{v:10.3f}" for v in results[prob, False]))
    return results


if __name__ == "__main__":
    main()
