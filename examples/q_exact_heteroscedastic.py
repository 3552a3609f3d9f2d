#!/usr/bin/env python
"""Heteroscedastic EXACT GP regression by conjugate gradients: the setup of m_heteroscedastic_regression.py (noise that grows with x,
a noise function sigma^2(x) = floor + exp(MLP(x)) in torch trained jointly with the kernel) on the exact GP at N = 3000, with no
inducing points and nothing N x N stored.

Per step the noise vector s = exp(MLP(x)) goes to the handle as it is (svgp_cg_set_noise reads the torch tensor and keeps a snapshot),
svgp_cg_lml_grad_noise returns the log marginal likelihood's estimate, its gradient in the kernel's hyperparameters and
s_bar = d lml / d sigma_i^2 into a torch tensor on the device, and `s.backward(-s_bar)` pulls it back through the MLP.  The estimator is
unbiased for the gradient but is not the derivative of the estimated value, so every step draws new probes.  The comparison is the
homoscedastic exact GP (one learned sigma^2) on the held-out mean negative log predictive density.

    python examples/q_exact_heteroscedastic.py      # needs an MI355X
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
from approxgp import DeviceConjugateGradients, _ffi, draw_probes  # noqa: E402
from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel  # noqa: E402

FLOOR, PROBES, TOL = 1e-4, 16, 1e-6


class Adam:
    def __init__(self, x, lr):
        self.x, self.lr, self.m, self.v, self.t = np.array(x, dtype=np.float64), lr, 0.0, 0.0, 0

    def step(self, grad):   # ascent
        self.t += 1
        self.m = 0.9 * self.m + 0.1 * grad
        self.v = 0.999 * self.v + 0.001 * grad**2
        self.x = self.x + self.lr * (self.m / (1 - 0.9**self.t)) / (np.sqrt(self.v / (1 - 0.999**self.t)) + 1e-8)


def nlpd(mu, v, y, sig2):
    tot = v + sig2
    return float(np.mean(0.5 * np.log(2 * np.pi * tot) + (y - mu) ** 2 / (2 * tot)))


def train(ctx, x, y, x_test, y_test, heteroscedastic, steps, seed=0):
    torch.manual_seed(seed)
    n = x.shape[0]
    theta = Adam([0.0, np.log(0.3), np.log(0.1)], 0.05)          # log variance, log lengthscale, log sigma^2 (homoscedastic only)
    xt = torch.tensor(np.concatenate([x, x_test])[:, None], dtype=torch.float64, device="cuda")
    mlp = torch.nn.Sequential(torch.nn.Linear(1, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1)).double().cuda()
    with torch.no_grad():
        mlp[2].bias.fill_(np.log(0.1))
    opt = torch.optim.Adam(mlp.parameters(), lr=0.02)
    s_bar = torch.zeros(n, dtype=torch.float64, device="cuda")
    dev = DeviceConjugateGradients(ctx, x, y, np.float64)

    def desc():
        var, ell, s2 = np.exp(theta.x[0]), np.exp(theta.x[1]), (FLOOR if heteroscedastic else np.exp(theta.x[2]))
        kernel = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.array([1.0 / ell]))), var)
        return dev.desc(kernel, s2, tol=TOL, maxiter=1000), (var, ell, s2)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(steps):
            (d, keep), (var, ell, s2) = desc()
            z = draw_probes(n, PROBES, step)                          # new probes each step
            if heteroscedastic:
                s = torch.exp(mlp(xt[:n]).squeeze(1))
                torch.cuda.synchronize()                              # (the library reads s on its own stream)
                dev.set_noise(s.detach().contiguous())
                lml, g, info = dev.lml_grad(d, z, wrt_noise=True, noise_grad_out=s_bar)
                opt.zero_grad()
                s.backward(-s_bar / n)                                # ascent on the lml per point
                opt.step()
                gs2 = 0.0
            else:
                lml, g, info = dev.lml_grad(d, z)
                gs2 = g["diag"] * s2
            theta.step(np.array([g["variance"] * var, g["inv_lengthscale"][0] * (-1.0 / ell), gs2]) / n)
        (d, keep), (var, ell, s2) = desc()
        with torch.no_grad():
            s_all = torch.exp(mlp(xt).squeeze(1)).contiguous() if heteroscedastic else None
        torch.cuda.synchronize()
        if heteroscedastic:
            dev.set_noise(s_all[:n].contiguous())
        lml, info = dev.fit(d, draw_probes(n, PROBES, steps))
        mu, v, _ = dev.predict(x_test)
    sig2 = s2 + (s_all[n:].cpu().numpy() if heteroscedastic else 0.0)
    dev.free()
    return lml / n, nlpd(mu, v, y_test, sig2)


def main(steps=150, n_train=3000, n_test=1000):
    rng = np.random.default_rng(1234)
    n = n_train + n_test
    x = rng.uniform(0.0, 1.0, n)
    sd = 0.05 + 0.6 * x**2                                        # the noise grows with x
    y = np.sin(4 * np.pi * x) + sd * rng.standard_normal(n)
    ctx = _ffi.Context(0)
    res = {}
    for het in (False, True):
        b, q = train(ctx, x[:n_train], y[:n_train], x[n_train:], y[n_train:], het, steps)
        res[het] = q
        print(f"{'heteroscedastic (sigma^2(x) = exp(MLP(x)))' if het else 'homoscedastic exact GP (one sigma^2)     '}: "
              f"{steps} steps, lml per point {b:.4f}, held-out mean NLPD {q:.4f}")
    print(f"true-noise NLPD floor {float(np.mean(0.5 * np.log(2 * np.pi * sd[n_train:] ** 2) + 0.5)):.4f}")
    ctx.close()
    return res


if __name__ == "__main__":
    main()
