#!/usr/bin/env python
"""Heteroscedastic sparse GP regression through the collapsed bound: data whose noise grows with x, a noise function
sigma^2(x) = floor + exp(MLP(x)) in torch trained jointly with the kernel, no variational parameters anywhere.

Per step the noise vector s = exp(MLP(x)) goes to the device as it is (a torch tensor), svgp_collapsed_grad_with_noise returns the bound,
its gradient in the kernel's hyperparameters and s_bar = d bound / d sigma_j^2 into a torch tensor on the device, and
`s.backward(-s_bar)` pulls it back through the MLP.  The comparison is homoscedastic VFE (one learned sigma^2) on the held-out mean
negative log predictive density.

    python examples/m_heteroscedastic_regression.py      # needs an MI355X
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
from approxgp import _ffi  # noqa: E402

FLOOR, JITTER = 1e-4, 1e-6


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


def train(ctx, data, x, n_train, n_test, y_test, heteroscedastic, steps, seed=0):
    torch.manual_seed(seed)
    M = 30
    z = np.linspace(x.min(), x.max(), M)
    theta = Adam([0.0, np.log(0.3), np.log(0.1)], 0.05)          # log variance, log lengthscale, log sigma^2 (homoscedastic only)
    xt = torch.tensor(x[:, None], dtype=torch.float64, device="cuda")
    mlp = torch.nn.Sequential(torch.nn.Linear(1, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1)).double().cuda()
    with torch.no_grad():
        mlp[2].bias.fill_(np.log(0.1))
    opt = torch.optim.Adam(mlp.parameters(), lr=0.02)
    s_bar = torch.zeros(n_train, dtype=torch.float64, device="cuda")

    def desc():
        var, ell, s2 = np.exp(theta.x[0]), np.exp(theta.x[1]), (FLOOR if heteroscedastic else np.exp(theta.x[2]))
        return _ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, [1.0 / ell], z, np.zeros(M), np.eye(M), JITTER, lik_sigma2=s2), (var, ell, s2)

    model = _ffi.DeviceModel(ctx, *desc()[0])
    for _ in range(steps):
        (d, keep), (var, ell, s2) = desc()
        model.update(d, keep)
        if heteroscedastic:
            s = torch.exp(mlp(xt[:n_train]).squeeze(1))
            torch.cuda.synchronize()                              # (the library reads s on its own stream)
            bound, _, g = model.collapsed_grad(data, 0, n_train, z_shape=(M,), noise=s.detach().contiguous(), want_noise_grad=s_bar)
            opt.zero_grad()
            s.backward(-s_bar / n_train)                          # ascent on the bound per point
            opt.step()
            gs2 = 0.0
        else:
            bound, _, g = model.collapsed_grad(data, 0, n_train, z_shape=(M,))
            gs2 = g["lik_sigma2"] * s2
        theta.step(np.array([g["variance"] * var, g["inv_lengthscale"][0] * (-1.0 / ell), gs2]) / n_train)
    (d, keep), (var, ell, s2) = desc()
    model.update(d, keep)
    with torch.no_grad():
        s_all = torch.exp(mlp(xt).squeeze(1)).contiguous() if heteroscedastic else None
    torch.cuda.synchronize()
    bound, _, _ = model.collapsed_q(data, 0, n_train, fetch=False, noise=s_all[:n_train].contiguous() if heteroscedastic else None)
    mu, v = model.marginals(data, n_train, n_test)
    sig2 = s2 + (s_all[n_train:].cpu().numpy() if heteroscedastic else 0.0)
    model.free()
    return bound / n_train, nlpd(mu, v, y_test, sig2)


def main(steps=300):
    rng = np.random.default_rng(1234)
    n_train, n_test = 4000, 2000
    n = n_train + n_test
    x = rng.uniform(0.0, 1.0, n)
    sd = 0.05 + 0.6 * x**2                                        # the noise grows with x
    y = np.sin(4 * np.pi * x) + sd * rng.standard_normal(n)
    ctx = _ffi.Context(0)
    data = _ffi.DeviceData(ctx, x, y, np.float64)                 # train = [0, n_train), test = [n_train, n): windows of one upload
    res = {}
    for het in (False, True):
        b, q = train(ctx, data, x, n_train, n_test, y[n_train:], het, steps)
        res[het] = q
        print(f"{'heteroscedastic (sigma^2(x) = exp(MLP(x)))' if het else 'homoscedastic VFE (one sigma^2)          '}: "
              f"{steps} steps, bound per point {b:.4f}, held-out mean NLPD {q:.4f}")
    print(f"true-noise NLPD floor {float(np.mean(0.5 * np.log(2 * np.pi * sd[n_train:] ** 2) + 0.5)):.4f}")
    data.free()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
