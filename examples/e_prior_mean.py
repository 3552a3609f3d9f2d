#!/usr/bin/env python
"""A learned prior mean: GP(CustomMean(mlp), k) trained through svgp_elbo_grad_with_mean.

The data carry a strong linear drift plus a periodic term (y = 0.3 x + sin(x) + noise), observed on x in [0, 80].  A small torch
network as the prior mean (a linear term plus a tanh MLP) takes the drift.  The SE kernel is held at unit variance and a unit
lengthscale, short enough for the sine with M = 64 inducing points: under that prior a constant-mean SVGP has to carry a drift of
+-12 through q(u) alone, and a few lengthscales past the last point its posterior mean falls back to the constant.  The two models are
compared on a held-out grid inside the data and on x in [80, 100], beyond it.  Measured on an MI355X (1000 Adam steps each):

                        final ELBO    RMSE inside [0.5, 79.5]    RMSE beyond [80, 100]
    ConstMean           -112 734      4.67                       22.6
    learned mean          -7 185      0.157                       6.11

The mean's values stay on the device: the network's output at the data is handed to the library as device-memory offsets, and one
value-and-gradient call writes d elbo / d mean(x) straight into a torch tensor on the same stream (svgp_elbo_grad_with_mean, on_device = 1).
NonCentered parametrisation: the mean at the inducing points has no effect there (alpha = Lk' \ m), so only mean(x) is passed:

    mux = net(x).reshape(-1)                                                  # mean(f.prior, x)
    elbo, _, g = model.elbo_grad(data, 0, N, N, prior_mean=mux.detach(), mean_grad=gbar)
    mux.backward(-gbar)                                                       # d(-elbo)/d mux = -mux_bar

The same SVGP with a ConstMean (trained constant) is the comparison.  Both print their final ELBO and the RMSE of the posterior mean on the two
held-out grids.

    python examples/e_prior_mean.py      # needs an MI355X
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
from approxgp import _ffi  # noqa: E402

M = 64


def truth(x):
    return 0.3 * x + np.sin(x)


def train(x, y, xt, yt, learned_mean, steps, seed=0):
    N = x.shape[0]
    torch.manual_seed(seed)
    lin = torch.nn.Linear(1, 1).to("cuda", torch.float64)
    mlp = torch.nn.Sequential(torch.nn.Linear(1, 32), torch.nn.Tanh(), torch.nn.Linear(32, 1)).to("cuda", torch.float64)
    net = lambda t: lin(t) + mlp(t)
    ctx = _ffi.Context(0, torch.cuda.current_stream().cuda_stream)   # the library's work is ordered with torch's on one stream
    sv = {"logvar": torch.zeros(1, dtype=torch.float64), "logil": torch.tensor([np.log(1.0)], dtype=torch.float64),
          "z": torch.tensor(np.linspace(0.0, 80.0, M)), "m": torch.zeros(M, dtype=torch.float64),
          "Aoff": torch.zeros((M, M), dtype=torch.float64), "logdiag": torch.zeros(M, dtype=torch.float64),
          "logs2": torch.tensor([np.log(0.1)], dtype=torch.float64), "c": torch.zeros(1, dtype=torch.float64)}
    for p in sv.values():
        p.requires_grad_(True)
    # the kernel is held at unit variance and unit lengthscale - short enough for the sine with 64 inducing points over the data's
    # range; everything else (z, q(u), the noise, the constant) is trained
    groups = [{"params": [p for k, p in sv.items() if k not in ("logvar", "logil")], "lr": 0.02}]
    groups += [{"params": list(lin.parameters()), "lr": 0.05}, {"params": list(mlp.parameters()), "lr": 0.005}] if learned_mean else []
    opt = torch.optim.Adam(groups)
    xs = lambda a: torch.as_tensor(a, device="cuda").reshape(-1, 1) / 50.0 - 1.0   # the MLP sees inputs scaled to [-1, 1]

    def desc():   # NonCentered: q(u) = N(m, A A') over the whitened inducing values
        var, il, s2 = float(sv["logvar"].detach().exp()), sv["logil"].detach().exp().numpy(), float(sv["logs2"].detach().exp())
        A = np.tril(sv["Aoff"].detach().numpy(), -1) + np.diag(sv["logdiag"].exp().detach().numpy())
        return _ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, il, sv["z"].detach().numpy(), sv["m"].detach().numpy(), A, 1e-5,
                              lik_sigma2=s2, mean_const=float(sv["c"].detach()))

    model = _ffi.DeviceModel(ctx, *desc())
    x_d, y_d = torch.tensor(x, device="cuda").reshape(1, -1).contiguous(), torch.tensor(y, device="cuda")
    data = _ffi.DeviceData.wrap(ctx, np.float64, 1, N, N, x_d.data_ptr(), y_d.data_ptr())
    gbar = torch.empty(N, dtype=torch.float64, device="cuda")
    t0 = time.perf_counter()
    val = None
    for it in range(1, steps + 1):
        opt.zero_grad()
        model.update(*desc())
        if learned_mean:
            mux = net(xs(x_d)).reshape(-1)
            val, _, g = model.elbo_grad(data, 0, N, float(N), prior_mean=mux.detach().contiguous(), mean_grad=gbar)
            mux.backward(-gbar)   # d(-elbo)/d mux = -mux_bar, on the device
        else:
            val, _, g = model.elbo_grad(data, 0, N, float(N))
        var, il, s2 = float(sv["logvar"].detach().exp()), sv["logil"].detach().exp(), float(sv["logs2"].detach().exp())
        sv["logvar"].grad = torch.tensor([-g["variance"] * var], dtype=torch.float64)
        sv["logil"].grad = -torch.tensor(g["inv_lengthscale"]) * il
        sv["z"].grad = -torch.tensor(np.asarray(g["z"])).reshape(-1)
        sv["m"].grad = -torch.tensor(g["m"])
        sv["Aoff"].grad = -torch.tensor(np.tril(g["Lq"], -1))
        sv["logdiag"].grad = -torch.tensor(np.diag(g["Lq"]).copy()) * sv["logdiag"].exp().detach()
        sv["logs2"].grad = torch.tensor([-g["lik_sigma2"] * s2], dtype=torch.float64)
        sv["c"].grad = torch.tensor([-g["mean_const"]], dtype=torch.float64)
        opt.step()
        if it == 1 or it % 200 == 0:
            print(f"  step {it:4d}  ELBO {val:12.2f}")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"  {steps} steps in {dt:.2f} s ({dt / steps * 1e3:.1f} ms per step)")
    # held-out RMSE of the posterior mean: svgp_predict gives mean_const + K*u alpha, the caller adds its mean at x*
    model.update(*desc())
    rmse = []
    for xg, yg in zip(xt, yt):
        off = net(xs(xg)).reshape(-1).detach().cpu().numpy() if learned_mean else 0.0
        pred = model.predict(xg, True, False, False)[0] + off
        rmse.append(float(np.sqrt(np.mean((pred - yg) ** 2))))
    data.free()
    model.free()
    ctx.close()
    return val, rmse


def main(steps=1000):
    rng = np.random.default_rng(2)
    N = 20_000
    x = np.sort(rng.uniform(0.0, 80.0, N))
    y = truth(x) + 0.1 * rng.standard_normal(N)
    xt = (np.linspace(0.5, 79.5, 2000), np.linspace(80.0, 100.0, 500))   # inside the data, beyond it
    yt = tuple(truth(a) for a in xt)
    print("SVGP with a ConstMean (trained constant):")
    c_elbo, c_rmse = train(x, y, xt, yt, False, steps)
    print("SVGP with a learned mean (linear + MLP) through svgp_elbo_grad_with_mean:")
    l_elbo, l_rmse = train(x, y, xt, yt, True, steps)
    print(f"final ELBO: ConstMean {c_elbo:.2f}, learned mean {l_elbo:.2f}")
    print(f"test RMSE inside the data  [0.5, 79.5]: ConstMean {c_rmse[0]:.4f}, learned mean {l_rmse[0]:.4f}")
    print(f"test RMSE beyond the data  [80, 100]:   ConstMean {c_rmse[1]:.4f}, learned mean {l_rmse[1]:.4f}")


if __name__ == "__main__":
    main()
