#!/usr/bin/env python
"""Deep kernel learning: a torch network in front of the SVGP, trained through d elbo / d x.

A two-layer MLP on the GPU maps raw 16-d inputs to d = 4 features; the features stay on the device, wrapped without a copy
(svgp_data_wrap_device), and one value-and-gradient call writes d elbo / d x straight into a torch tensor on the same stream
(svgp_elbo_grad_inputs, on_device = 1).  Autograd takes it from there:

    feats = net(raw).T.contiguous()                                   # (d, N) on the GPU: feature-major, what the library reads
    data = DeviceData.wrap(ctx, float64, d, N, N, feats.data_ptr(), y.data_ptr())
    elbo, _, g = model.elbo_grad(data, 0, N, N, inputs=(gx.data_ptr(), N))
    feats.backward(-gx)                                               # the network's gradient of -ELBO

One Adam optimiser holds the network (learning rate 0.005) and the SVGP parameters (0.02: log variance, log inverse
lengthscales, z, m, the factor of cov(q), log sigma^2).
N = 20 000, M = 64, Gaussian likelihood.  The same SVGP trained on the untrained network's FIXED features is the comparison.

    python examples/d_input_gradients.py      # needs an MI355X
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
from approxgp import _ffi  # noqa: E402


def train(raw, y, train_net, steps, seed=0):
    N, M, d = raw.shape[0], 64, 4
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(), torch.nn.Linear(32, d)).to("cuda", torch.float64)
    for p in net.parameters():
        p.requires_grad_(train_net)
    ctx = _ffi.Context(0, torch.cuda.current_stream().cuda_stream)   # the library's work is ordered with torch's on one stream
    with torch.no_grad():
        f0 = net(raw)
    rng = np.random.default_rng(seed)
    sv = {"logvar": torch.zeros(1, dtype=torch.float64), "logil": torch.zeros(d, dtype=torch.float64),
          "z": torch.tensor(f0[rng.choice(N, M, replace=False)].T.cpu().numpy()), "m": torch.zeros(M, dtype=torch.float64),
          "Aoff": torch.zeros((M, M), dtype=torch.float64), "logdiag": torch.zeros(M, dtype=torch.float64), "logs2": torch.tensor([np.log(0.1)], dtype=torch.float64)}
    for p in sv.values():
        p.requires_grad_(True)
    groups = [{"params": list(sv.values()), "lr": 0.02}] + ([{"params": list(net.parameters()), "lr": 0.005}] if train_net else [])
    opt = torch.optim.Adam(groups)

    def desc():   # the factor of cov(q): strictly lower part as it is, diagonal through exp (it stays positive)
        var, il, s2 = float(sv["logvar"].detach().exp()), sv["logil"].detach().exp().numpy(), float(sv["logs2"].detach().exp())
        A = np.tril(sv["Aoff"].detach().numpy(), -1) + np.diag(sv["logdiag"].exp().detach().numpy())
        return _ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, il, sv["z"].detach().numpy(), sv["m"].detach().numpy(), A, 1e-5,
                              lik_sigma2=s2)

    model = _ffi.DeviceModel(ctx, *desc())
    gx = torch.empty((d, N), dtype=torch.float64, device="cuda")
    t0 = time.perf_counter()
    first = last = None
    for it in range(1, steps + 1):
        opt.zero_grad()
        model.update(*desc())
        feats = net(raw).T.contiguous()
        data = _ffi.DeviceData.wrap(ctx, np.float64, d, N, N, feats.data_ptr(), y.data_ptr())
        val, _, g = model.elbo_grad(data, 0, N, float(N), inputs=(gx.data_ptr(), N) if train_net else None)
        data.free()
        if train_net:
            feats.backward(-gx)
        var, il, s2 = float(sv["logvar"].detach().exp()), sv["logil"].detach().exp(), float(sv["logs2"].detach().exp())
        sv["logvar"].grad = torch.tensor([-g["variance"] * var], dtype=torch.float64)
        sv["logil"].grad = -torch.tensor(g["inv_lengthscale"]) * il
        sv["z"].grad = -torch.tensor(np.asarray(g["z"]))
        sv["m"].grad = -torch.tensor(g["m"])
        sv["Aoff"].grad = -torch.tensor(np.tril(g["Lq"], -1))
        sv["logdiag"].grad = -torch.tensor(np.diag(g["Lq"]).copy()) * sv["logdiag"].exp().detach()
        sv["logs2"].grad = torch.tensor([-g["lik_sigma2"] * s2], dtype=torch.float64)
        opt.step()
        first = val if first is None else first
        last = val
        if it == 1 or it % 100 == 0:
            print(f"  step {it:4d}  ELBO {val:12.2f}")
    dt = time.perf_counter() - t0
    print(f"  {steps} steps in {dt:.2f} s ({dt / steps * 1e3:.1f} ms per step)")
    model.free()
    ctx.close()
    return first, last


def main(steps=400):
    rng = np.random.default_rng(1)
    N = 20_000
    raw = rng.standard_normal((N, 16))
    w = rng.standard_normal(16)
    u = raw @ (w / np.linalg.norm(w))                                 # the signal lives on one direction of the raw inputs
    y = np.sin(2.0 * u) + 0.5 * np.tanh(u) + 0.1 * rng.standard_normal(N)
    raw_t, y_t = torch.tensor(raw, device="cuda"), torch.tensor(y, device="cuda")
    print("SVGP on the untrained network's fixed features:")
    f_first, f_last = train(raw_t, y_t, False, steps)
    print("network and SVGP trained together through d elbo / d x:")
    j_first, j_last = train(raw_t, y_t, True, steps)
    print(f"final ELBO: fixed features {f_last:.2f}, learned features {j_last:.2f} (both started at {j_first:.2f})")
    assert j_last > f_last, "the learned feature map should fit better than the fixed one"


if __name__ == "__main__":
    main()
