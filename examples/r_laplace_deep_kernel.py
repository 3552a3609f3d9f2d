#!/usr/bin/env python
"""Deep kernel CLASSIFICATION with the Laplace approximation: a torch MLP maps 6-dimensional inputs to 2 features, an SE-ARD GP with a
Bernoulli-logistic likelihood sits on the features (LaplaceApproximation's device handle, svgp_laplace_*), and both are trained jointly
on approx_lml.  What makes it possible is the gradient of approx_lml with respect to the GP's INPUTS (svgp_laplace_lml_grad_inputs,
the total derivative at the Newton mode): the features stay in torch's device memory (DeviceData.wrap, no host round trip), x_bar is
written into a torch tensor, and one `features.backward(-x_bar)` carries it into the MLP.  The kernel's own parameters take their
gradients from the same call.  The labels depend on all six inputs through ONE nonlinear index, which a stationary ARD kernel on the raw
inputs cannot exploit: the same GP is trained on the raw inputs for comparison.

    python examples/r_laplace_deep_kernel.py          # needs an MI355X
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402
from approxgp import _ffi  # noqa: E402


def make_data(N, n_test, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(N + n_test, 6))
    u = np.tanh(X @ np.array([1.0, -0.8, 0.6, 0.9, -0.7, 0.5]))         # the 1-D index the labels really depend on: every input enters
    p = 1.0 / (1.0 + np.exp(-6.0 * np.sin(5.0 * u)))
    y = (rng.uniform(size=N + n_test) < p).astype(np.float64)
    return X[:N], y[:N], X[N:], y[N:]


def train(X, y, Xte, yte, deep, steps, seed=0):
    """-> (approx_lml / N at the first step, at the last, held-out accuracy).  deep: the MLP in front; otherwise the raw inputs with
    their own ARD lengthscales"""
    torch.manual_seed(seed)
    N = X.shape[0]
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y.copy()).cuda()
    d = 2 if deep else X.shape[1]
    mlp = torch.nn.Sequential(torch.nn.Linear(X.shape[1], 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                              torch.nn.Linear(32, d)).double().cuda() if deep else None
    log_var = torch.zeros((), dtype=torch.float64, requires_grad=True)
    log_il = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([log_var, log_il] + (list(mlp.parameters()) if deep else []), lr=0.01)

    ctx = _ffi.default_context()
    feats_buf = torch.empty((d, N), dtype=torch.float64, device="cuda")   # feature-major: what the library reads in place
    x_bar = torch.empty_like(feats_buf)
    torch.cuda.synchronize()
    data = _ffi.DeviceData.wrap(ctx, np.float64, d, N, N, feats_buf.data_ptr(), yt.data_ptr())
    dev = ag.DeviceLaplace(ctx, data=data)
    features = (lambda A: mlp(A)) if deep else (lambda A: A)

    def desc():   # warm start: every Newton loop begins at the previous step's mode
        k = float(log_var.detach().exp()) * ag.TransformedKernel(ag.SqExponentialKernel(), ag.ARDTransform(log_il.detach().exp().numpy()))
        return dev.desc(k, ag.BernoulliLikelihood(), 1e-6, warm_start=True)

    first = last = None
    for step in range(steps):
        opt.zero_grad()
        f = features(Xt)                                   # (N, d), in torch's graph
        with torch.no_grad():
            feats_buf.copy_(f.T)
        torch.cuda.synchronize()                           # the library runs on its own stream
        ds, keep = desc()
        lml, dv, dil, _, info = dev.lml_grad(ds, wrt_inputs=True, x_grad_out=x_bar)
        if deep:
            f.backward(-x_bar.T / N)                       # d(-lml / N) / d features, straight from device memory
        log_var.grad = torch.tensor(-dv * float(log_var.detach().exp()) / N, dtype=torch.float64)
        log_il.grad = torch.from_numpy(-dil * log_il.detach().exp().numpy() / N)
        opt.step()
        first = lml / N if step == 0 else first
        if step % 25 == 0 or step == steps - 1:
            print(f"  step {step:3d}  approx_lml / N {lml / N:8.4f}  Newton steps {info.iterations}")
    with torch.no_grad():
        feats_buf.copy_(features(Xt).T)
        fte = features(torch.from_numpy(Xte).cuda()).T.contiguous().cpu().numpy()
    torch.cuda.synchronize()
    ds, keep = desc()
    last = dev.fit(ds)[0] / N
    mean = dev.predict(fte, var=False)[0]                  # the latent mean: its sign is the predicted class
    dev.free()
    data.free()
    return first, last, float(np.mean((mean > 0) == (yte > 0.5)))


def main(N=2000, n_test=1000, steps=300):
    X, y, Xte, yte = make_data(N, n_test, 3)
    out = {}
    for name, deep in (("Laplace GP on the raw inputs (ARD)", False), ("Laplace GP on MLP features (deep kernel)", True)):
        print(name)
        out[name] = train(X, y, Xte, yte, deep, steps)
    for name, (a, b, acc) in out.items():
        print(f"{name:42s} approx_lml / N {a:8.4f} -> {b:8.4f}   held-out accuracy {acc:.4f}")
    return out


if __name__ == "__main__":
    main()
