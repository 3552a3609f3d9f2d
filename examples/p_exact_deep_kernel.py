#!/usr/bin/env python
"""Deep kernel learning with an EXACT GP: a torch MLP maps 6-dimensional inputs to 2 features, an SE-ARD exact GP by matrix-free
conjugate gradients (ConjugateGradients' device handle, svgp_cg_*) sits on the features, and both are trained jointly on the log
marginal likelihood (Wilson et al. 2016 on GPyTorch's BBMM).  What makes it possible is the gradient of the lml with respect to the
GP's INPUTS (svgp_cg_lml_grad_inputs): the features stay in torch's device memory (DeviceData.wrap, no host round trip), x_bar is written
into a torch tensor, and one `features.backward(-x_bar)` carries it into the MLP.  The kernel's own parameters and the noise take their
gradients from the same call.  The target depends on all six inputs through ONE nonlinear index, which a stationary ARD kernel on the raw
inputs cannot exploit: the same GP is trained on the raw inputs for comparison.

    python examples/p_exact_deep_kernel.py          # needs an MI355X
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
    u = np.tanh(X @ np.array([1.0, -0.8, 0.6, 0.9, -0.7, 0.5]))         # the 1-D index the target really depends on: every input enters
    y = np.sin(5.0 * u) + 0.1 * rng.standard_normal(N + n_test)
    return X[:N], y[:N], X[N:], y[N:]


def train(X, y, Xte, yte, deep, steps, seed=0):
    """-> (lml / N before, after, held-out RMSE).  deep: the MLP in front; otherwise the raw inputs with their own ARD lengthscales"""
    torch.manual_seed(seed)
    N = X.shape[0]
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y.copy()).cuda()
    d = 2 if deep else X.shape[1]
    mlp = torch.nn.Sequential(torch.nn.Linear(X.shape[1], 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                              torch.nn.Linear(32, d)).double().cuda() if deep else None
    log_var, log_noise = torch.zeros((), dtype=torch.float64, requires_grad=True), torch.tensor(np.log(0.05), dtype=torch.float64, requires_grad=True)
    log_il = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    params = [log_var, log_noise, log_il] + (list(mlp.parameters()) if deep else [])
    opt = torch.optim.Adam(params, lr=0.01)

    ctx = _ffi.default_context()
    feats_buf = torch.empty((d, N), dtype=torch.float64, device="cuda")   # feature-major: what the library reads in place
    x_bar = torch.empty_like(feats_buf)
    torch.cuda.synchronize()
    data = _ffi.DeviceData.wrap(ctx, np.float64, d, N, N, feats_buf.data_ptr(), yt.data_ptr())
    dev = ag.DeviceConjugateGradients(ctx, data=data)
    fixed = ag.draw_probes(N, 16, 10_000)   # reporting only: the lml before and after on one set of probes
    features = (lambda A: mlp(A)) if deep else (lambda A: A)

    def kernel():
        return float(log_var.detach().exp()) * ag.TransformedKernel(ag.SqExponentialKernel(), ag.ARDTransform(log_il.detach().exp().numpy()))

    first = last = None
    for step in range(steps):
        opt.zero_grad()
        f = features(Xt)                                   # (N, d), in torch's graph
        with torch.no_grad():
            feats_buf.copy_(f.T)
        torch.cuda.synchronize()                           # the library runs on its own stream
        desc, keep = dev.desc(kernel(), float(log_noise.detach().exp()), tol=1e-6, maxiter=500)
        # fresh probes at every step: the trace estimator is unbiased for the gradient but is not the derivative of the estimated
        # value, and a network with a thousand weights would learn to exploit the error of one fixed set of probes
        lml, g, info = dev.lml_grad(desc, ag.draw_probes(N, 16, step), wrt_inputs=True, x_grad_out=x_bar)
        if deep:
            f.backward(-x_bar.T / N)                       # d(-lml / N) / d features, straight from device memory
        log_var.grad = torch.tensor(-g["variance"] * float(log_var.detach().exp()) / N, dtype=torch.float64)
        log_noise.grad = torch.tensor(-g["diag"] * float(log_noise.detach().exp()) / N, dtype=torch.float64)
        log_il.grad = torch.from_numpy(-g["inv_lengthscale"] * log_il.detach().exp().numpy() / N)
        opt.step()
        if step == 0:
            first = dev.fit(desc, fixed)[0] / N
        if step % 20 == 0 or step == steps - 1:
            print(f"  step {step:3d}  lml / N {lml / N:8.4f}  noise variance {float(log_noise.detach().exp()):.4f}  CG iterations {info.iterations}")
    with torch.no_grad():
        feats_buf.copy_(features(Xt).T)
        fte = features(torch.from_numpy(Xte).cuda()).T.contiguous().cpu().numpy()
    torch.cuda.synchronize()
    desc, keep = dev.desc(kernel(), float(log_noise.detach().exp()), tol=1e-6, maxiter=500)
    last = dev.fit(desc, fixed)[0] / N
    mean = dev.predict(fte, var=False)[0]
    dev.free()
    data.free()
    return first, last, float(np.sqrt(np.mean((mean - yte) ** 2)))


def main(N=3000, n_test=1000, steps=200):
    X, y, Xte, yte = make_data(N, n_test, 3)
    out = {}
    for name, deep in (("exact GP on the raw inputs (ARD)", False), ("exact GP on MLP features (deep kernel)", True)):
        print(name)
        out[name] = train(X, y, Xte, yte, deep, steps)
    for name, (a, b, rmse) in out.items():
        print(f"{name:42s} lml / N {a:8.4f} -> {b:8.4f}   held-out RMSE {rmse:.4f}   (the noise's own: 0.1)")
    return out


if __name__ == "__main__":
    main()
