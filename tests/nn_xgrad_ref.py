"""The NearestNeighbors (Vecchia) lml of tests/nn_noise_ref.py's formula header, restated in float64 torch as a loop of
torch.linalg.solve over the rows of a table, so that d lml / d x at the fixed table comes from autograd.  The Matern profiles take
the square root of torch.where(r2 > 0, r2, 1) and mask: the derivative at coincident points is then the correct zero, not NaN."""
import numpy as np
import torch

import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o


def _kappa(family, r2):
    """the unit-variance kernel of the squared scaled distance"""
    if family == o.KERNEL_SE:
        return torch.exp(-0.5 * r2)
    pos = r2 > 0
    r = torch.where(pos, torch.sqrt(torch.where(pos, r2, torch.ones_like(r2))), torch.zeros_like(r2))
    if family == o.KERNEL_MATERN32:
        return (1.0 + np.sqrt(3.0) * r) * torch.exp(-np.sqrt(3.0) * r)
    return (1.0 + np.sqrt(5.0) * r + (5.0 / 3.0) * r2) * torch.exp(-np.sqrt(5.0) * r)


def _r2(a, b):
    return ((a[:, :, None] - b[:, None, :]) ** 2).sum(0)   # the difference per entry, then the square


def lml_and_xbar(kernel, x, y, table, diag=0.0, s=None, mu=None, mean_const=0.0):
    """-> (lml, x_bar (d, n)): the sum over the points, and its gradient with respect to x by autograd"""
    xt = torch.tensor(nr._dn(x).astype(np.float64), requires_grad=True)
    n = xt.shape[1]
    sc = xt * torch.tensor(kernel.inv_lengthscale, dtype=torch.float64)[:, None]
    sig2 = torch.tensor(diag + (np.zeros(n) if s is None else np.asarray(s, dtype=np.float64)))
    delta = torch.tensor(np.asarray(y, dtype=np.float64) - mean_const - (np.zeros(n) if mu is None else np.asarray(mu, dtype=np.float64)))
    val = 0.0 * sc.sum()   # (n = 1: no block reads x, and its gradient is the zero it should be)
    for i in range(n):
        idx = torch.tensor(ns.row(table, i))
        F, r = kernel.variance + sig2[i], delta[i]
        if len(idx):
            pts = sc[:, idx]
            C = kernel.variance * _kappa(kernel.family, _r2(pts, pts)) + torch.diag(sig2[idx])
            c = kernel.variance * _kappa(kernel.family, _r2(pts, sc[:, i:i + 1]))[:, 0]
            b = torch.linalg.solve(C, c)
            F, r = F - c @ b, r - b @ delta[idx]
        val = val + nr.LOG2PI + torch.log(F) + r * r / F
    lml = -0.5 * val
    lml.backward()
    return float(lml.detach()), xt.grad.numpy()
