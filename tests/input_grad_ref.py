"""Reference d elbo / d x for the input-gradient tests, in float64.

The oracle's adjoint (svgp_oracle.elbo_grad) is restated up to P = Kuf_bar; then, with W = P o dk/dr2,
    x_bar_fj = 2 lambda_f^2 sum_i W_ij (x_fj - z_fi)
- the oracle's Wf reduced over the inducing rows instead of over the points (its z gradient)."""
import numpy as np
import scipy.linalg as sla

import svgp_oracle as o


def input_grad(sva, x, y, lik=o.LIK_GAUSSIAN, sigma2=1.0, num_data=None, quadrature_n=0, point_grads=None):
    """-> x_bar, (d, n) float64, for the batch x (any layout svgp_oracle accepts; a vector is d = 1).
    point_grads = (sum_e, g_mu, g_v): a likelihood the caller evaluated (svgp_elbo_grad_ext_inputs' route)."""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    k = sva.kernel
    il = np.asarray(k.inv_lengthscale, dtype=np.float64)
    z = np.asarray(sva.z, dtype=np.float64)
    M, n = z.shape[1], x.shape[1]
    scale = (float(num_data) if num_data is not None else float(n)) / n
    r2_uf = o._scaled_sqdist(k, z, x)
    Kuf = o._kappa(k, r2_uf)
    Kuu = o._kappa(k, o._scaled_sqdist(k, z, z)) + sva.jitter * np.eye(M)
    Lk = o._chol_lower_checked(Kuu.copy())
    if sva.centered:
        m = sla.solve_triangular(Lk, sva.m.astype(np.float64) - sva.mean_const, lower=True)
        Lq = sla.solve_triangular(Lk, np.tril(sva.Lq).astype(np.float64), lower=True)
    else:
        m, Lq = sva.m.astype(np.float64), np.tril(sva.Lq).astype(np.float64)
    A = sla.solve_triangular(Lk, Kuf, lower=True)
    C = Lq.T @ A
    if point_grads is not None:
        gmu, gv = (np.asarray(a, dtype=np.float64) for a in point_grads[1:])
    else:
        mu = sva.mean_const + A.T @ m
        v = k.variance - np.sum(A * A, 0) + np.sum(C * C, 0) + o.DEFAULT_SIGMA2
        gmu, gv, _ = o.expected_loglik_grads(lik, mu, v, np.asarray(y, dtype=np.float64), sigma2, quadrature_n)
    gmu, gv = scale * gmu, scale * gv
    Abar = np.outer(m, gmu) + 2.0 * (Lq @ C - A) * gv[None, :]
    P = sla.solve_triangular(Lk, Abar, lower=True, trans="T")   # Kuf_bar
    W = P * o._dkappa_dr2(k, r2_uf)
    xbar = np.empty_like(x)
    for f in range(x.shape[0]):
        xbar[f] = 2.0 * il[f] ** 2 * (x[f] * W.sum(0) - z[f] @ W)
    return xbar
