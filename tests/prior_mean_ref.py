"""Float64 reference for prior mean offsets (svgp_*_with_mean, svgp_model_set_mean_z).

A model may carry offsets muz at the inducing points and a call offsets mux at the batch's points; both add to the constant mean:
    mean(f.prior, x_j) = c + mux[j],   mean(fz)_k = c + muz[k].
The posterior mean is mu_j = (c + mux[j]) + (A' m~)_j; Centered m~ = Lk \\ (m - c - muz), NonCentered m~ = m (muz has no effect).
This is the oracle's elbo_grad (oracle/svgp_oracle.py) with the scalar c replaced by those vectors; the gradient dict gains
"mean_x" = scale dE_j/dmu_j and "mean_z" = -m_bar (Centered) or 0 (NonCentered), and "mean_const" stays sum(mean_x) + sum(mean_z)."""
import numpy as np
import scipy.linalg as sla

import svgp_oracle as o


def _offsets(sva, n, mux, muz):
    mux = np.zeros(n) if mux is None else np.asarray(mux, dtype=np.float64).reshape(n)
    muz = np.zeros(sva.z.shape[1]) if muz is None else np.asarray(muz, dtype=np.float64).reshape(sva.z.shape[1])
    return mux, muz


def _whitened(sva, Lk, muz):
    if sva.centered:
        m = sla.solve_triangular(Lk, (sva.m.astype(np.float64) - sva.mean_const) - muz, lower=True)
        Lq = sla.solve_triangular(Lk, np.tril(sva.Lq).astype(np.float64), lower=True)
    else:
        m, Lq = sva.m.astype(np.float64), np.tril(sva.Lq).astype(np.float64)
    return m, Lq


def marginals(sva, x, mux=None, muz=None):
    """-> (mu, v + 1e-18) of the batch x: what svgp_marginals_with_mean returns."""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    mux, muz = _offsets(sva, x.shape[1], mux, muz)
    k = sva.kernel
    z = sva.z.astype(np.float64)
    Kuf = o._kappa(k, o._scaled_sqdist(k, z, x))
    Lk = o._chol_lower_checked(o._kappa(k, o._scaled_sqdist(k, z, z)) + sva.jitter * np.eye(z.shape[1]))
    m, Lq = _whitened(sva, Lk, muz)
    A = sla.solve_triangular(Lk, Kuf, lower=True)
    C = Lq.T @ A
    return (sva.mean_const + mux) + A.T @ m, k.variance - np.sum(A * A, 0) + np.sum(C * C, 0) + o.DEFAULT_SIGMA2


def elbo(sva, x, y, mux=None, muz=None, lik=o.LIK_GAUSSIAN, sigma2=1.0, num_data=None, quadrature_n=0):
    return elbo_grad(sva, x, y, mux, muz, lik, sigma2, num_data, quadrature_n, want_grad=False)[0]


def elbo_grad(sva, x, y, mux=None, muz=None, lik=o.LIK_GAUSSIAN, sigma2=1.0, num_data=None, quadrature_n=0, point_grads=None,
              want_grad=True):
    """-> (elbo, dict(variance, inv_lengthscale, z, m, Lq, lik_sigma2, mean_const, mean_x, mean_z)).  point_grads = (sum_e, g_mu, g_v):
    a likelihood the caller evaluated on the marginals (svgp_elbo_grad_with_mean with g_mu / g_v)."""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    y = None if y is None else np.asarray(y, dtype=np.float64)
    k = sva.kernel
    il = k.inv_lengthscale
    z = sva.z.astype(np.float64)
    M, n = z.shape[1], x.shape[1]
    mux, muz = _offsets(sva, n, mux, muz)
    scale = (float(num_data) if num_data is not None else float(n)) / n
    r2_uf = o._scaled_sqdist(k, z, x)
    Kuf = o._kappa(k, r2_uf)
    r2_uu = o._scaled_sqdist(k, z, z)
    Kuu = o._kappa(k, r2_uu) + sva.jitter * np.eye(M)
    Lk = o._chol_lower_checked(Kuu.copy())
    m, Lq = _whitened(sva, Lk, muz)
    A = sla.solve_triangular(Lk, Kuf, lower=True)
    C = Lq.T @ A
    mu = (sva.mean_const + mux) + A.T @ m
    v = k.variance - np.sum(A * A, 0) + np.sum(C * C, 0) + o.DEFAULT_SIGMA2
    kl = 0.5 * (np.sum(Lq * Lq) + m @ m - M - 2.0 * np.sum(np.log(np.diag(Lq))))
    if point_grads is not None:
        E, gmu, gv, gs2 = float(point_grads[0]), np.asarray(point_grads[1], dtype=np.float64), np.asarray(point_grads[2], dtype=np.float64), 0.0
    else:
        E = o.expected_loglik(lik, mu, np.sqrt(v), y, sigma2, quadrature_n)
        if not want_grad:
            return E * scale - kl, None
        gmu, gv, gs2 = o.expected_loglik_grads(lik, mu, v, y, sigma2, quadrature_n)
    gmu, gv, gs2 = scale * gmu, scale * gv, scale * gs2
    Abar = np.outer(m, gmu) + 2.0 * (Lq @ C - A) * gv[None, :]
    m_bar = A @ gmu - m
    Lq_bar = np.tril(2.0 * (A * gv[None, :]) @ C.T) - (Lq - np.diag(1.0 / np.diag(Lq)))
    P = sla.solve_triangular(Lk, Abar, lower=True, trans="T")
    Lk_bar = -np.tril(P @ A.T)
    muz_bar = np.zeros(M)
    if sva.centered:
        r_bar = sla.solve_triangular(Lk, m_bar, lower=True, trans="T")
        R = sla.solve_triangular(Lk, Lq_bar, lower=True, trans="T")
        Lk_bar -= np.tril(np.outer(r_bar, m)) + np.tril(R @ Lq.T)
        m_bar, Lq_bar = r_bar, np.tril(R)
        muz_bar = -r_bar                       # m enters only through m - c - muz
    H = o.chol_backward(Lk, Lk_bar)
    var_bar = float(np.sum(P * Kuf) / k.variance + np.sum(H * (Kuu - sva.jitter * np.eye(M))) / k.variance + np.sum(gv))
    Wf = P * o._dkappa_dr2(k, r2_uf)
    Wu = H * o._dkappa_dr2(k, r2_uu)
    il_bar = np.zeros_like(il)
    z_bar = np.zeros_like(z)
    for f in range(z.shape[0]):
        dzx = z[f][:, None] - x[f][None, :]
        dzz = z[f][:, None] - z[f][None, :]
        il_bar[f] = 2.0 * il[f] * (np.sum(Wf * dzx * dzx) + np.sum(Wu * dzz * dzz))
        z_bar[f] = 2.0 * il[f] ** 2 * (np.sum(Wf * dzx, 1) + 2.0 * np.sum(Wu * dzz, 1))
    grads = dict(variance=var_bar, inv_lengthscale=il_bar, z=z_bar, m=m_bar, Lq=Lq_bar, lik_sigma2=gs2,
                 mean_const=float(np.sum(gmu) + np.sum(muz_bar)), mean_x=gmu, mean_z=muz_bar)
    return E * scale - kl, grads
