"""Float64 numpy restatement of the collapsed bound with per-point noise variances and any prior mean (svgp_collapsed_*_with_noise),
in M x M form so that it works at any n.  With Kuu = k(z, z) + jitter I = Lk Lk', A = Lk \\ Kuf and, per point j of the window,
    sigma_j^2 = sigma2 + s_j,  w_j = 1 / sigma_j^2,  r_j = y_j - mean_const - mux_j:
    C = sum w_j a_j a_j',  b = sum w_j a_j r_j,  rr = sum w_j r_j^2,  t = sum w_j (variance - |a_j|^2),  ld = sum log sigma_j^2,
    B = I + C = LB LB',  c = LB \\ b,
    bound = -n/2 log 2 pi - ld / 2 - sum log diag LB - rr / 2 + c'c / 2 - t / 2
    m_w = LB' \\ c,  S_w = inv(B);  centered: m = mean_const + muz + Lk m_w,  Lq = Lk chol(S_w).
The gradient is taken by the envelope route of tests/collapsed_ref.py: d elbo / d q = 0 at the optimal q, so the ELBO's partial
derivatives there - svgp_oracle.elbo_grad with the point gradients of the Gaussian likelihood evaluated with sigma_j^2 - are the
bound's total ones; the per-point blocks are
    s_bar_j = -1 / (2 sigma_j^2) + ((r_j - mu~_j)^2 + v_j) / (2 sigma_j^4),   mux_bar_j = (r_j - mu~_j) / sigma_j^2
with mu~_j = a_j' m_w and v_j = variance - |a_j|^2 + a_j' S_w a_j the marginals of the optimal q without the prior mean.
tests/test_collapsed_noise_cpu.py pins all of this to the dense n x n expression and to central differences."""
import math
from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla

import input_grad_ref
import svgp_oracle as o


@dataclass
class CollapsedNoise:
    bound: float
    fit: float
    trace: float
    logdet_B: float
    logdet_kuu: float
    m_w: np.ndarray     # whitened optimum
    Lq_w: np.ndarray
    Lk: np.ndarray
    S_w: np.ndarray


def _vec(v, n):
    return np.zeros(n) if v is None else np.asarray(v, dtype=np.float64).reshape(n)


def collapsed(kernel, z, jitter, x, sigma2, s, y, mean_const=0.0, mux=None, chunk=8192) -> CollapsedNoise:
    z = o._as_dn(np.asarray(z, dtype=np.float64))
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    M, n = z.shape[1], x.shape[1]
    sig = sigma2 + _vec(s, n)
    mux = _vec(mux, n)
    Lk = np.linalg.cholesky(o.kernelmatrix(kernel, z) + jitter * np.eye(M))
    C, b, t, rr = np.zeros((M, M)), np.zeros(M), 0.0, 0.0
    for j0 in range(0, n, chunk):
        sl = slice(j0, j0 + chunk)
        w, r = 1.0 / sig[sl], y[sl] - mean_const - mux[sl]
        A = sla.solve_triangular(Lk, o.kernelmatrix(kernel, z, x[:, sl]), lower=True)
        C += (A * w) @ A.T
        b += A @ (w * r)
        t += float(np.sum(w * (kernel.variance - np.sum(A * A, 0))))
        rr += float(np.sum(w * r * r))
    LB = np.linalg.cholesky(np.eye(M) + C)
    c = sla.solve_triangular(LB, b, lower=True)
    sld = float(np.sum(np.log(np.diag(LB))))
    fit = -0.5 * n * math.log(2 * math.pi) - 0.5 * float(np.sum(np.log(sig))) - sld - 0.5 * rr + 0.5 * float(c @ c)
    trace = -0.5 * t
    m_w = sla.solve_triangular(LB, c, lower=True, trans="T")
    LBinv = sla.solve_triangular(LB, np.eye(M), lower=True)
    S_w = LBinv.T @ LBinv
    Lq_w = np.linalg.cholesky(0.5 * (S_w + S_w.T))
    return CollapsedNoise(fit + trace, fit, trace, 2 * sld, 2 * float(np.sum(np.log(np.diag(Lk)))), m_w, Lq_w, Lk, S_w)


def optimal_q(r: CollapsedNoise, mean_const=0.0, muz=None, centered=False):
    """-> (m, Lq) of the optimal q in the asked parametrisation."""
    if not centered:
        return r.m_w, r.Lq_w
    return mean_const + _vec(muz, r.m_w.shape[0]) + r.Lk @ r.m_w, r.Lk @ r.Lq_w


def dense_bound(kernel, z, jitter, x, sigma2, s, y, mean_const=0.0, mux=None):
    """log N(r | 0, Qff + diag sigma^2) - 1/2 sum (k_jj - q_jj) / sigma_j^2 from the n x n matrices -> (bound, fit, trace)."""
    z = o._as_dn(np.asarray(z, dtype=np.float64))
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    M, n = z.shape[1], x.shape[1]
    sig = sigma2 + _vec(s, n)
    r = np.asarray(y, dtype=np.float64) - mean_const - _vec(mux, n)
    Kuf = o.kernelmatrix(kernel, z, x)
    Q = Kuf.T @ np.linalg.solve(o.kernelmatrix(kernel, z) + jitter * np.eye(M), Kuf)
    L = np.linalg.cholesky(Q + np.diag(sig))
    a = sla.solve_triangular(L, r, lower=True)
    fit = -0.5 * n * math.log(2 * math.pi) - float(np.sum(np.log(np.diag(L)))) - 0.5 * float(a @ a)
    trace = -0.5 * float(np.sum((o.kernelmatrix_diag(kernel, x) - np.diag(Q)) / sig))
    return fit + trace, fit, trace


def bound_grad(kernel, z, jitter, x, sigma2, s, y, mean_const=0.0, mux=None, want_x=False):
    """-> (CollapsedNoise, dict): variance, inv_lengthscale, z (d, M), lik_sigma2, mean_const, noise (n,) = s_bar, mean_x (n,) =
    mux_bar and, with want_x, x (d, n): the bound's total derivatives, by the envelope route."""
    z = o._as_dn(np.asarray(z, dtype=np.float64))
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    n = x.shape[1]
    sig = sigma2 + _vec(s, n)
    mux = _vec(mux, n)
    r = collapsed(kernel, z, jitter, x, sigma2, s, y, mean_const, mux)
    A = sla.solve_triangular(r.Lk, o.kernelmatrix(kernel, z, x), lower=True)
    Cq = r.Lq_w.T @ A
    res = (y - mean_const - mux) - A.T @ r.m_w
    v = kernel.variance - np.sum(A * A, 0) + np.sum(Cq * Cq, 0) + o.DEFAULT_SIGMA2
    gmu, gv = res / sig, -0.5 / sig
    s_bar = -0.5 / sig + 0.5 * (res * res + v) / sig**2
    sva = o.SVA(kernel, z, r.m_w, r.Lq_w, jitter=jitter, mean_const=mean_const, centered=False)
    _, g = o.elbo_grad(sva, x, None, point_grads=(0.0, gmu, gv))
    out = dict(variance=g["variance"], inv_lengthscale=g["inv_lengthscale"], z=g["z"], mean_const=g["mean_const"],
               lik_sigma2=float(np.sum(s_bar)), noise=s_bar, mean_x=gmu, m=g["m"], Lq=g["Lq"])
    if want_x:
        out["x"] = input_grad_ref.input_grad(sva, x, None, point_grads=(0.0, gmu, gv))
    return r, out


def problem(n, M, d, seed=0, family=o.KERNEL_SE, ard=False, dtype=np.float64, mean_const=0.0, noise_decades=4.0, mean_scale=1.0):
    """tests/collapsed_ref.problem plus a noise vector whose entries span `noise_decades` orders of magnitude (sigma_j^2 = sigma2 + s_j,
    s_j >= 0, the observations carry that noise) and prior mean offsets of the size of y at x and at z.  Values are rounded through
    `dtype`, so an fp32 device run and the fp64 reference see identical inputs.  -> kernel, z, x, y, sigma2, s, mux, muz"""
    rng = np.random.default_rng(2000 * seed + 7 * n + 3 * M + d)
    x = rng.random((d, n))
    z = rng.random((d, M))
    il = (1.0 + rng.random(d)) * (2.0 if d <= 3 else 1.0 / math.sqrt(d)) * 2.0
    if not ard:
        il = np.full(d, il[0])
    w = rng.standard_normal(d)
    sigma2 = 0.01 * (1.0 + rng.random())
    s = sigma2 * (10.0 ** (noise_decades * rng.random(n)) - 1.0)
    tw = rng.standard_normal(d)
    mux = mean_scale * np.cos(2.0 * (tw @ x))
    muz = mean_scale * np.cos(2.0 * (tw @ z))
    y = np.sin(3.0 * (w @ x)) + mux + np.sqrt(sigma2 + s) * rng.standard_normal(n) + mean_const
    rd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    kernel = o.Kernel(family, float(rd(0.8 + 0.5 * rng.random())), rd(il))
    return kernel, rd(z), rd(x), rd(y), float(rd(sigma2)), rd(s), rd(mux), rd(muz)
