"""Float64 numpy restatement of the collapsed (Titsias 2009, eqs. 11 / 12) bound and the optimal q(u), in M x M form so that it
works at any n (the sums over points are accumulated in chunks; no n x n matrix).  With Kuu = k(z, z) + jitter I = Lk Lk',
A = Lk \\ Kuf, r = y - mean_const:  C = A A', b = A r, t = tr C, rr = r'r,  B = I + C / s2 = LB LB',  c = LB \\ b / s2,
    bound = -n/2 log(2 pi s2) - sum log diag LB - rr / (2 s2) + c'c / 2 - (n variance - t) / (2 s2)
    m_w = LB' \\ c,  S_w = inv(B),  Lq_w = chol(S_w);  centered: m = mean_const + Lk m_w,  Lq = Lk Lq_w.
The gradient of the bound is taken by the envelope route: d elbo / d q = 0 at the optimal q, so svgp_oracle.elbo_grad at that q
gives the bound's total derivatives in the hyperparameters and z (tests/test_collapsed_cpu.py pins this to central differences of
svgp_oracle.titsias_bound)."""
import math
from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla

import svgp_oracle as o


@dataclass
class Collapsed:
    bound: float
    fit: float
    trace: float
    logdet_B: float
    logdet_kuu: float
    m_w: np.ndarray     # whitened optimum
    Lq_w: np.ndarray
    Lk: np.ndarray
    S_w: np.ndarray


def collapsed(kernel, z, jitter, x, sigma2, y, mean_const=0.0, chunk=8192) -> Collapsed:
    z = o._as_dn(np.asarray(z, dtype=np.float64))
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    M, n = z.shape[1], x.shape[1]
    Lk = np.linalg.cholesky(o.kernelmatrix(kernel, z) + jitter * np.eye(M))
    C, b, t, rr = np.zeros((M, M)), np.zeros(M), 0.0, 0.0
    for j0 in range(0, n, chunk):
        xs, r = x[:, j0:j0 + chunk], y[j0:j0 + chunk] - mean_const
        A = sla.solve_triangular(Lk, o.kernelmatrix(kernel, z, xs), lower=True)
        C += A @ A.T
        b += A @ r
        t += float(np.sum(A * A))
        rr += float(r @ r)
    B = np.eye(M) + C / sigma2
    LB = np.linalg.cholesky(B)
    c = sla.solve_triangular(LB, b, lower=True) / sigma2
    sld = float(np.sum(np.log(np.diag(LB))))
    fit = -0.5 * n * math.log(2 * math.pi * sigma2) - sld - rr / (2 * sigma2) + 0.5 * float(c @ c)
    trace = -(n * kernel.variance - t) / (2 * sigma2)
    m_w = sla.solve_triangular(LB, c, lower=True, trans="T")
    LBinv = sla.solve_triangular(LB, np.eye(M), lower=True)
    S_w = LBinv.T @ LBinv
    Lq_w = np.linalg.cholesky(0.5 * (S_w + S_w.T))
    return Collapsed(fit + trace, fit, trace, 2 * sld, 2 * float(np.sum(np.log(np.diag(Lk)))), m_w, Lq_w, Lk, S_w)


def optimal_sva(kernel, z, jitter, x, sigma2, y, mean_const=0.0, centered=False):
    """-> (oracle SVA at the optimal q in the asked parametrisation, Collapsed)."""
    r = collapsed(kernel, z, jitter, x, sigma2, y, mean_const)
    if centered:
        m, Lq = mean_const + r.Lk @ r.m_w, r.Lk @ r.Lq_w
    else:
        m, Lq = r.m_w, r.Lq_w
    return o.SVA(kernel, z, m, Lq, jitter=jitter, mean_const=mean_const, centered=centered), r


def bound_grad(kernel, z, jitter, x, sigma2, y, mean_const=0.0):
    """-> (bound, gradient dict of svgp_oracle.elbo_grad at the optimal q): variance, inv_lengthscale, z, lik_sigma2, mean_const are
    the bound's total derivatives; m and Lq are the (vanishing) partials in q."""
    sva, r = optimal_sva(kernel, z, jitter, x, sigma2, y, mean_const)
    val, g = o.elbo_grad(sva, x, y, lik=o.LIK_GAUSSIAN, sigma2=sigma2)
    return r.bound, val, g


def posterior_at(kernel, z, jitter, x, sigma2, y, xs, mean_const=0.0):
    """mean (n*), cov (n* x n*) of the SVGP posterior at the optimal q, from the whitened form directly."""
    r = collapsed(kernel, z, jitter, x, sigma2, y, mean_const)
    z = o._as_dn(np.asarray(z, dtype=np.float64))
    xs = o._as_dn(np.asarray(xs, dtype=np.float64))
    As = sla.solve_triangular(r.Lk, o.kernelmatrix(kernel, z, xs), lower=True)
    mean = mean_const + As.T @ r.m_w
    cov = o.kernelmatrix(kernel, xs) - As.T @ As + As.T @ r.S_w @ As
    return mean, cov


def problem(n, M, d, seed=0, family=o.KERNEL_SE, ard=False, dtype=np.float64, mean_const=0.0):
    """A seeded regression problem: x uniform in [0, 1]^d, z a subset-like draw, y = smooth function + noise + mean_const.  Arrays are
    float64 values rounded through `dtype`, so an fp32 device run and the fp64 reference see identical inputs."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * M + d)
    x = rng.random((d, n))
    z = rng.random((d, M))
    il = (1.0 + rng.random(d)) * (2.0 if d <= 3 else 1.0 / math.sqrt(d)) * 2.0
    if not ard:
        il = np.full(d, il[0])
    w = rng.standard_normal(d)
    sigma2 = 0.05 + 0.1 * rng.random()
    y = np.sin(3.0 * (w @ x)) + math.sqrt(sigma2) * rng.standard_normal(n) + mean_const
    rd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    kernel = o.Kernel(family, float(rd(0.8 + 0.5 * rng.random())), rd(il))
    return kernel, rd(z), rd(x), rd(y), float(rd(sigma2))
