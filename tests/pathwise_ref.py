"""Float64 numpy restatement of pathwise posterior function samples (svgp_sampler_*; Wilson et al. 2020, Matheron's rule):

    f_s(x) = mean(x) + Phi(x) w_s + k(x, z) V_s,     V_s = Kuu^-1 (u_s - mean(z) - Phi(z) w_s),
    phi_l(x) = sqrt(2 variance / L) cos(sum_k omega_lk invl_k x_k + tau_l),
    NonCentered: u_s - mean(z) = Lk (m + Lq eps_s);    Centered: u_s - mean(z) = (m - mean(z)) + Lq eps_s;    mean(z) = mean_const + muz

with difference-form distances (svgp_oracle.kernelmatrix) and a Cholesky solve.  evaluate(..., f32=True) runs the data-sized stage
alone in float32, from the float64 V rounded once: what a straight float32 chain loses against float64 on the same numbers."""
import numpy as np
import scipy.linalg as sla

import svgp_oracle as o


def features(kernel, x, omega, tau, dtype=np.float64):
    """Phi(x): (n, L) without the amplitude sqrt(2 variance / L); every operation in `dtype`."""
    x = o._as_dn(np.asarray(x)).astype(dtype)
    xs = x * kernel.inv_lengthscale.astype(dtype)[:, None]
    phase = xs.T @ np.asarray(omega, dtype=dtype).T + np.asarray(tau, dtype=dtype)[None, :]
    return np.cos(phase)


def amplitude(kernel, L):
    return np.sqrt(2.0 * kernel.variance / L) if L > 0 else 0.0


def setup(sva, omega, tau, w, eps, muz=None):
    """The M-sized stage in float64 -> dict(u (M, S), V (M, S), Kuu, cond)."""
    z = sva.z.astype(np.float64)
    M = z.shape[1]
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, M)
    S = eps.shape[0]
    w = np.asarray(w, dtype=np.float64).reshape(S, -1)
    L = w.shape[1]
    Kuu = o.kernelmatrix(sva.kernel, z)
    Kuu[np.diag_indices_from(Kuu)] += sva.jitter
    Lk = np.linalg.cholesky(Kuu)
    mean_z = sva.mean_const + (0.0 if muz is None else np.asarray(muz, dtype=np.float64))
    m, Lq = sva.m.astype(np.float64), np.tril(sva.Lq.astype(np.float64))
    if sva.centered:
        u0 = (m - mean_z)[:, None] + Lq @ eps.T
    else:
        u0 = Lk @ (m[:, None] + Lq @ eps.T)
    phiz = amplitude(sva.kernel, L) * (features(sva.kernel, z, omega, tau) @ w.T) if L > 0 else np.zeros((M, S))
    V = sla.cho_solve((Lk, True), u0 - phiz)
    return {"u": u0 + np.broadcast_to(mean_z, (M,))[:, None], "V": V, "Kuu": Kuu, "cond": float(np.linalg.cond(Kuu))}


def evaluate(sva, st, x, omega, tau, w, mux=None, f32=False):
    """The data-sized stage -> F (S, n): F[s, j] = f_s(x_j).  f32: every array rounded once to float32 (V from its float64 values) and
    every operation of the stage in float32."""
    dt = np.float32 if f32 else np.float64
    x = o._as_dn(np.asarray(x)).astype(dt)
    z = sva.z.astype(dt)
    V = st["V"].astype(dt)
    S = V.shape[1]
    w = np.asarray(w, dtype=np.float64).reshape(S, -1)
    L = w.shape[1]
    Kxz = o.kernelmatrix(sva.kernel, x, z)          # difference-form distances, in dt
    F = (Kxz @ V).T
    if L > 0:
        wa = (amplitude(sva.kernel, L) * w).astype(dt)
        F = F + (features(sva.kernel, x, omega, tau, dt) @ wa.T).T
    mean = np.full(x.shape[1], sva.mean_const, dtype=dt)
    if mux is not None:
        mean = mean + np.asarray(mux, dtype=dt)
    F = mean[None, :] + F
    assert F.dtype == dt
    return F


def posterior_moments(sva, x, muz=None, mux=None):
    """Exact mean (n,) and covariance (n, n) of the posterior process at x, float64: what the samples' moments approach as L grows."""
    x = o._as_dn(np.asarray(x)).astype(np.float64)
    z = sva.z.astype(np.float64)
    Kuu = o.kernelmatrix(sva.kernel, z)
    Kuu[np.diag_indices_from(Kuu)] += sva.jitter
    Lk = np.linalg.cholesky(Kuu)
    mean_z = sva.mean_const + (0.0 if muz is None else np.asarray(muz, dtype=np.float64))
    m, Lq = sva.m.astype(np.float64), np.tril(sva.Lq.astype(np.float64))
    if sva.centered:
        du, Su = m - mean_z, Lq @ Lq.T
    else:
        du, Su = Lk @ m, Lk @ (Lq @ Lq.T) @ Lk.T
    Kxz = o.kernelmatrix(sva.kernel, x, z)
    Q = sla.cho_solve((Lk, True), Kxz.T)            # Kuu^-1 Kzx
    mean = sva.mean_const + (0.0 if mux is None else np.asarray(mux, dtype=np.float64)) + Q.T @ du
    cov = o.kernelmatrix(sva.kernel, x) - Kxz @ Q + Q.T @ Su @ Q
    return mean, cov


def recipe(M, d, family, seed, centered=False, mean_const=0.0, with_muz=False, variance=1.3, jitter=1e-3, dtype=np.float64):
    """The input recipe of the GPU tests: z ~ U[-3, 3]^d, ARD inverse lengthscales 0.8 M^(1/d) / 3 * U[0.8, 1.25], a whitened q of
    moderate size; Centered models are built from it (m = mean(z) + Lk m_w, Lq = Lk Lq_w).  Every array is rounded to `dtype` and
    returned widened, so that the restatement and the device start from the same numbers.  -> (SVA, muz or None)"""
    rng = np.random.default_rng(seed)
    rd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    z = rd(rng.uniform(-3.0, 3.0, size=(d, M)))
    invl = rd(0.8 * M ** (1.0 / d) / 3.0 * rng.uniform(0.8, 1.25, size=d))
    kernel = o.Kernel(family, variance, invl)
    m_w = 0.5 * rng.standard_normal(M)
    Lq_w = np.tril(0.3 * rng.standard_normal((M, M)) / np.sqrt(M), -1) + np.diag(rng.uniform(0.3, 0.8, size=M))
    muz = rd(0.2 * np.sin(z[0])) if with_muz else None
    if centered:
        Kuu = o.kernelmatrix(kernel, z)
        Kuu[np.diag_indices_from(Kuu)] += jitter
        Lk = np.linalg.cholesky(Kuu)
        m = mean_const + (0.0 if muz is None else muz) + Lk @ m_w
        Lq = Lk @ Lq_w
    else:
        m, Lq = m_w, Lq_w
    return o.SVA(kernel, z, rd(m), rd(Lq), jitter=jitter, mean_const=mean_const, centered=centered), muz
