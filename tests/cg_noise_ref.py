"""Numpy restatement of the exact GP by conjugate gradients with per-point noise variances (svgp_cg_set_noise, svgp_cg_lml_grad_noise),
in float64 and with float32 vectors, on top of tests/cg_ref.py and tests/cg_precond_ref.py:
  sigma_i^2 = T(diag) + T(s_i) in the data dtype T with one rounding,   Khat = K + D,  D = diag(sigma^2),
  s_bar_i = d lml / d sigma_i^2 = 1/2 alpha_i^2 - (1 / 2T) sum_t w_it p_it   (t ascending in float64, rounded once to T),
  variance d_variance = 1/2 alpha' Khat alpha - (1 / 2T) sum_t w_t' Khat p_t - sum_i sigma_i^2 s_bar_i,
  P = Z Kuu^-1 Z' + D:  P^-1 r = D^-1 (r - Z W Z' D^-1 r),  W = Lu^-T B^-1 Lu^-1,  B = I + Lu^-1 (Z' D^-1 Z) Lu^-T,
  log det P = sum_i log sigma_i^2 + log det B,  probes z_t = D^1/2 eps_t + Z Lu^-T xi_t,
  sampler right-hand sides delta - Phi(X) w_s - sigma_i eps_si.
The batched recurrences are cg_ref.mbcg and cg_precond_ref.pmbcg themselves; the kernel chains are cg_ref's."""
import math

import numpy as np

import cg_precond_ref as pr
import cg_ref as cr
import svgp_oracle as o

DIAG = 0.05


def xy(N, d, seed=0):
    """tests/test_gpu_cg.py's _xy (x ~ U[-3, 3]^d, y = sin(sum x) + 0.1 noise), restated so that the CPU suite needs no GPU module"""
    rng = np.random.default_rng(1000 + 7 * N + 13 * d + seed)
    x = rng.uniform(-3, 3, size=(d, N))
    return x, np.sin(x.sum(0)) + 0.1 * rng.standard_normal(N)


def noise_vector(N, seed=11):
    """the suites' per-point term: s = exp(U[log 0.02, log 0.5])"""
    return np.exp(np.random.default_rng(seed).uniform(math.log(0.02), math.log(0.5), size=N))


def sigma2(diag, s, dtype=np.float64):
    """T(diag) + T(s) in T, as float64 values"""
    return (dtype(diag) + np.asarray(s).astype(dtype)).astype(dtype).astype(np.float64)


def khat(kernel, x, sig2):
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    return o.kernelmatrix(kernel, x) + np.diag(np.asarray(sig2, dtype=np.float64))


def kmv_f32(kernel, x, V, sig2):
    """the float32 chain of Khat V (cg_ref.kmv_f32 with the per-point factor)"""
    K, _ = cr.kernel_chain(kernel, x, np.float32)
    V = np.asarray(V, dtype=np.float32)
    return K @ V + np.asarray(sig2, dtype=np.float32)[:, None] * V


def dense_lml(kernel, x, sig2, delta):
    """the exact GP: log N(delta; 0, K + D), float64"""
    Kh = khat(kernel, x, sig2)
    L = np.linalg.cholesky(Kh)
    a = np.linalg.solve(L, np.asarray(delta, dtype=np.float64))
    return -0.5 * (float(a @ a) + 2.0 * float(np.log(np.diag(L)).sum()) + len(a) * math.log(2 * math.pi))


def _dot(u, v):
    return np.einsum("is,is->s", u.astype(np.float64), v.astype(np.float64))


def s_bar(X, P, T, dtype):
    """from the panels X = [alpha, w_t] and P = [alpha, p_t]: t ascending in float64, one rounding"""
    X64, P64 = X.astype(np.float64), P.astype(np.float64)
    if T < 1:
        return np.full(X.shape[0], np.nan, dtype=dtype)
    tr = np.zeros(X.shape[0])
    for t in range(1, T + 1):
        tr = tr + X64[:, t] * P64[:, t]
    return (0.5 * (X64[:, 0] * P64[:, 0]) - tr / (2.0 * T)).astype(dtype)


def _chain(kernel, x, dtype):
    if dtype == np.float64:
        K, dKv, dKil = cr.dense_dk(kernel, x)
        il = kernel.inv_lengthscale
        return K, [dKil[c] * il[c] for c in range(len(il))], il
    K, D2 = cr.kernel_chain(kernel, x, dtype)
    return K, D2, kernel.inv_lengthscale.astype(dtype).astype(np.float64)


def _gradient(kernel, K, D2, il, dgv, X, P, T, dtype):
    up = _dot(X, P)
    KP = np.asarray(K @ P + dgv[:, None] * P, dtype=dtype)
    sb = s_bar(X, P, T, dtype)
    return {
        "diag": cr._combine(up, T),
        "variance": (cr._combine(_dot(X, KP), T) - float(np.sum(dgv.astype(np.float64) * sb.astype(np.float64)))) / kernel.variance,
        "inv_lengthscale": np.array([cr._combine(_dot(X, np.asarray(D2[c] @ P, dtype=dtype)), T) / il[c] for c in range(len(D2))]),
        "mean_const": float(X[:, 0].astype(np.float64).sum()),
        "noise": sb,
    }


def estimate(kernel, x, diag, s, delta, probes, tol, maxiter, dtype=np.float64, grad=False):
    """cg_ref.estimate with Khat = K + D (s None: D = T(diag) I, the plain handle); the gradient carries "noise" = s_bar"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    probes = np.asarray(probes, dtype=np.float64).reshape(N, -1)
    T = probes.shape[1]
    K, D2, il = _chain(kernel, x, dtype)
    dgv = sigma2(diag, np.zeros(N) if s is None else s, dtype).astype(dtype)
    B = np.column_stack([np.asarray(delta, dtype=np.float64), probes]).astype(dtype)
    X, iters, rel, ca, cb, bb = cr.mbcg(lambda P: K @ P + dgv[:, None] * P, B, tol, maxiter, dtype)
    quad = float(_dot(B[:, :1], X[:, :1])[0])
    logdet = sum(bb[t] * cr.lanczos_quad(ca[t], cb[t]) for t in range(1, T + 1) if ca[t]) / T if T else float("nan")
    out = {"quad": quad, "logdet": logdet, "lml": -0.5 * (quad + logdet + N * math.log(2 * math.pi)), "alpha": X[:, 0], "W": X[:, 1:],
           "iters": iters, "rel": rel}
    if grad:
        P = B.copy()
        P[:, 0] = X[:, 0]
        out["grad"] = _gradient(kernel, K, D2, il, dgv, X, P, T, dtype)
    return out


def dense_estimate(kernel, x, sig2, delta, probes):
    """cg_ref.dense_estimate with Khat = K + D: dense float64 solves in place of CG, the exact quadratic form in place of the
    quadrature; "noise" is the estimator of d lml / d sigma_i^2"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    probes = np.asarray(probes, dtype=np.float64).reshape(N, -1)
    T = probes.shape[1]
    K, dKv, dKil = cr.dense_dk(kernel, x)
    Kh = K + np.diag(np.asarray(sig2, dtype=np.float64))
    lam, Q = np.linalg.eigh(Kh)
    alpha = np.linalg.solve(Kh, delta)
    W = np.linalg.solve(Kh, probes)
    quad = float(delta @ alpha)
    logdet = float(np.sum((Q.T @ probes) ** 2 * np.log(lam)[:, None]) / T)
    term = lambda dK: 0.5 * alpha @ dK @ alpha - np.einsum("it,ij,jt->", W, dK, probes) / (2.0 * T)
    sb = 0.5 * alpha * alpha - (W * probes).sum(1) / (2.0 * T)
    return {"quad": quad, "logdet": logdet, "lml": -0.5 * (quad + logdet + N * math.log(2 * math.pi)), "alpha": alpha,
            "grad": {"diag": float(sb.sum()), "variance": term(dKv), "inv_lengthscale": np.array([term(d) for d in dKil]),
                     "mean_const": float(alpha.sum()), "noise": sb}}


def dense_noise_gradient(kernel, x, sig2, delta):
    """the exact d lml / d sigma_i^2 = 1/2 (alpha_i^2 - (Khat^-1)_ii)"""
    Ki = np.linalg.inv(khat(kernel, x, sig2))
    a = Ki @ np.asarray(delta, dtype=np.float64)
    return 0.5 * (a * a - np.diag(Ki))


class Nystrom:
    """cg_precond_ref.Nystrom with D = diag(sig2) in place of s2 I; sig2: the values the device forms (sigma2(diag, s, dtype))"""

    def __init__(self, kernel, x, zp, sig2, jitter=1e-4, dtype=np.float64):
        x = o._as_dn(np.asarray(x, dtype=np.float64))
        zp = o._as_dn(np.asarray(zp, dtype=np.float64))
        self.N, self.k, self.dtype = x.shape[1], zp.shape[1], dtype
        self.sig2 = np.asarray(sig2, dtype=np.float64)
        self.Z = o.kernelmatrix(kernel, x, zp)
        Kuu = o.kernelmatrix(kernel, zp, zp) + jitter * kernel.variance * np.eye(self.k)
        self.Lu = np.linalg.cholesky(Kuu)
        self.G = self.Z.T @ (self.Z / self.sig2[:, None])
        A = np.linalg.solve(self.Lu, np.linalg.solve(self.Lu, self.G).T)
        self.B = np.eye(self.k) + 0.5 * (A + A.T)
        self.LB = np.linalg.cholesky(self.B)
        Li = np.linalg.inv(self.Lu)
        self.W = Li.T @ np.linalg.solve(self.B, Li)
        self.logdet = float(np.log(self.sig2).sum()) + 2.0 * float(np.log(np.diag(self.LB)).sum())
        self.Zv = self.Z if dtype == np.float64 else cr.kernel_chain(kernel, x, dtype, xt=zp)[0].T.copy()
        self.isig = (1.0 / self.sig2).astype(dtype)
        self.ssig = np.sqrt(self.sig2).astype(dtype)

    def dense(self):
        return self.Z @ np.linalg.solve(self.Lu.T, np.linalg.solve(self.Lu, self.Z.T)) + np.diag(self.sig2)

    def apply(self, R):
        R = np.asarray(R, dtype=self.dtype)
        u = (R * self.isig[:, None]).astype(self.dtype)
        t = (self.Zv.T @ u).astype(self.dtype)
        v = (-(self.W @ t.astype(np.float64))).astype(self.dtype)
        return ((self.Zv @ v + R).astype(self.dtype) * self.isig[:, None]).astype(self.dtype)

    def probes(self, eps, xi):
        u = np.linalg.solve(self.Lu.T, np.asarray(xi, dtype=np.float64)).astype(self.dtype)
        return (self.Zv @ u + self.ssig[:, None] * np.asarray(eps, dtype=np.float64).astype(self.dtype)).astype(self.dtype)


def estimate_precond(kernel, x, zp, diag, s, delta, eps, xi, tol, maxiter, jitter=1e-4, dtype=np.float64, grad=False):
    """cg_precond_ref.estimate with D"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    dgv = sigma2(diag, s, dtype).astype(dtype)
    ny = Nystrom(kernel, x, zp, dgv.astype(np.float64), jitter, dtype)
    eps = np.asarray(eps, dtype=np.float64).reshape(N, -1)
    T = eps.shape[1]
    K, D2, il = _chain(kernel, x, dtype)
    cols = [np.asarray(delta, dtype=np.float64).astype(dtype)[:, None]]
    if T:
        cols.append(ny.probes(eps, xi))
    B = np.column_stack(cols).astype(dtype)
    X, iters, rel, ca, cb, rho0 = pr.pmbcg(lambda P: K @ P + dgv[:, None] * P, ny.apply, B, tol, maxiter, dtype)
    quad = float(_dot(B[:, :1], X[:, :1])[0])
    logdet = float("nan")
    if T:
        logdet = ny.logdet + sum(rho0[t] * cr.lanczos_quad(ca[t], cb[t]) for t in range(1, T + 1) if ca[t]) / T
    out = {"quad": quad, "logdet": logdet, "lml": -0.5 * (quad + logdet + N * math.log(2 * math.pi)), "alpha": X[:, 0], "iters": iters,
           "rel": rel, "logdet_p": ny.logdet}
    if grad:
        P = B.copy()
        P[:, 0] = X[:, 0]
        if T:
            P[:, 1:] = ny.apply(B[:, 1:])
        out["grad"] = _gradient(kernel, K, D2, il, dgv, X, P, T, dtype)
    return out


def predict(kernel, x, sig2, delta, xs, mean_const=0.0):
    """the dense posterior's latent mean and variance at xs"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    xs = o._as_dn(np.asarray(xs, dtype=np.float64))
    Kh = khat(kernel, x, sig2)
    Ks = o.kernelmatrix(kernel, x, xs)
    return mean_const + Ks.T @ np.linalg.solve(Kh, delta), kernel.variance - np.einsum("ij,ij->j", Ks, np.linalg.solve(Kh, Ks))


def sample_rhs(delta, phi_w, eps, sig2, dtype=np.float64):
    """B_s = delta - Phi(X) w_s - sigma_i eps_si, formed in float64 and rounded once; eps (S, N), phi_w (N, S) or None -> (N, S)"""
    d64 = np.asarray(delta, dtype=np.float64).astype(dtype).astype(np.float64)
    e64 = np.asarray(eps).astype(dtype).astype(np.float64).T
    ph = 0.0 if phi_w is None else np.asarray(phi_w).astype(dtype).astype(np.float64)
    return ((d64[:, None] - ph) - np.sqrt(np.asarray(sig2, dtype=np.float64))[:, None] * e64).astype(dtype)
