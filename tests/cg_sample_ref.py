"""Float64 numpy restatement of the pathwise function samples of the exact GP (svgp_cg_sampler_*; csrc/cg_sample.hip) with dense solves:

    f_s(x) = mean_const + sum_l phi_l(x) w_sl + sum_j k(x, X_j) V_js,      V_s = Khat^-1 (delta - Phi(X) w_s - sigma eps_s)
    d f_s / d x_c = invl_c [ - sum_l sin(phase_l) omega_lc amp w_sl + 2 sum_j g(r_j^2) (xs_c - Xs_jc) V_js ]
    phi_l(x) = amp cos(phase_l),  phase_l = omega_l . xs + tau_l,  xs = invl o x,  amp = sqrt(2 variance / L),  Khat = K(X, X) + sigma^2 I

with difference-form distances in float64.  evaluate / gradient take V as an argument, so the data-sized stage can be checked given
whatever V the device holds; with f32=True they run that stage as a float32 chain in the style of cg_ref.kmv_f32 (every array rounded
once, expansion-form r^2 clamped at 0, float32 kappa and 2 g, float32 phase and cosine, float32 products and sums).  Each also returns
the per-point sum of the absolute values of its terms, the scale of the suite's matvec bound."""
import numpy as np

import cg_ref as cr
import svgp_oracle as o


def amplitude(kernel, L):
    return np.sqrt(2.0 * kernel.variance / L) if L > 0 else 0.0


def _phase(kernel, x, omega, tau, dt):
    xs = x.astype(dt) * kernel.inv_lengthscale.astype(dt)[:, None]
    return xs.T @ np.asarray(omega, dtype=dt).reshape(-1, x.shape[0]).T + np.asarray(tau, dtype=dt)[None, :]   # (n, L)


def sigma_of(diag, dtype=np.float64):
    """sqrt of the noise variance as the device holds it (rounded to the data dtype first)"""
    return float(np.sqrt(np.float64(np.dtype(dtype).type(diag))))


def rhs(kernel, x, diag, delta, omega, tau, w, eps, dtype=np.float64):
    """B (N, S) = delta - Phi(X) w_s - sigma eps_s in float64"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, N)
    S = eps.shape[0]
    w = np.asarray(w, dtype=np.float64).reshape(S, -1)
    L = w.shape[1]
    B = np.asarray(delta, dtype=np.float64)[:, None] - sigma_of(diag, dtype) * eps.T
    if L > 0:
        B = B - amplitude(kernel, L) * (np.cos(_phase(kernel, x, omega, tau, np.float64)) @ w.T)
    return B


def solve(kernel, x, diag, B):
    """V = Khat^-1 B by a dense float64 solve -> (V, Khat)"""
    Kh = cr.khat(kernel, x, diag)
    return np.linalg.solve(Kh, B), Kh


def _tile(kernel, X, xs, dt):
    """K(xs, X) (n, N), 2 g (n, N) and the scaled coordinate differences (d, n, N) in dt: float64 by differences, float32 by the expansion"""
    il = kernel.inv_lengthscale.astype(dt)
    Xs, ps = X.astype(dt) * il[:, None], xs.astype(dt) * il[:, None]
    diff = ps[:, :, None] - Xs[:, None, :]
    if dt == np.float64:
        r2 = (diff * diff).sum(0)
    else:
        r2 = (ps * ps).sum(0)[:, None] + (Xs * Xs).sum(0)[None, :] - dt(2) * (ps.T @ Xs)
        r2 = np.maximum(r2, dt(0)).astype(dt)
    K, g2 = cr._kappa(kernel.family, r2, kernel.variance)
    return K.astype(dt), g2.astype(dt), diff


def evaluate(kernel, X, V, xs, omega, tau, w, mean_const=0.0, f32=False):
    """-> (F (S, n), A (S, n)): F[s, j] = f_s(xs_j) given V (N, S); A the sum of |terms|"""
    dt = np.float32 if f32 else np.float64
    X, xs = o._as_dn(np.asarray(X)), o._as_dn(np.asarray(xs))
    V = np.asarray(V).astype(dt)
    S = V.shape[1]
    w = np.asarray(w, dtype=np.float64).reshape(S, -1)
    L = w.shape[1]
    K, _, _ = _tile(kernel, X, xs, dt)
    F = (K @ V).T
    A = (np.abs(K).astype(np.float64) @ np.abs(V).astype(np.float64)).T + abs(mean_const)
    if L > 0:
        wa = (amplitude(kernel, L) * w).astype(dt)
        C = np.cos(_phase(kernel, xs, omega, tau, dt))
        F = F + (C @ wa.T).T
        A = A + (np.abs(C).astype(np.float64) @ np.abs(wa).astype(np.float64).T).T
    F = (dt(mean_const) + F).astype(dt)
    return F, A


def gradient(kernel, X, V, xs, omega, tau, w, f32=False):
    """-> (G (S, d, n), A (S, d, n)): G[s, c, j] = d f_s / d x_c at xs_j given V; A the sum of |terms|"""
    dt = np.float32 if f32 else np.float64
    X, xs = o._as_dn(np.asarray(X)), o._as_dn(np.asarray(xs))
    V = np.asarray(V).astype(dt)
    S = V.shape[1]
    w = np.asarray(w, dtype=np.float64).reshape(S, -1)
    L = w.shape[1]
    d, n = xs.shape
    il = kernel.inv_lengthscale.astype(dt)
    _, g2, diff = _tile(kernel, X, xs, dt)
    G, A = np.zeros((S, d, n), dtype=dt), np.zeros((S, d, n))
    aV = np.abs(V).astype(np.float64)
    for c in range(d):
        T = (g2 * diff[c]).astype(dt)
        G[:, c, :] = (T @ V).T
        A[:, c, :] = (np.abs(T).astype(np.float64) @ aV).T
    if L > 0:
        om = np.asarray(omega, dtype=dt).reshape(L, d)
        ms = -np.sin(_phase(kernel, xs, omega, tau, dt))
        wa = (amplitude(kernel, L) * w).astype(dt)
        for c in range(d):
            Wc = (wa * om[:, c][None, :]).astype(dt)
            G[:, c, :] += (ms @ Wc.T).T
            A[:, c, :] += (np.abs(ms).astype(np.float64) @ np.abs(Wc).astype(np.float64).T).T
    G = (G * il[None, :, None]).astype(dt)
    A = A * np.abs(il.astype(np.float64))[None, :, None]
    return G, A


def sample(kernel, X, diag, delta, xs, omega, tau, w, eps, mean_const=0.0):
    """the whole restatement in float64 -> (F (S, n), G (S, d, n), V (N, S))"""
    V, _ = solve(kernel, X, diag, rhs(kernel, X, diag, delta, omega, tau, w, eps))
    return evaluate(kernel, X, V, xs, omega, tau, w, mean_const)[0], gradient(kernel, X, V, xs, omega, tau, w)[0], V


def posterior_moments(kernel, X, diag, delta, xs, mean_const=0.0):
    """exact posterior mean (n,) and covariance (n, n) of f at xs"""
    X, xs = o._as_dn(np.asarray(X, dtype=np.float64)), o._as_dn(np.asarray(xs, dtype=np.float64))
    Kh = cr.khat(kernel, X, diag)
    Ks = o.kernelmatrix(kernel, X, xs)
    return mean_const + Ks.T @ np.linalg.solve(Kh, delta), o.kernelmatrix(kernel, xs) - Ks.T @ np.linalg.solve(Kh, Ks)
