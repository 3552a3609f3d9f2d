"""Float64 numpy restatement of the input gradient of pathwise posterior function samples (svgp_sampler_eval_grad), on pathwise_ref:

    d f_s / d x_c (x) = invl_c [ - sum_l sin(phase_l) omega_lc (amp w_sl) + 2 sum_i g(r_i^2) (xs_c - zs_ic) V_is ],
    xs = invl o x,  phase_l = omega_l . xs + tau_l,  amp = sqrt(2 variance / L),  r_i^2 = |xs - zs_i|^2,  g = variance dkappa / d(r^2)
    g:  SE -variance e^{-r^2 / 2} / 2;   Matern-3/2 -(3/2) variance e^{-sqrt(3) r};   Matern-5/2 -(5/6) variance (1 + sqrt(5) r) e^{-sqrt(5) r}

(the forms of svgp_oracle._dkappa_dr2: no division by r) with difference-form distances, the difference taken per entry before the
product.  It is the gradient of f_s minus the prior mean: the offsets mux are the caller's, and so is their Jacobian.
gradient(..., f32=True) runs the data-sized stage alone in float32, from the float64 V rounded once, as pathwise_ref.evaluate does."""
import numpy as np

import pathwise_ref as pw
import svgp_oracle as o


def dkappa_dr2(kernel, r2):
    """variance dkappa / d(r^2) in r2's dtype."""
    dt = r2.dtype.type
    var = dt(kernel.variance)
    if kernel.family == o.KERNEL_SE:
        return dt(-0.5) * var * np.exp(dt(-0.5) * r2)
    r = np.sqrt(r2)
    if kernel.family == o.KERNEL_MATERN32:
        return dt(-1.5) * var * np.exp(-dt(np.sqrt(3.0)) * r)
    if kernel.family == o.KERNEL_MATERN52:
        s = dt(np.sqrt(5.0)) * r
        return dt(-5.0 / 6.0) * var * (dt(1) + s) * np.exp(-s)
    raise ValueError("unknown kernel family")


def gradient(sva, st, x, omega, tau, w, f32=False, skip=None):
    """The data-sized stage -> G (S, d, n): G[s, c, j] = d f_s / d x_c at x_j.  f32: every array rounded once to float32 (V from its
    float64 values) and every operation of the stage in float32.  skip: an inducing point whose term is left out of the sum."""
    dt = np.float32 if f32 else np.float64
    x = o._as_dn(np.asarray(x)).astype(dt)
    z = sva.z.astype(dt)
    V = st["V"].astype(dt)                       # (M, S)
    S = V.shape[1]
    w = np.asarray(w, dtype=np.float64).reshape(S, -1)
    L = w.shape[1]
    d, n = x.shape
    il = sva.kernel.inv_lengthscale.astype(dt)
    diff = (x[:, :, None] - z[:, None, :]) * il[:, None, None]          # (d, n, M): (x_c - z_ic) invl_c
    r2 = np.zeros((n, z.shape[1]), dtype=dt)
    for c in range(d):
        r2 += diff[c] * diff[c]
    g2 = dt(2) * dkappa_dr2(sva.kernel, r2)                              # (n, M)
    if skip is not None:
        g2[:, skip] = 0
    G = np.zeros((S, d, n), dtype=dt)
    for c in range(d):
        G[:, c, :] = ((g2 * diff[c]) @ V).T
    if L > 0:
        om = np.asarray(omega, dtype=dt)
        xs = x * il[:, None]
        phase = xs.T @ om.T + np.asarray(tau, dtype=dt)[None, :]         # (n, L)
        ms = -np.sin(phase)
        wa = (pw.amplitude(sva.kernel, L) * w).astype(dt)                # (S, L)
        for c in range(d):
            G[:, c, :] += (ms @ (wa * om[:, c][None, :]).T).T
    G *= il[None, :, None]
    assert G.dtype == dt
    return G


def central_differences(f, x, c, h):
    """(f(x + h e_c) - f(x - h e_c)) / (2 h) for f: (d, n) -> (..., n)."""
    xp, xm = np.array(x, dtype=np.float64), np.array(x, dtype=np.float64)
    xp[c] += h
    xm[c] -= h
    return (f(xp) - f(xm)) / (2.0 * h)
