"""Float64 numpy restatement of the input gradient of the exact GP by conjugate gradients (csrc/cg_xgrad.hip; svgp_cg_lml_grad_inputs),
used by the CPU and the GPU tests: with alpha, w_t of the batched solve (cg_ref.estimate, cg_precond_ref.pmbcg) and p_t = z_t or
P^-1 z_t,
    x_bar[c, i] = il_c^2 sum_j 2 g(r_ij^2) (x_ic - x_jc) [ alpha_i alpha_j - (1 / 2T) sum_t (w_it p_jt + w_jt p_it) ]
the same trace estimator as the hyperparameter blocks.  dtype float32: 2 g from cg_ref.kernel_chain's float32 chain, the scaled
coordinate difference per entry and the product with the right panel in float32."""
import numpy as np

import cg_precond_ref as pr
import cg_ref as cr
import svgp_oracle as o


def x_bar(kernel, x, alpha, W, P, dtype=np.float64):
    """(d, N) from alpha (N,), W = [w_t] (N, T), P = [p_t] (N, T), T >= 1"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    d, N = x.shape
    alpha, W, P = (np.asarray(a, dtype=np.float64) for a in (alpha, W, P))
    T = W.shape[1]
    Lp = np.column_stack([alpha, W, P])
    Rp = np.column_stack([alpha, -P / (2.0 * T), -W / (2.0 * T)])
    if dtype == np.float64:
        il = kernel.inv_lengthscale
        xs = x * il[:, None]
        _, g2 = cr._kappa(kernel.family, o._scaled_sqdist(kernel, x, x), kernel.variance)
    else:
        il = kernel.inv_lengthscale.astype(dtype)
        xs = x.astype(dtype) * il[:, None]
        r2 = (xs * xs).sum(0)[:, None] + (xs * xs).sum(0)[None, :] - dtype(2) * (xs.T @ xs)
        r2 = np.maximum(r2, dtype(0)).astype(dtype)
        np.fill_diagonal(r2, dtype(0))
        _, g2 = cr._kappa(kernel.family, r2, kernel.variance)
        Rp = Rp.astype(dtype)
    out = np.zeros((d, N))
    for c in range(d):
        G = (g2 * (xs[c][:, None] - xs[c][None, :])).astype(dtype)   # (2 g dc)_ij
        out[c] = float(il[c]) * np.einsum("is,is->i", Lp, (G @ Rp).astype(np.float64))
    return out


def estimate(kernel, x, diag, delta, probes, tol, maxiter, dtype=np.float64):
    """cg_ref.estimate with its gradient, and grad["x"]"""
    r = cr.estimate(kernel, x, diag, delta, probes, tol, maxiter, dtype=dtype, grad=True)
    N = r["alpha"].shape[0]
    Z = np.asarray(probes, dtype=np.float64).reshape(N, -1).astype(dtype)
    r["grad"]["x"] = x_bar(kernel, x, r["alpha"], r["W"], Z, dtype)
    return r


def estimate_precond(kernel, x, zp, diag, delta, eps, xi, tol, maxiter, jitter=1e-4, dtype=np.float64):
    """cg_precond_ref.estimate's solve, and x_bar with p_t = P^-1 z_t -> {"alpha", "W", "P", "x", "inv_lengthscale"}"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    ny = pr.Nystrom(kernel, x, zp, diag, jitter, dtype)
    eps = np.asarray(eps, dtype=np.float64).reshape(N, -1)
    T = eps.shape[1]
    if dtype == np.float64:
        K, _, dKil = cr.dense_dk(kernel, x)
        il = kernel.inv_lengthscale
        D2 = [dKil[c] * il[c] for c in range(len(il))]
    else:
        K, D2 = cr.kernel_chain(kernel, x, dtype)
        il = kernel.inv_lengthscale.astype(dtype).astype(np.float64)
    dg = dtype(diag)
    B = np.column_stack([np.asarray(delta, dtype=np.float64).astype(dtype)[:, None], ny.probes(eps, xi)]).astype(dtype)
    X = pr.pmbcg(lambda V: K @ V + dg * V, ny.apply, B, tol, maxiter, dtype)[0]
    P = np.asarray(ny.apply(B[:, 1:]), dtype=dtype)
    dot = lambda u, v: np.einsum("is,is->s", u.astype(np.float64), v.astype(np.float64))
    Pa = np.column_stack([X[:, 0], P]).astype(dtype)
    dil = np.array([cr._combine(dot(X, np.asarray(D2[c] @ Pa, dtype=dtype)), T) / il[c] for c in range(len(D2))])
    return {"alpha": X[:, 0], "W": X[:, 1:], "P": P, "x": x_bar(kernel, x, X[:, 0], X[:, 1:], P, dtype), "inv_lengthscale": dil}


def central_differences(kernel, x, diag, delta, h=1e-5):
    """(d, N) central differences of svgp_oracle.exact_gp_logpdf in every coordinate of every point"""
    x = o._as_dn(np.asarray(x, dtype=np.float64)).copy()
    d, N = x.shape
    out = np.zeros((d, N))
    for c in range(d):
        for i in range(N):
            keep = x[c, i]
            x[c, i] = keep + h
            up = o.exact_gp_logpdf(kernel, x, diag, delta)
            x[c, i] = keep - h
            dn = o.exact_gp_logpdf(kernel, x, diag, delta)
            x[c, i] = keep
            out[c, i] = (up - dn) / (2 * h)
    return out
