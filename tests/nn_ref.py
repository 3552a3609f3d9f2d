"""Reference NearestNeighbors (Vecchia) approximation for the tests, in float64 numpy, on top of svgp_oracle's kernel matrix.

A restatement of the reference's src/NearestNeighborsModule.jl in its own order: make_row (:27-29) is one `solve` per point, make_F
(:46-61) the conditional variance, make_B (:15-21) and approx_root_prec (:90-95) the dense U = (I - B)' F^-1/2, posterior (:97-106)
alpha = U (U' delta), approx_lml (:108-113) = -(logdet(InvRoot(U)) + n log 2 pi + alpha' delta) / 2, and the predictions of
AbstractGPs' PosteriorGP with C = InvRoot(U): V = U' k(x, x*).

`diag` is added to every diagonal entry (0: the reference, which ignores fx.Sigma_y).  `dtype` runs the whole restatement in
another float type (the float32 figure the GPU tolerances rest on).  lml_joint is the second formulation: the joint Cholesky of
each (m + 1) block.  lml_grad is the closed-form gradient:
    gF = -1/(2F) + r^2/(2F^2),  w = C \\ delta_ns:  kd_bar = gF,  c_bar = -2 gF b + (r/F) w,  C_bar = gF b b' - (r/F) sym(w b'),
    d / d diag = gF (1 + b'b) - (r/F) w'b."""
import numpy as np

import svgp_oracle as o

LOG2PI = float(np.log(2.0 * np.pi))


def kernel_of(family, variance, inv_lengthscale):
    return o.Kernel(family, float(variance), np.atleast_1d(np.asarray(inv_lengthscale, dtype=np.float64)))


def _dn(x):
    x = np.asarray(x)
    return x[None, :] if x.ndim == 1 else x


def synth(n, d, seed, dtype=np.float64):
    """x ~ U(-2, 2)^d (d, n), y = sin(sum x) + 0.1 noise"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, size=(d, n))
    y = np.sin(x.sum(axis=0)) + 0.1 * rng.standard_normal(n)
    return x.astype(dtype), y.astype(dtype)


def invl_for(d, ard):
    """inverse lengthscales in [0.8, 1.1]"""
    return np.linspace(0.8, 1.1, d) if (ard and d > 1) else np.full(d, 0.9)


def factors(kernel, x, k, diag=0.0, dtype=np.float64):
    """-> (B dense n x n strictly lower, F (n,)): make_B / make_F with one solve per point"""
    x = _dn(x).astype(dtype)
    n = x.shape[1]
    B = np.zeros((n, n), dtype=dtype)
    F = np.zeros(n, dtype=dtype)
    for i in range(n):
        m = min(i, k)
        kd = dtype(kernel.variance) + dtype(diag)
        if m == 0:
            F[i] = kd
            continue
        ns = x[:, i - m:i]
        C = o.kernelmatrix(kernel, ns).astype(dtype) + dtype(diag) * np.eye(m, dtype=dtype)
        c = o.kernelmatrix(kernel, ns, x[:, i:i + 1]).astype(dtype)[:, 0]
        b = np.linalg.solve(C, c)
        B[i, i - m:i] = b
        F[i] = kd - c @ b
    return B, F


def banded(B, k):
    """dense strictly-lower B -> (n, kb) band, kb = min(k, n - 1): band[i, t] = B[i, i - kb + t]"""
    n = B.shape[0]
    kb = min(k, n - 1)
    out = np.zeros((n, kb), dtype=B.dtype)
    for i in range(n):
        for t in range(kb):
            j = i - kb + t
            if j >= 0:
                out[i, t] = B[i, j]
    return out


def fit(kernel, x, y, k, diag=0.0, mean_const=0.0, dtype=np.float64):
    """-> dict(B, F, U, alpha, delta, lml): posterior(nn, fx, y) and approx_lml through the dense U"""
    B, F = factors(kernel, x, k, diag, dtype)
    n = B.shape[0]
    U = (np.eye(n, dtype=dtype) - B).T / np.sqrt(F)[None, :]
    delta = (np.asarray(y, dtype=dtype) - dtype(mean_const))
    alpha = U @ (U.T @ delta)
    logdet = -2.0 * np.sum(np.log(np.diag(U)))       # logdet(InvRoot(U))
    lml = -(logdet + n * dtype(LOG2PI) + alpha @ delta) / 2
    return dict(B=B, F=F, U=U, alpha=alpha, delta=delta, lml=float(lml), mean_const=float(mean_const))


def lml(kernel, x, y, k, diag=0.0, mean_const=0.0, dtype=np.float64):
    return fit(kernel, x, y, k, diag, mean_const, dtype)["lml"]


def lml_joint(kernel, x, y, k, diag=0.0, mean_const=0.0):
    """the same value from the joint Cholesky of each (m + 1) block: the last row of L^-1 [delta_ns; delta_i] is r_i / sqrt(F_i)"""
    x = _dn(x).astype(np.float64)
    n = x.shape[1]
    delta = np.asarray(y, dtype=np.float64) - mean_const
    s = 0.0
    for i in range(n):
        m = min(i, k)
        pts = x[:, i - m:i + 1]
        L = np.linalg.cholesky(o.kernelmatrix(kernel, pts) + diag * np.eye(m + 1))
        z = np.linalg.solve(L, delta[i - m:i + 1])
        s += LOG2PI + 2.0 * np.log(L[m, m]) + z[m] ** 2
    return -0.5 * s


def exact_lml(kernel, x, y, diag, mean_const=0.0):
    x = _dn(x).astype(np.float64)
    n = x.shape[1]
    K = o.kernelmatrix(kernel, x) + diag * np.eye(n)
    L = np.linalg.cholesky(K)
    z = np.linalg.solve(L, np.asarray(y, dtype=np.float64) - mean_const)
    return float(-0.5 * z @ z - np.sum(np.log(np.diag(L))) - 0.5 * n * LOG2PI)


def exact_predict(kernel, x, y, diag, xs, mean_const=0.0):
    """the exact GP posterior with cov(fx) = K + diag I: (mean, cov) at xs"""
    x, xs = _dn(x).astype(np.float64), _dn(xs).astype(np.float64)
    K = o.kernelmatrix(kernel, x) + diag * np.eye(x.shape[1])
    Ks = o.kernelmatrix(kernel, x, xs)
    mean = mean_const + Ks.T @ np.linalg.solve(K, np.asarray(y, dtype=np.float64) - mean_const)
    cov = o.kernelmatrix(kernel, xs) - Ks.T @ np.linalg.solve(K, Ks)
    return mean, cov


def predict(cache, kernel, x, xs, ys=None):
    """-> (mean, var, cov) at xs; with ys the cross-covariance cov(xs, ys) in place of cov"""
    dt = cache["U"].dtype
    x, xs = _dn(x).astype(dt), _dn(xs).astype(dt)
    Kx = o.kernelmatrix(kernel, x, xs).astype(dt)
    V = cache["U"].T @ Kx
    mean = dt.type(cache["mean_const"]) + Kx.T @ cache["alpha"]
    var = dt.type(kernel.variance) - np.sum(V * V, axis=0)
    if ys is None:
        return mean, var, o.kernelmatrix(kernel, xs).astype(dt) - V.T @ V
    ys = _dn(ys).astype(dt)
    Vy = cache["U"].T @ o.kernelmatrix(kernel, x, ys).astype(dt)
    return mean, var, o.kernelmatrix(kernel, xs, ys).astype(dt) - V.T @ Vy


def _dkappa(kernel, r2):
    """d (unit-variance kernel) / d r2"""
    if kernel.family == o.KERNEL_SE:
        return -0.5 * np.exp(-0.5 * r2)
    if kernel.family == o.KERNEL_MATERN32:
        return -1.5 * np.exp(-np.sqrt(3.0 * r2))
    s = np.sqrt(5.0 * r2)
    return -(5.0 / 6.0) * (1.0 + s) * np.exp(-s)


def lml_grad(kernel, x, y, k, diag=0.0, mean_const=0.0):
    """-> (lml, d / d variance, d / d inv_lengthscale (d,), d / d diag): the closed form, every adjoint contracted entry by entry"""
    x = _dn(x).astype(np.float64)
    d, n = x.shape
    il, var = kernel.inv_lengthscale, kernel.variance
    delta = np.asarray(y, dtype=np.float64) - mean_const
    val, gvar, gdiag, gil = 0.0, 0.0, 0.0, np.zeros(d)
    for i in range(n):
        m = min(i, k)
        kd = var + diag
        if m == 0:
            F, r = kd, delta[i]
            gF = -0.5 / F + 0.5 * r * r / (F * F)
            val += LOG2PI + np.log(F) + r * r / F
            gvar += gF
            gdiag += gF
            continue
        pts = x[:, i - m:i + 1]
        Kall = o.kernelmatrix(kernel, pts)
        C, c = Kall[:m, :m] + diag * np.eye(m), Kall[:m, m]
        b, w = np.linalg.solve(C, c), np.linalg.solve(C, delta[i - m:i])
        F, r = kd - c @ b, delta[i] - b @ delta[i - m:i]
        val += LOG2PI + np.log(F) + r * r / F
        gF = -0.5 / F + 0.5 * r * r / (F * F)
        Cbar = gF * np.outer(b, b) - (r / F) * 0.5 * (np.outer(w, b) + np.outer(b, w))
        cbar = -2.0 * gF * b + (r / F) * w
        # adjoint of the (m + 1) x (m + 1) kernel block: C_bar, c_bar once (c appears once in F and r), kd_bar
        Kbar = np.zeros((m + 1, m + 1))
        Kbar[:m, :m] = Cbar
        Kbar[:m, m] = cbar
        Kbar[m, m] = gF
        gvar += np.sum(Kbar * Kall) / var
        gdiag += gF + np.trace(Cbar)
        diff = pts[:, :, None] - pts[:, None, :]                       # (d, m + 1, m + 1)
        r2 = np.einsum("f,fab->ab", il ** 2, diff ** 2)
        G = Kbar * var * _dkappa(kernel, r2)
        gil += 2.0 * il * np.einsum("ab,fab->f", G, diff ** 2)
    return -0.5 * val, gvar, gil, gdiag
