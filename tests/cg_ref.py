"""Float64 numpy restatement of the exact GP by conjugate gradients (csrc/cg.hip, cg_api.hip; svgp_cg_*), used by the CPU and the GPU
tests: the dense Khat through svgp_oracle.kernelmatrix, the same batched CG recurrence with per-column stopping, the Lanczos
quadrature through numpy.linalg.eigh, the dense-solve forms of the estimator and of its gradient, and a float32 chain of the kmv
product (expansion-form r^2, float32 kappa, float32 accumulation) with which the whole restatement also runs in float32."""
import math

import numpy as np

import svgp_oracle as o

_S3, _S5 = math.sqrt(3.0), math.sqrt(5.0)


def khat(kernel, x, diag):
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    return o.kernelmatrix(kernel, x) + diag * np.eye(x.shape[1])


def _kappa(family, r2, var):
    """kappa and 2 g = 2 d kappa / d r^2 in r2's dtype"""
    t = r2.dtype.type
    if family == o.KERNEL_SE:
        k = t(var) * np.exp(t(-0.5) * r2)
        return k, -k
    r = np.sqrt(r2)
    if family == o.KERNEL_MATERN32:
        e = np.exp(-t(_S3) * r)
        return t(var) * (t(1) + t(_S3) * r) * e, t(-3.0 * var) * e
    e = np.exp(-t(_S5) * r)
    return t(var) * (t(1) + t(_S5) * r + t(5.0 / 3.0) * r2) * e, t(-5.0 / 3.0 * var) * (t(1) + t(_S5) * r) * e


def kernel_chain(kernel, x, dtype=np.float32, xt=None):
    """K(xt, x) (xt None: x) and the list of 2 g (xs_ic - xs_jc)^2 per coordinate, every operation in `dtype`: r^2 in the expansion
    form |xs_i|^2 + |xs_j|^2 - 2 xs_i . xs_j clamped at 0, kappa in dtype, the coordinate difference per entry"""
    x = o._as_dn(np.asarray(x)).astype(dtype)
    p = x if xt is None else o._as_dn(np.asarray(xt)).astype(dtype)
    il = kernel.inv_lengthscale.astype(dtype)
    xs, ps = x * il[:, None], p * il[:, None]
    r2 = (ps * ps).sum(0)[:, None] + (xs * xs).sum(0)[None, :] - dtype(2) * (ps.T @ xs)
    r2 = np.maximum(r2, dtype(0)).astype(dtype)
    K, g2 = _kappa(kernel.family, r2, kernel.variance)
    D = [(g2 * (ps[c][:, None] - xs[c][None, :]) ** 2).astype(dtype) for c in range(x.shape[0])]
    return K.astype(dtype), D


def kmv_f32(kernel, x, V, diag=0.0):
    """the float32 chain of Khat V: float32 tile, float32 accumulation (numpy's float32 product)"""
    K, _ = kernel_chain(kernel, x, np.float32)
    V = np.asarray(V, dtype=np.float32)
    return K @ V + np.float32(diag) * V


def dense_dk(kernel, x):
    """float64, by differences: K, dK / d variance, [dK / d inv_lengthscale_c]"""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    il = kernel.inv_lengthscale
    xs = x * il[:, None]
    r2 = o._scaled_sqdist(kernel, x, x)
    K, g2 = _kappa(kernel.family, r2, kernel.variance)
    return K, K / kernel.variance, [g2 * (xs[c][:, None] - xs[c][None, :]) ** 2 / il[c] for c in range(x.shape[0])]


def mbcg(matvec, B, tol, maxiter, dtype=np.float64):
    """Batched CG on the columns of B with the device's recurrence: vectors in `dtype`, dots and scalars in float64, a column frozen once
    |r| <= tol |b|.  -> X, iterations, relative residuals, per-column lists of the step lengths a and residual ratios b, |b|^2"""
    B = np.asarray(B, dtype=dtype)
    if B.ndim == 1:
        B = B[:, None]
    N, S = B.shape
    dot = lambda u, v: np.einsum("is,is->s", u.astype(np.float64), v.astype(np.float64))
    X, R, P = np.zeros((N, S), dtype=dtype), B.copy(), B.copy()
    bb = dot(B, B)
    rr = bb.copy()
    act = bb > 0
    iters = np.zeros(S, dtype=np.int64)
    ca, cb = [[] for _ in range(S)], [[] for _ in range(S)]
    k = 0
    while act.any() and k < maxiter:
        Q = np.asarray(matvec(P), dtype=dtype)
        pq = dot(P, Q)
        if np.any(~(pq[act] > 0)):
            raise np.linalg.LinAlgError("a curvature p' Khat p is not positive")
        a = np.where(act, rr / np.where(act, pq, 1.0), 0.0)
        X[:, act] = X[:, act] + a[act].astype(dtype) * P[:, act]
        R[:, act] = R[:, act] - a[act].astype(dtype) * Q[:, act]
        rn = dot(R, R)
        be = np.where(act, rn / np.where(act, rr, 1.0), 0.0)
        for s in np.flatnonzero(act):
            ca[s].append(a[s])
            cb[s].append(be[s])
        rr = np.where(act, rn, rr)
        iters[act] = k + 1
        act = act & ~(rr <= tol * tol * bb)
        P[:, act] = R[:, act] + be[act].astype(dtype) * P[:, act]
        k += 1
    rel = np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, 1.0)), 0.0)
    return X, iters, rel, ca, cb, bb


def lanczos_matrix(a, b):
    m = len(a)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    T = np.zeros((m, m))
    for j in range(m):
        T[j, j] = 1.0 / a[j] + (b[j - 1] / a[j - 1] if j else 0.0)
        if j + 1 < m:
            T[j, j + 1] = T[j + 1, j] = math.sqrt(b[j]) / a[j]
    return T


def lanczos_quad(a, b):
    """e_1' log(T) e_1 through numpy.linalg.eigh"""
    lam, Q = np.linalg.eigh(lanczos_matrix(a, b))
    return float(np.sum(Q[0] ** 2 * np.log(lam)))


def _combine(v, T):
    return 0.5 * v[0] - v[1:].sum() / (2.0 * T)


def estimate(kernel, x, diag, delta, probes, tol, maxiter, dtype=np.float64, grad=False):
    """The device's computation restated: one batched solve of [delta, z_1 .. z_T], quad, the quadrature of log det, lml and (grad) the
    gradient {variance, inv_lengthscale, diag, mean_const}.  dtype float32: the kernel chain of kernel_chain in float32."""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    probes = np.asarray(probes, dtype=np.float64).reshape(N, -1)
    T = probes.shape[1]
    if dtype == np.float64:
        K, dKv, dKil = dense_dk(kernel, x)
        il = kernel.inv_lengthscale
        D2 = [dKil[c] * il[c] for c in range(len(il))]
    else:
        K, D2 = kernel_chain(kernel, x, dtype)
        il = kernel.inv_lengthscale.astype(dtype).astype(np.float64)
    dg = dtype(diag)
    B = np.column_stack([np.asarray(delta, dtype=np.float64), probes]).astype(dtype)
    X, iters, rel, ca, cb, bb = mbcg(lambda P: K @ P + dg * P, B, tol, maxiter, dtype)
    dot = lambda u, v: np.einsum("is,is->s", u.astype(np.float64), v.astype(np.float64))
    quad = float(dot(B[:, :1], X[:, :1])[0])
    logdet = sum(bb[t] * lanczos_quad(ca[t], cb[t]) for t in range(1, T + 1) if ca[t]) / T if T else float("nan")
    out = {"quad": quad, "logdet": logdet, "lml": -0.5 * (quad + logdet + N * math.log(2 * math.pi)), "alpha": X[:, 0], "W": X[:, 1:],
           "iters": iters, "rel": rel, "coef": (ca, cb), "bb": bb}
    if grad:
        P = B.copy()
        P[:, 0] = X[:, 0]
        up = dot(X, P)
        KP = np.asarray(K @ P + dg * P, dtype=dtype)
        out["grad"] = {
            "diag": _combine(up, T),
            "variance": _combine(dot(X, KP) - diag * up, T) / kernel.variance,
            "inv_lengthscale": np.array([_combine(dot(X, np.asarray(D2[c] @ P, dtype=dtype)), T) / il[c] for c in range(len(D2))]),
            "mean_const": float(X[:, 0].astype(np.float64).sum()),
        }
    return out


def dense_estimate(kernel, x, diag, delta, probes):
    """The estimator and its gradient with dense float64 solves in place of CG and the exact quadratic form z' log(Khat) z in place of
    the quadrature: what the iteration converges to."""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    probes = np.asarray(probes, dtype=np.float64).reshape(N, -1)
    T = probes.shape[1]
    K, dKv, dKil = dense_dk(kernel, x)
    Kh = K + diag * np.eye(N)
    lam, Q = np.linalg.eigh(Kh)
    alpha = np.linalg.solve(Kh, delta)
    W = np.linalg.solve(Kh, probes)
    quad = float(delta @ alpha)
    logdet = float(np.sum((Q.T @ probes) ** 2 * np.log(lam)[:, None]) / T)
    term = lambda dK: 0.5 * alpha @ dK @ alpha - np.einsum("it,ij,jt->", W, dK, probes) / (2.0 * T)
    return {"quad": quad, "logdet": logdet, "lml": -0.5 * (quad + logdet + N * math.log(2 * math.pi)), "alpha": alpha,
            "grad": {"diag": term(np.eye(N)), "variance": term(dKv), "inv_lengthscale": np.array([term(d) for d in dKil]),
                     "mean_const": float(alpha.sum())}}


def unit_probes(N):
    """sqrt(N) e_t, t = 1 .. N: E z z' = I exactly, so the estimator is the exact log det and trace"""
    return math.sqrt(N) * np.eye(N)


def predict(kernel, x, diag, delta, xs, mean_const=0.0):
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    xs = o._as_dn(np.asarray(xs, dtype=np.float64))
    Kh = khat(kernel, x, diag)
    Ks = o.kernelmatrix(kernel, x, xs)
    return mean_const + Ks.T @ np.linalg.solve(Kh, delta), kernel.variance - np.einsum("ij,ij->j", Ks, np.linalg.solve(Kh, Ks))
