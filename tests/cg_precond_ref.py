"""Numpy restatement of the Nystrom preconditioner of the conjugate gradients (csrc/cg.hip, cg_api.hip; svgp_cg_set_preconditioner,
svgp_cg_precond_*, svgp_cg_fit_precond), in float64 and with float32 vectors as cg_ref.mbcg does it:
  P = Z Kuu^-1 Z' + s2 I,  Z = K(x, z_p),  Kuu = K(z_p, z_p) + jitter variance I = Lu Lu',
  P^-1 r = (r - Z W Z' r) / s2,  W = Lu^-T B^-1 Lu^-1 / s2,  B = I + Lu^-1 (Z'Z) Lu^-T / s2,  log det P = N log s2 + log det B.
The k-sized stage is float64 for both dtypes, the Gram Z'Z accumulated in float64 from float64 entries (the device's rule); with dtype
float32 the two N x k products of an application use float32 entries (cg_ref.kernel_chain) and float32 accumulation."""
import math

import numpy as np

import cg_ref as cr
import svgp_oracle as o


class Nystrom:
    def __init__(self, kernel, x, zp, diag, jitter=1e-4, dtype=np.float64):
        x = o._as_dn(np.asarray(x, dtype=np.float64))
        zp = o._as_dn(np.asarray(zp, dtype=np.float64))
        self.N, self.k, self.dtype = x.shape[1], zp.shape[1], dtype
        self.s2 = float(dtype(diag))
        self.Z = o.kernelmatrix(kernel, x, zp)   # N x k, float64
        Kuu = o.kernelmatrix(kernel, zp, zp) + jitter * kernel.variance * np.eye(self.k)
        self.Lu = np.linalg.cholesky(Kuu)
        self.G = self.Z.T @ self.Z
        A = np.linalg.solve(self.Lu, np.linalg.solve(self.Lu, self.G).T)
        self.B = np.eye(self.k) + 0.5 * (A + A.T) / self.s2
        self.LB = np.linalg.cholesky(self.B)
        Li = np.linalg.inv(self.Lu)
        self.Wu = Li.T @ np.linalg.solve(self.B, Li)   # W s2
        self.logdet = self.N * math.log(self.s2) + 2.0 * float(np.log(np.diag(self.LB)).sum())
        # the entries the two products of an application use
        self.Zv = self.Z if dtype == np.float64 else cr.kernel_chain(kernel, x, dtype, xt=zp)[0].T.copy()

    def dense(self):
        """P, float64"""
        return self.Z @ np.linalg.solve(self.Lu.T, np.linalg.solve(self.Lu, self.Z.T)) + self.s2 * np.eye(self.N)

    def cross(self, V):
        return (self.Zv.T @ np.asarray(V, dtype=self.dtype)).astype(self.dtype)

    def apply(self, R):
        R = np.asarray(R, dtype=self.dtype)
        t = self.cross(R)
        v = (-(self.Wu @ t.astype(np.float64)) / (self.s2 * self.s2)).astype(self.dtype)
        return (self.Zv @ v + self.dtype(1.0 / self.s2) * R).astype(self.dtype)

    def probes(self, eps, xi):
        """z_t = sigma eps_t + Z Lu^-T xi_t"""
        u = np.linalg.solve(self.Lu.T, np.asarray(xi, dtype=np.float64)).astype(self.dtype)
        return (self.Zv @ u + self.dtype(math.sqrt(self.s2)) * np.asarray(eps, dtype=np.float64).astype(self.dtype)).astype(self.dtype)


def pmbcg(matvec, papply, B, tol, maxiter, dtype=np.float64):
    """cg_ref.mbcg with the preconditioned recurrence: z = P^-1 r, rho = r'z, a = rho / p'q, beta = rho_new / rho, p = z + beta p; a column
    is frozen once |r| <= tol |b| (the true residual).  -> X, iterations, relative residuals, lists of a and beta, rho_0 = b' P^-1 b"""
    B = np.asarray(B, dtype=dtype)
    if B.ndim == 1:
        B = B[:, None]
    N, S = B.shape
    dot = lambda u, v: np.einsum("is,is->s", u.astype(np.float64), v.astype(np.float64))
    X, R = np.zeros((N, S), dtype=dtype), B.copy()
    bb = dot(B, B)
    rr = bb.copy()
    act = bb > 0
    Zv = np.asarray(papply(R), dtype=dtype)
    P = Zv.copy()
    rho = dot(R, Zv)
    rho0 = rho.copy()
    iters = np.zeros(S, dtype=np.int64)
    ca, cb = [[] for _ in range(S)], [[] for _ in range(S)]
    k = 0
    while act.any() and k < maxiter:
        Q = np.asarray(matvec(P), dtype=dtype)
        pq = dot(P, Q)
        if np.any(~(pq[act] > 0)):
            raise np.linalg.LinAlgError("a curvature p' Khat p is not positive")
        a = np.where(act, rho / np.where(act, pq, 1.0), 0.0)
        X[:, act] = X[:, act] + a[act].astype(dtype) * P[:, act]
        R[:, act] = R[:, act] - a[act].astype(dtype) * Q[:, act]
        rn = dot(R, R)
        was = act.copy()
        rr = np.where(act, rn, rr)
        iters[act] = k + 1
        act = act & ~(rr <= tol * tol * bb)
        Zv = np.asarray(papply(R), dtype=dtype)
        rz = dot(R, Zv)
        be = np.where(act, rz / np.where(act, rho, 1.0), 0.0)
        for s in np.flatnonzero(was):
            ca[s].append(a[s])
            cb[s].append(be[s])
        rho = np.where(act, rz, rho)
        P[:, act] = Zv[:, act] + be[act].astype(dtype) * P[:, act]
        k += 1
    rel = np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, 1.0)), 0.0)
    return X, iters, rel, ca, cb, rho0


def exact_probes(N, k):
    """eps = sqrt(T) [I_N 0] (N x T), xi = sqrt(T) [0 I_k] (k x T), T = N + k: (1 / T) sum_t z_t z_t' = P exactly"""
    T = N + k
    eps, xi = np.zeros((N, T)), np.zeros((k, T))
    eps[:, :N] = math.sqrt(T) * np.eye(N)
    xi[:, N:] = math.sqrt(T) * np.eye(k)
    return eps, xi


def estimate(kernel, x, zp, diag, delta, eps, xi, tol, maxiter, jitter=1e-4, dtype=np.float64, grad=False):
    """The device's preconditioned computation restated: one batched solve of [delta, z_1 .. z_T], quad, log det Khat = log det P + (1 / T)
    sum_t (z_t' P^-1 z_t) e_1' log(T_t) e_1, lml and (grad) the gradient with the trace terms w_t' dKhat (P^-1 z_t)."""
    x = o._as_dn(np.asarray(x, dtype=np.float64))
    N = x.shape[1]
    ny = Nystrom(kernel, x, zp, diag, jitter, dtype)
    eps = np.asarray(eps, dtype=np.float64).reshape(N, -1)
    T = eps.shape[1]
    if dtype == np.float64:
        K, dKv, dKil = cr.dense_dk(kernel, x)
        il = kernel.inv_lengthscale
        D2 = [dKil[c] * il[c] for c in range(len(il))]
    else:
        K, D2 = cr.kernel_chain(kernel, x, dtype)
        il = kernel.inv_lengthscale.astype(dtype).astype(np.float64)
    dg = dtype(diag)
    cols = [np.asarray(delta, dtype=np.float64).astype(dtype)[:, None]]
    if T:
        cols.append(ny.probes(eps, xi))
    B = np.column_stack(cols).astype(dtype)
    X, iters, rel, ca, cb, rho0 = pmbcg(lambda P: K @ P + dg * P, ny.apply, B, tol, maxiter, dtype)
    dot = lambda u, v: np.einsum("is,is->s", u.astype(np.float64), v.astype(np.float64))
    quad = float(dot(B[:, :1], X[:, :1])[0])
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
        up = dot(X, P)
        KP = np.asarray(K @ P + dg * P, dtype=dtype)
        out["grad"] = {
            "diag": cr._combine(up, T),
            "variance": cr._combine(dot(X, KP) - diag * up, T) / kernel.variance,
            "inv_lengthscale": np.array([cr._combine(dot(X, np.asarray(D2[c] @ P, dtype=dtype)), T) / il[c] for c in range(len(D2))]),
            "mean_const": float(X[:, 0].astype(np.float64).sum()),
        }
    return out
