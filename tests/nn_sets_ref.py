"""The NearestNeighbors (Vecchia) restatement of tests/nn_ref.py with the conditioning sets given as a table, in float64 numpy on top
of svgp_oracle's kernel matrix.

`table` is (n, kb) integers, kb = min(k, n - 1): row i lists the points that point i is conditioned on, the valid entries first (each
in [0, i), distinct), -1 after them.  window_table(n, k) writes the reference's rule out (the m = min(i, k) points before i), with
which every function here is nn_ref's; nearest_table is the brute-force search the device is compared with: the min(i, kb)
points j < i with the smallest sum_f ((x_j,f - x_i,f) il_f)^2, evaluated from differences in `dtype`, ties to the lower index, rows
in ascending index.

fit returns the dict nn_ref.fit returns (dense B, F, U, alpha, ...), so nn_ref.predict serves both.  two_kl is twice the KL
divergence from the exact GP N(0, K + diag I) to its Vecchia approximation: sum_i log F_i - log det(K + diag I)."""
import numpy as np

import nn_ref as nr
import svgp_oracle as o

LOG2PI = nr.LOG2PI


def window_table(n, k):
    kb = min(k, n - 1)
    t = np.full((n, kb), -1, dtype=np.int32)
    for i in range(n):
        m = min(i, kb)
        t[i, :m] = np.arange(i - m, i)
    return t


def search_dist2(x, i, il, dtype=np.float64):
    """(i,) squared distances of the points before i to point i, as the search defines them"""
    x = nr._dn(x).astype(dtype)
    il = np.asarray(il, dtype=np.float64).astype(dtype)
    r2 = np.zeros(i, dtype=dtype)
    for f in range(x.shape[0]):
        df = ((x[f, :i] - x[f, i]) * il[f]).astype(dtype)
        r2 = (r2 + df * df).astype(dtype)
    return r2


def nearest_table(x, k, il=None, dtype=np.float64):
    x = nr._dn(x)
    d, n = x.shape
    il = np.ones(d) if il is None else np.broadcast_to(np.asarray(il, dtype=np.float64), (d,))
    kb = min(k, n - 1)
    t = np.full((n, kb), -1, dtype=np.int32)
    for i in range(n):
        m = min(i, kb)
        if m == 0:
            continue
        order = np.argsort(search_dist2(x, i, il, dtype), kind="stable")   # stable: ties to the lower index
        t[i, :m] = np.sort(order[:m])
    return t


def row(table, i):
    r = np.asarray(table[i])
    return r[r >= 0].astype(np.int64)


def factors(kernel, x, table, diag=0.0, dtype=np.float64):
    """-> (B dense n x n strictly lower, F (n,)): one solve per point over its row of the table"""
    x = nr._dn(x).astype(dtype)
    n = x.shape[1]
    B = np.zeros((n, n), dtype=dtype)
    F = np.zeros(n, dtype=dtype)
    for i in range(n):
        ns = row(table, i)
        kd = dtype(kernel.variance) + dtype(diag)
        if len(ns) == 0:
            F[i] = kd
            continue
        pts = x[:, ns]
        C = o.kernelmatrix(kernel, pts).astype(dtype) + dtype(diag) * np.eye(len(ns), dtype=dtype)
        c = o.kernelmatrix(kernel, pts, x[:, i:i + 1]).astype(dtype)[:, 0]
        b = np.linalg.solve(C, c)
        B[i, ns] = b
        F[i] = kd - c @ b
    return B, F


def table_factors(B, table):
    """dense B -> (n, kb): out[i, t] = B[i, table[i, t]], 0 where the entry is -1"""
    table = np.asarray(table)
    out = np.zeros(table.shape, dtype=B.dtype)
    for i in range(table.shape[0]):
        for t in range(table.shape[1]):
            if table[i, t] >= 0:
                out[i, t] = B[i, table[i, t]]
    return out


def fit(kernel, x, y, table, diag=0.0, mean_const=0.0, dtype=np.float64):
    B, F = factors(kernel, x, table, diag, dtype)
    n = B.shape[0]
    U = (np.eye(n, dtype=dtype) - B).T / np.sqrt(F)[None, :]
    delta = (np.asarray(y, dtype=dtype) - dtype(mean_const))
    alpha = U @ (U.T @ delta)
    logdet = -2.0 * np.sum(np.log(np.diag(U)))
    lml = -(logdet + n * dtype(LOG2PI) + alpha @ delta) / 2
    return dict(B=B, F=F, U=U, alpha=alpha, delta=delta, lml=float(lml), mean_const=float(mean_const))


def lml(kernel, x, y, table, diag=0.0, mean_const=0.0, dtype=np.float64):
    return fit(kernel, x, y, table, diag, mean_const, dtype)["lml"]


predict = nr.predict


def lml_grad(kernel, x, y, table, diag=0.0, mean_const=0.0):
    """-> (lml, d / d variance, d / d inv_lengthscale (d,), d / d diag) at the fixed table: nn_ref.lml_grad over the rows"""
    x = nr._dn(x).astype(np.float64)
    d, n = x.shape
    il, var = kernel.inv_lengthscale, kernel.variance
    delta = np.asarray(y, dtype=np.float64) - mean_const
    val, gvar, gdiag, gil = 0.0, 0.0, 0.0, np.zeros(d)
    for i in range(n):
        ns = row(table, i)
        m = len(ns)
        kd = var + diag
        if m == 0:
            F, r = kd, delta[i]
            gF = -0.5 / F + 0.5 * r * r / (F * F)
            val += LOG2PI + np.log(F) + r * r / F
            gvar += gF
            gdiag += gF
            continue
        idx = np.concatenate([ns, [i]])
        pts = x[:, idx]
        Kall = o.kernelmatrix(kernel, pts)
        C, c = Kall[:m, :m] + diag * np.eye(m), Kall[:m, m]
        b, w = np.linalg.solve(C, c), np.linalg.solve(C, delta[ns])
        F, r = kd - c @ b, delta[i] - b @ delta[ns]
        val += LOG2PI + np.log(F) + r * r / F
        gF = -0.5 / F + 0.5 * r * r / (F * F)
        Cbar = gF * np.outer(b, b) - (r / F) * 0.5 * (np.outer(w, b) + np.outer(b, w))
        cbar = -2.0 * gF * b + (r / F) * w
        Kbar = np.zeros((m + 1, m + 1))
        Kbar[:m, :m] = Cbar
        Kbar[:m, m] = cbar
        Kbar[m, m] = gF
        gvar += np.sum(Kbar * Kall) / var
        gdiag += gF + np.trace(Cbar)
        diff = pts[:, :, None] - pts[:, None, :]
        r2 = np.einsum("f,fab->ab", il ** 2, diff ** 2)
        G = Kbar * var * nr._dkappa(kernel, r2)
        gil += 2.0 * il * np.einsum("ab,fab->f", G, diff ** 2)
    return -0.5 * val, gvar, gil, gdiag


def sum_log_f(kernel, x, table, diag):
    return float(np.sum(np.log(factors(kernel, x, table, diag)[1])))


def logdet_exact(kernel, x, diag):
    x = nr._dn(x).astype(np.float64)
    return float(np.linalg.slogdet(o.kernelmatrix(kernel, x) + diag * np.eye(x.shape[1]))[1])


def two_kl(kernel, x, table, diag):
    return sum_log_f(kernel, x, table, diag) - logdet_exact(kernel, x, diag)


def morton_order(x, bits=16):
    """the permutation that sorts d = 2 points along a Morton (Z-order) curve"""
    x = np.asarray(x)
    q = ((x - x.min(axis=1, keepdims=True)) / np.ptp(x, axis=1, keepdims=True) * (2 ** bits - 1)).astype(np.uint64)
    code = np.zeros(x.shape[1], dtype=np.uint64)
    for b in range(bits):
        for f in range(2):
            code |= ((q[f] >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b + f)
    return np.argsort(code, kind="stable")


def quality_problem(seed, n=600):
    """the problem of the quality claim: n uniform points in [-3, 3]^2 in Morton order"""
    x = np.random.default_rng(seed).uniform(-3.0, 3.0, size=(2, n))
    return x[:, morton_order(x)]


QUALITY = dict(k=10, variance=1.3, inv_lengthscale=(0.9, 0.9), diag=0.05, seeds=(0, 1, 2))
