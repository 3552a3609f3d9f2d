"""The NearestNeighbors (Vecchia) restatement with per-point noise variances and per-point prior-mean offsets, in float64 numpy
on top of tests/nn_ref.py, tests/nn_sets_ref.py and svgp_oracle's kernel matrix (none of them edited).

    sigma_j^2 = diag + s_j,    delta_j = y_j - mean_const - mu_j
per point i over its conditioning set ns(i) (a row of `table`; nn_sets_ref.window_table(n, k) is the window):
    C = k(ns, ns) + diag(sigma^2_ns),  c = k(ns, x_i),  kd = variance + sigma_i^2,  b = C \\ c,  w = C \\ delta_ns
    F = kd - c'b,  r = delta_i - b'delta_ns,  gF = -1/(2F) + r^2/(2F^2),  lml = -1/2 sum_i (log 2 pi + log F_i + r_i^2 / F_i)
    s_bar_j    = d lml / d sigma_j^2 = gF_j + sum_{(i, t): ns(i)_t = j} (gF_i b_it^2 - (r_i / F_i) w_it b_it)
    mean_bar_j = d lml / d mean(x_j) = alpha_j = r_j / F_j - sum_{(i, t): ns(i)_t = j} b_it r_i / F_i
    d_diag = sum_j s_bar_j,   d_mean_const = sum_j mean_bar_j
s = None / mu = None are vectors of zeros, with which every function here is nn_sets_ref's.  `dtype` runs a whole function in another
float type, as nn_ref.factors does (the float32 figures the GPU tolerances of s_bar and mean_bar rest on)."""
import numpy as np

import nn_local_ref as nl
import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o

LOG2PI = nr.LOG2PI


def noise_vector(n, seed):
    """s = exp(U[log 0.02, log 0.5]): the noise of the conjugate-gradient tests"""
    return np.exp(np.random.default_rng(seed).uniform(np.log(0.02), np.log(0.5), n))


def mean_vector(x):
    """a smooth function of x"""
    x = nr._dn(x).astype(np.float64)
    return 0.3 * np.cos(0.7 * x.sum(axis=0)) + 0.05 * x[0]


def hub_table(n, k, hubs, seed):
    """(n, min(k, n - 1)) random table in which every point of `hubs` sits in every later row; every fifth row is short"""
    rng = np.random.default_rng(seed)
    kb = min(k, n - 1)
    t = np.full((n, kb), -1, dtype=np.int32)
    for i in range(1, n):
        m = min(i, kb)
        must = [h for h in hubs if h < i][:m]
        rest = np.setdiff1d(np.arange(i), must)
        extra = rng.choice(rest, size=min(m - len(must), len(rest)), replace=False) if m > len(must) else []
        r = sorted(set(must) | set(int(e) for e in extra))
        if i % 5 == 0:
            r = sorted(set(must) | set(r[:max(1, len(r) // 2)]))
        t[i, :len(r)] = r
    return t


def random_table(n, k, seed):
    """a caller's table: random predecessors in ascending index, every seventh row short"""
    rng = np.random.default_rng(seed)
    kb = min(k, n - 1)
    t = np.full((n, kb), -1, dtype=np.int32)
    for i in range(1, n):
        m = min(i, kb)
        if i % 7 == 0:
            m = max(1, m // 2)
        t[i, :m] = np.sort(rng.choice(i, size=m, replace=False))
    return t


def _vectors(n, diag, s, mu, y, mean_const, dtype):
    s = np.zeros(n) if s is None else np.asarray(s, dtype=np.float64)
    mu = np.zeros(n) if mu is None else np.asarray(mu, dtype=np.float64)
    sig2 = (dtype(diag) + s.astype(dtype)).astype(dtype)
    delta = (np.asarray(y, dtype=dtype) - dtype(mean_const) - mu.astype(dtype)).astype(dtype)
    return sig2, delta


def points(kernel, x, y, table, diag=0.0, s=None, mu=None, mean_const=0.0, dtype=np.float64):
    """-> list over i of dict(ns, b, w, F, r): one pair of solves per point"""
    x = nr._dn(x).astype(dtype)
    n = x.shape[1]
    sig2, delta = _vectors(n, diag, s, mu, y, mean_const, dtype)
    out = []
    for i in range(n):
        idx = ns.row(table, i)
        kd = dtype(kernel.variance) + sig2[i]
        if len(idx) == 0:
            out.append(dict(ns=idx, b=np.zeros(0, dtype), w=np.zeros(0, dtype), F=kd, r=delta[i]))
            continue
        pts = x[:, idx]
        C = o.kernelmatrix(kernel, pts).astype(dtype) + np.diag(sig2[idx])
        c = o.kernelmatrix(kernel, pts, x[:, i:i + 1]).astype(dtype)[:, 0]
        b, w = np.linalg.solve(C, c), np.linalg.solve(C, delta[idx])
        out.append(dict(ns=idx, b=b, w=w, F=kd - c @ b, r=delta[i] - b @ delta[idx]))
    return out


def fit(kernel, x, y, table, diag=0.0, s=None, mu=None, mean_const=0.0, dtype=np.float64):
    """-> the dict of nn_ref.fit (dense B, F, U, alpha, delta, lml, mean_const): nn_ref.predict serves it; a mean function's value at
    x* is the caller's to add"""
    pp = points(kernel, x, y, table, diag, s, mu, mean_const, dtype)
    n = len(pp)
    B = np.zeros((n, n), dtype=dtype)
    F = np.array([p["F"] for p in pp], dtype=dtype)
    for i, p in enumerate(pp):
        B[i, p["ns"]] = p["b"]
    U = (np.eye(n, dtype=dtype) - B).T / np.sqrt(F)[None, :]
    _, delta = _vectors(n, diag, s, mu, y, mean_const, dtype)
    alpha = U @ (U.T @ delta)
    logdet = -2.0 * np.sum(np.log(np.diag(U)))
    lml = -(logdet + n * dtype(LOG2PI) + alpha @ delta) / 2
    return dict(B=B, F=F, U=U, alpha=alpha, delta=delta, lml=float(lml), mean_const=float(mean_const))


def lml(kernel, x, y, table, diag=0.0, s=None, mu=None, mean_const=0.0, dtype=np.float64):
    """the sum over the points, directly"""
    pp = points(kernel, x, y, table, diag, s, mu, mean_const, dtype)
    return float(-0.5 * sum(LOG2PI + np.log(np.float64(p["F"])) + np.float64(p["r"]) ** 2 / np.float64(p["F"]) for p in pp))


def exact_lml(kernel, x, y, diag, s=None, mu=None, mean_const=0.0):
    """the dense exact GP with cov(fx) = K + diag(sigma^2)"""
    x = nr._dn(x).astype(np.float64)
    n = x.shape[1]
    sig2, delta = _vectors(n, diag, s, mu, y, mean_const, np.float64)
    L = np.linalg.cholesky(o.kernelmatrix(kernel, x) + np.diag(sig2))
    z = np.linalg.solve(L, delta)
    return float(-0.5 * z @ z - np.sum(np.log(np.diag(L))) - 0.5 * n * LOG2PI)


def point_grads(kernel, x, y, table, diag=0.0, s=None, mu=None, mean_const=0.0, dtype=np.float64):
    """-> (lml, s_bar (n,), mean_bar (n,)) by the two formulas above; the solves and the per-pair terms in `dtype`, the sums over
    the pairs in float64 (the device's rule)"""
    pp = points(kernel, x, y, table, diag, s, mu, mean_const, dtype)
    n = len(pp)
    s_bar, mean_bar, val = np.zeros(n), np.zeros(n), 0.0
    for i, p in enumerate(pp):
        F, r = np.float64(p["F"]), np.float64(p["r"])
        gF, rF = -0.5 / F + 0.5 * r * r / (F * F), r / F
        val += LOG2PI + np.log(F) + r * r / F
        s_bar[i] += gF
        mean_bar[i] += rF
        if len(p["ns"]):
            b, w = p["b"].astype(np.float64), p["w"].astype(np.float64)
            pair = ((gF * b - rF * w) * b).astype(dtype).astype(np.float64)
            np.add.at(s_bar, p["ns"], pair)
            np.add.at(mean_bar, p["ns"], -b * rF)
    return -0.5 * val, s_bar, mean_bar


def lml_grad(kernel, x, y, table, diag=0.0, s=None, mu=None, mean_const=0.0):
    """-> (lml, d / d variance, d / d inv_lengthscale (d,), d / d diag, d / d mean_const): nn_sets_ref.lml_grad's contraction of the
    block adjoints with the two vectors in place; d / d diag and d / d mean_const are the sums of s_bar and mean_bar"""
    x = nr._dn(x).astype(np.float64)
    d, n = x.shape
    il, var = kernel.inv_lengthscale, kernel.variance
    pp = points(kernel, x, y, table, diag, s, mu, mean_const)
    gvar, gil = 0.0, np.zeros(d)
    for i, p in enumerate(pp):
        F, r, b, w, idx = p["F"], p["r"], p["b"], p["w"], p["ns"]
        m = len(idx)
        gF = -0.5 / F + 0.5 * r * r / (F * F)
        if m == 0:
            gvar += gF
            continue
        pts = x[:, np.concatenate([idx, [i]])]
        Kall = o.kernelmatrix(kernel, pts)
        Kbar = np.zeros((m + 1, m + 1))
        Kbar[:m, :m] = gF * np.outer(b, b) - (r / F) * 0.5 * (np.outer(w, b) + np.outer(b, w))
        Kbar[:m, m] = -2.0 * gF * b + (r / F) * w
        Kbar[m, m] = gF
        gvar += np.sum(Kbar * Kall) / var
        diff = pts[:, :, None] - pts[:, None, :]
        r2 = np.einsum("f,fab->ab", il ** 2, diff ** 2)
        gil += 2.0 * il * np.einsum("ab,fab->f", Kbar * var * nr._dkappa(kernel, r2), diff ** 2)
    val, s_bar, mean_bar = point_grads(kernel, x, y, table, diag, s, mu, mean_const)
    return val, gvar, gil, float(np.sum(s_bar)), float(np.sum(mean_bar))


def predict_local(kernel, x, y, xs, qtable, diag=0.0, s=None, mu=None, mean_const=0.0, dtype=np.float64):
    """nn_local_ref.predict_local conditioned on the two vectors -> (mean, var) = (mean_const + c'C^-1 delta_ns*, variance - c'C^-1 c)"""
    x, xs = nr._dn(x).astype(dtype), nr._dn(xs).astype(dtype)
    sig2, delta = _vectors(x.shape[1], diag, s, mu, y, mean_const, dtype)
    nq = xs.shape[1]
    mean, var = np.full(nq, dtype(mean_const), dtype=dtype), np.full(nq, dtype(kernel.variance), dtype=dtype)
    for q in range(nq):
        idx = ns.row(qtable, q)
        if len(idx) == 0:
            continue
        pts = x[:, idx]
        C = o.kernelmatrix(kernel, pts).astype(dtype) + np.diag(sig2[idx])
        c = o.kernelmatrix(kernel, pts, xs[:, q:q + 1]).astype(dtype)[:, 0]
        b = np.linalg.solve(C, c)
        mean[q] += b @ delta[idx]
        var[q] -= c @ b
    return mean, var


query_table = nl.query_table
