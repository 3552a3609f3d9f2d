"""Local (nearest-neighbour kriging) predictions of the NearestNeighbors approximation, restated in float64 numpy on top of
svgp_oracle's kernel matrix, in the style of tests/nn_sets_ref.py.

Every test point x* is conditioned on ns*, its min(k, n) nearest TRAINING points (GpGp `predictions`, GPvecchia, spNNGP):
    C = k(ns*, ns*) + diag I,  c = k(ns*, x*)
    mean(x*) = mean_const + c' C^-1 (y_ns* - mean_const),   var(x*) = k(x*, x*) - c' C^-1 c        (the latent variance: no diag)

query_table is the brute-force search the device is compared with: the points j with the smallest sum_f ((x_j,f - x*_f) il_f)^2,
evaluated from differences in `dtype`, ties to the lower index, rows in ascending index; a distance that is not finite is never
chosen, so such a row comes out short, -1 after its valid entries.  predict_local is one dense solve per test point over its row;
a test point with a coordinate that is not finite gives NaN."""
import numpy as np

import nn_ref as nr
import svgp_oracle as o


def query_dist2(x, xs, q, il, dtype=np.float64):
    """(n,) squared distances of the training points to test point q, as the search defines them"""
    x, xs = nr._dn(x).astype(dtype), nr._dn(xs).astype(dtype)
    il = np.asarray(il, dtype=np.float64).astype(dtype)
    r2 = np.zeros(x.shape[1], dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(x.shape[0]):
            df = ((x[f] - xs[f, q]) * il[f]).astype(dtype)
            r2 = (r2 + df * df).astype(dtype)
    return r2


def query_table(x, xs, k, il=None, dtype=np.float64):
    """(n*, min(k, n)) int32"""
    x, xs = nr._dn(x), nr._dn(xs)
    d, n = x.shape
    il = np.ones(d) if il is None else np.broadcast_to(np.asarray(il, dtype=np.float64), (d,))
    kq = min(k, n)
    t = np.full((xs.shape[1], kq), -1, dtype=np.int32)
    for q in range(xs.shape[1]):
        r2 = query_dist2(x, xs, q, il, dtype)
        order = np.argsort(r2, kind="stable")          # stable: ties to the lower index; NaN sorts last
        order = order[np.isfinite(r2[order])][:kq]
        t[q, :len(order)] = np.sort(order)
    return t


def predict_local(kernel, x, y, xs, table, diag=0.0, mean_const=0.0, dtype=np.float64):
    """-> (mean (n*,), var (n*,)): one solve per test point over row q of the table"""
    x, xs = nr._dn(x).astype(dtype), nr._dn(xs).astype(dtype)
    delta = np.asarray(y, dtype=dtype) - dtype(mean_const)
    ns_ = xs.shape[1]
    mean, var = np.zeros(ns_, dtype=dtype), np.zeros(ns_, dtype=dtype)
    for q in range(ns_):
        if not np.all(np.isfinite(xs[:, q])):
            mean[q] = var[q] = np.nan
            continue
        r = np.asarray(table[q])
        ns = r[r >= 0].astype(np.int64)
        mean[q], var[q] = dtype(mean_const), dtype(kernel.variance)
        if len(ns) == 0:
            continue
        pts = x[:, ns]
        C = o.kernelmatrix(kernel, pts).astype(dtype) + dtype(diag) * np.eye(len(ns), dtype=dtype)
        c = o.kernelmatrix(kernel, pts, xs[:, q:q + 1]).astype(dtype)[:, 0]
        b = np.linalg.solve(C, c)
        mean[q] += b @ delta[ns]
        var[q] -= c @ b
    return mean, var
