#!/usr/bin/env python
"""Held-out metrics on the device: the models of examples/a_regression.py and examples/b_classification.py, trained briefly on a
training split, then scored on a held-out split through svgp_predictive - the predictive distribution of the OBSERVATION, not of the
latent f:

  * regression:     test RMSE = sqrt(sum_sq_err / n) and mean NLPD = -sum_lpd / n, both from the call's summary (no per-point transfer);
  * classification: the class-1 probability E[y*] per test point, the mean NLPD of the test labels and the accuracy at p = 1/2.

    python examples/j_heldout_metrics.py      # needs an MI355X
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "approximategps.jl_amd"))
import approxgp as ag  # noqa: E402
from approxgp import _ffi  # noqa: E402


def softplus(v):
    return np.log1p(np.exp(-abs(v))) + max(v, 0.0)


def invsoftplus(v):
    return v + np.log(-np.expm1(-v))


def regression(ctx, steps=150, batch=100, lr=0.01, seed=1234):
    """a_regression.py's model (SE kernel, M = 20, Gaussian noise 0.3), Adam on minibatches of the training split."""
    rng = np.random.default_rng(seed)
    N, M, n_test = 10_000, 20, 2_000
    x = rng.uniform(-1, 1, N)
    y = np.sin(3 * np.pi * x) + 0.3 * np.cos(9 * np.pi * x) + 0.5 * np.sin(7 * np.pi * x) + 0.3 * rng.standard_normal(N)
    n_train = N - n_test
    lik_noise, jitter = 0.3, 1e-5
    theta = {"k": np.array([invsoftplus(1.3), invsoftplus(0.3)]), "z": x[:M].copy(), "m": np.zeros(M), "A": np.eye(M)}
    data = _ffi.DeviceData(ctx, x, y, np.float64)          # train = [0, n_train), test = [n_train, N): windows of one upload
    adam = {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in theta.items()}

    def desc():
        var, ell = softplus(theta["k"][0]), softplus(theta["k"][1])
        return _ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, [1.0 / ell], theta["z"], theta["m"], np.tril(theta["A"]), jitter,
                              likelihood=_ffi.LIK_GAUSSIAN, lik_sigma2=lik_noise), ell

    model = _ffi.DeviceModel(ctx, *desc()[0])
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    for step in range(1, steps + 1):
        (d, keep), ell = desc()
        model.update(d, keep)
        off = int(rng.integers(0, n_train - batch))
        _, _, g = model.elbo_grad(data, off, batch, float(n_train), z_shape=(M,))
        grads = {"k": -np.array([g["variance"] * sig(theta["k"][0]), g["inv_lengthscale"][0] * (-1.0 / ell**2) * sig(theta["k"][1])]),
                 "z": -np.asarray(g["z"]), "m": -np.asarray(g["m"]), "A": -np.tril(np.asarray(g["Lq"]))}
        for k in theta:
            m1, m2 = adam[k]
            m1[...] = 0.9 * m1 + 0.1 * grads[k]
            m2[...] = 0.999 * m2 + 0.001 * grads[k] ** 2
            theta[k] = theta[k] - lr * (m1 / (1 - 0.9**step)) / (np.sqrt(m2 / (1 - 0.999**step)) + 1e-8)
    model.update(*desc()[0])
    s = model.predictive(data, n_train, n_test, want=("summary",))["summary"]
    rmse, nlpd = np.sqrt(s.sum_sq_err / s.n_points), -s.sum_lpd / s.n_points
    print(f"regression:     {steps} Adam steps, {s.n_points} held-out points: RMSE {rmse:.4f} (noise sd {np.sqrt(lik_noise):.4f}), mean NLPD {nlpd:.4f}")
    model.free()
    data.free()
    return rmse, nlpd


def classification(ctx, seed=1, maxiter=300):
    """b_classification.py's model (SE kernel, Bernoulli-logistic, N = 30, M = 15), L-BFGS on the negative ELBO."""
    rng = np.random.default_rng(seed)
    x_true = np.arange(0.0, 6.0 + 1e-9, 0.02)
    k_true = lambda a, b: 10.0 * np.exp(-0.5 * (0.9 * (a[:, None] - b[None, :])) ** 2)
    f_true = np.linalg.cholesky(k_true(x_true, x_true) + 1e-6 * np.eye(x_true.size)) @ rng.standard_normal(x_true.size)
    y_true = (rng.random(x_true.size) < 1.0 / (1.0 + np.exp(-f_true))).astype(np.float64)
    N, M, jitter = 30, 15, 1e-3
    train = np.zeros(x_true.size, dtype=bool)
    train[rng.choice(x_true.size, N, replace=False)] = True
    x, y, xt, yt = x_true[train], y_true[train], x_true[~train], y_true[~train]
    data, test = _ffi.DeviceData(ctx, x, y, np.float64), _ffi.DeviceData(ctx, xt, yt, np.float64)

    def unpack(t):
        return np.exp(t[0]), np.exp(t[1]), t[2:2 + M], t[2 + M:2 + 2 * M], np.tril(t[2 + 2 * M:].reshape(M, M))

    def desc(t):
        var, prec, z, m, A = unpack(t)
        A = A + 1e-9 * np.eye(M) * (np.abs(np.diag(A)) < 1e-9)
        return _ffi.make_desc(np.float64, _ffi.KERNEL_SE, var, [prec], z, m, A, jitter, likelihood=_ffi.LIK_BERNOULLI_LOGISTIC)

    t0 = np.concatenate([np.log([rng.random() + 0.1, rng.random() + 0.1]), rng.uniform(0, 6, M), np.zeros(M), np.eye(M).ravel()])
    model = _ffi.DeviceModel(ctx, *desc(t0))

    def loss_and_grad(t):
        var, prec, z, m, A = unpack(t)
        try:
            model.update(*desc(t))
            val, _, g = model.elbo_grad(data, 0, N, float(N), z_shape=(M,))
        except (_ffi.PosDefException, _ffi.DomainError):
            return 1e10, np.zeros_like(t)
        grad = np.concatenate([[g["variance"] * var, g["inv_lengthscale"][0] * prec], np.asarray(g["z"]), np.asarray(g["m"]),
                               np.tril(np.asarray(g["Lq"])).ravel()])
        return -val, -grad

    res = minimize(loss_and_grad, t0, jac=True, method="L-BFGS-B", options={"maxiter": maxiter})
    model.update(*desc(res.x))
    out = model.predictive(test, want=("summary", "ymean"))
    s, p1 = out["summary"], out["ymean"]
    nlpd, acc = -s.sum_lpd / s.n_points, float(((p1 > 0.5) == (yt > 0.5)).mean())
    print(f"classification: {res.nit} L-BFGS iterations, {s.n_points} held-out points: mean NLPD {nlpd:.4f} (coin flip {np.log(2):.4f}), "
          f"accuracy {acc:.3f}")
    print("  x          :", np.round(xt[::30], 2))
    print("  p(y* = 1)  :", np.round(p1[::30], 2))
    print("  true p     :", np.round(1.0 / (1.0 + np.exp(-f_true[~train][::30])), 2))
    # the same through the reference-shaped API: posterior(sva, lfx, y).predict_y / log_predictive_density
    var, prec, z, m, A = unpack(res.x)
    A = A + 1e-9 * np.eye(M) * (np.abs(np.diag(A)) < 1e-9)
    f = ag.GP(var * ag.TransformedKernel(ag.SqExponentialKernel(), ag.ScaleTransform(prec)))
    sva = ag.SparseVariationalApproximation(f(z, jitter), ag.MvNormal.from_cholesky(m, A))
    post = ag.posterior(sva, ag.LatentGP(f, ag.BernoulliLikelihood(), 1e-6)(x), y, ctx=ctx)
    assert np.allclose(post.predict_y(xt)[0], p1, rtol=0, atol=1e-10)
    assert abs(-post.log_predictive_density(xt, yt).mean() - nlpd) < 1e-10
    for h in (model, data, test):
        h.free()
    return nlpd, acc


def main():
    ctx = _ffi.default_context()
    return regression(ctx), classification(ctx)


if __name__ == "__main__":
    main()
