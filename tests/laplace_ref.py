"""Reference Laplace approximation for the tests, in float64 numpy, on top of svgp_oracle's kernel matrix and log-likelihoods
(the restatement tests/test_reference_literal_pin.py makes, extended to every likelihood, predictions and the gradient).

Follows the reference's src/LaplaceApproximationModule.jl: the Newton loop of _newton_inner_loop (:256-276, RW Alg. 3.1) with
its isapprox stopping rule (keep f when it holds), laplace_lml (:157-165, :250-254) recomputed at f_opt, predictions :425-463
(RW 3.21 / 3.29), and the gradient of approx_lml with respect to the kernel parameters in closed form (RW Alg. 5.1, any
likelihood through d3 log p):
    R = sW B^-1 sW,  s2 = diag(K - K R K) d3 / 2 (d lml / d f_opt: W = -d2 so dW/df = -d3),  u = s2 - R K s2,  P = a a' / 2 - R / 2 + (u g' + g u') / 2,
    d lml / d theta = sum_ik P_ik dK_ik / d theta."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular
from scipy.special import expit, log_ndtr

import svgp_oracle as o


def d2d3(lik, f, y, s2):
    """d2 log p(y|f) / df2 and d3 log p(y|f) / df3 per point."""
    f = np.asarray(f, dtype=np.float64)
    if lik == o.LIK_GAUSSIAN:
        return np.full_like(f, -1.0 / s2), np.zeros_like(f)
    if lik == o.LIK_BERNOULLI_LOGISTIC:
        s = expit(f)
        v = s * (1.0 - s)
        return -v, -v * (1.0 - 2.0 * s)
    if lik == o.LIK_POISSON_EXP:
        e = np.exp(f)
        return -e, -e
    if lik in (o.LIK_EXPONENTIAL_EXP, o.LIK_GAMMA_EXP):
        e = y * np.exp(-f)
        return -e, e
    if lik == o.LIK_BERNOULLI_NORMCDF:
        sg = np.where(y > 0.5, 1.0, -1.0)
        t = sg * f
        h = np.exp(-0.5 * t * t - 0.5 * np.log(2 * np.pi) - log_ndtr(t))
        h1 = -h * (t + h)
        return h1, sg * (-h1 * (t + h) - h * (1.0 + h1))
    raise ValueError(lik)


def _terms(lik, f, y, s2):
    ll = float(np.sum(o.loglik(lik, f, y, s2)))
    g = np.asarray(o._dloglik(lik, f, y, s2), dtype=np.float64)
    d2, d3 = d2d3(lik, f, y, s2)
    return ll, g, -d2, d3


def intermediates(K, lik, y, s2, f):
    """_laplace_train_intermediates (:201-240) at f"""
    ll, g, W, d3 = _terms(lik, f, y, s2)
    sW = np.sqrt(np.maximum(W, 0.0))
    B = np.eye(K.shape[0]) + (sW[:, None] * K) * sW[None, :]
    L = np.linalg.cholesky(B)
    b = W * f + g
    a = b - sW * cho_solve((L, True), sW * (K @ b))
    return dict(ll=ll, g=g, W=W, sW=sW, d3=d3, L=L, a=a, f=f)


def kernel_of(family, variance, inv_lengthscale):
    return o.Kernel(family, float(variance), np.atleast_1d(np.asarray(inv_lengthscale, dtype=np.float64)))


def fit(kernel, x, y, lik, s2=1.0, jitter=0.0, f_init=None, maxiter=100, eps=np.finfo(np.float64).eps):
    """-> (lml, cache, iterations, converged).  eps: of the compute type (isapprox's sqrt(eps(T)))."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    K = o.kernelmatrix(kernel, x).astype(np.float64) + jitter * np.eye(y.size)
    f = np.zeros(y.size) if f_init is None else np.asarray(f_init, dtype=np.float64).copy()
    rtol = np.sqrt(eps)
    converged, it = False, 0
    for it in range(1, maxiter + 1):
        c = intermediates(K, lik, y, s2, f)
        fnew = K @ c["a"]
        if np.linalg.norm(f - fnew) <= rtol * max(np.linalg.norm(f), np.linalg.norm(fnew)):
            converged = True
            break
        f = fnew
    if not converged:   # converged: the loop keeps f, whose intermediates c already are (the recomputation gives the same)
        c = intermediates(K, lik, y, s2, f)
    c["K"] = K
    lml = -0.5 * float(c["a"] @ f) + c["ll"] - float(np.sum(np.log(np.diag(c["L"]))))
    return lml, c, it, converged


def round32(a):
    """every entry rounded once to float32 (the least an fp32 evaluation does to a stored operand), float64 afterwards"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def fit_one_rounding(kernel, x, y, lik, s2=1.0, jitter=0.0, maxiter=100):
    """-> (cache, iterations): the forward-error model of an fp32 Newton loop from zero - fit() in float64 arithmetic, with an
    exact solve, but K and every vector a step stores (g, W, sW, b, a, fnew) rounded once to float32, and float32's stop rule.
    Its cache feeds predict(..., one_rounding=True): the one-rounding model of a prediction from the mode up."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K = round32(o.kernelmatrix(kernel, x).astype(np.float64) + jitter * np.eye(y.size))
    f, rtol = np.zeros(y.size), np.sqrt(np.finfo(np.float32).eps)

    def step(f):
        _, g, W, _ = _terms(lik, f, y, s2)
        g, W = round32(g), round32(W)
        sW = round32(np.sqrt(np.maximum(W, 0.0)))
        L = np.linalg.cholesky(np.eye(K.shape[0]) + (sW[:, None] * K) * sW[None, :])
        b = round32(W * f + g)
        return dict(g=g, W=W, sW=sW, L=L, a=round32(b - sW * cho_solve((L, True), sW * (K @ b))), f=f, K=K)

    for it in range(1, maxiter + 1):
        c = step(f)
        fnew = round32(K @ c["a"])
        if np.linalg.norm(f - fnew) <= rtol * max(np.linalg.norm(f), np.linalg.norm(fnew)):
            return c, it
        f = fnew
    return step(f), maxiter


def lml_grad(kernel, x, y, lik, s2=1.0, jitter=0.0, f_init=None, maxiter=100, eps=np.finfo(np.float64).eps, one_rounding=False):
    """-> (lml, d lml / d variance, d lml / d inv_lengthscale (d,)).  one_rounding: the forward-error model of an fp32 evaluation
    (as tests/f32_grad_accuracy.py's for the SVGP gradient) - the same closed form in float64 arithmetic with K, R and every vector
    the reduction reads (a, g, s2, u) rounded once to float32; pass eps of float32 with it for the format's Newton stop."""
    lml, c, _, _ = fit(kernel, x, y, lik, s2, jitter, f_init, maxiter, eps)
    rnd = round32 if one_rounding else (lambda v: v)
    K, sW, L, g, a, d3 = rnd(c["K"]), rnd(c["sW"]), c["L"], rnd(c["g"]), rnd(c["a"]), rnd(c["d3"])
    Linv = solve_triangular(L, np.eye(L.shape[0]), lower=True)
    R = rnd(sW[:, None] * (Linv.T @ Linv) * sW[None, :])
    sigma = np.diag(K) - np.einsum("ij,ji->i", K @ R, K)
    s2v = rnd(0.5 * sigma * d3)
    u = rnd(s2v - R @ (K @ s2v))
    P = 0.5 * np.outer(a, a) - 0.5 * R + 0.5 * (np.outer(u, g) + np.outer(g, u))
    xd = o._as_dn(np.asarray(x, dtype=np.float64))
    il = np.asarray(kernel.inv_lengthscale, dtype=np.float64)
    diff2 = (xd[:, :, None] - xd[:, None, :]) ** 2                      # (d, n, n)
    r2 = np.einsum("f,fij->ij", il ** 2, diff2)
    unit = kernel_of(kernel.family, 1.0, il)
    kap = o._kappa(unit, r2)
    if kernel.family == o.KERNEL_SE:
        dk = -0.5 * kap
    elif kernel.family == o.KERNEL_MATERN32:
        dk = -1.5 * np.exp(-np.sqrt(3.0 * r2))
    else:
        s = np.sqrt(5.0 * r2)
        dk = -(5.0 / 6.0) * (1.0 + s) * np.exp(-s)
    dvar = float(np.sum(P * kap))
    dil = np.array([float(np.sum(P * kernel.variance * dk * 2.0 * il[f] * diff2[f])) for f in range(il.size)])
    return lml, dvar, dil


def predict(cache, kernel, x, xs, ys=None, one_rounding=False):
    """-> (mean, var, cov) at xs (cov(xs, ys) when ys is given): RW 3.21 / 3.29.  Inputs of any float type (float32-rounded
    x / xs for an fp32 device handle) are taken as they are, in float64 arithmetic.  one_rounding: the forward-error model of an
    fp32 evaluation - every stored operand (k(x, x*), g, sW, L^-1 sW k(x, x*), k(x*, x*)) rounded once to float32."""
    rnd = round32 if one_rounding else (lambda a: a)
    x = np.asarray(x, dtype=np.float64)
    kx = rnd(o.kernelmatrix(kernel, x, np.asarray(xs, dtype=np.float64)).astype(np.float64))
    mean = kx.T @ rnd(cache["g"])
    sW = rnd(cache["sW"])
    v = rnd(solve_triangular(cache["L"], sW[:, None] * kx, lower=True))
    var = kernel.variance - np.sum(v * v, axis=0)
    if ys is None:
        cov = rnd(o.kernelmatrix(kernel, np.asarray(xs, dtype=np.float64)).astype(np.float64)) - v.T @ v
    else:
        ky = rnd(o.kernelmatrix(kernel, x, np.asarray(ys, dtype=np.float64)).astype(np.float64))
        vy = rnd(solve_triangular(cache["L"], sW[:, None] * ky, lower=True))
        cov = rnd(o.kernelmatrix(kernel, np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)).astype(np.float64)) - v.T @ vy
    return mean, var, cov


def synth(lik, n, d, seed, dtype=np.float64):
    """x (d, n) and observations y for `lik` from a latent draw."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, size=(d, n))
    f = np.sin(2.0 * x[0]) + (0.5 * np.cos(3.0 * x[1]) if d > 1 else 0.0)
    if lik == o.LIK_GAUSSIAN:
        y = f + 0.1 * rng.standard_normal(n)
    elif lik in (o.LIK_BERNOULLI_LOGISTIC, o.LIK_BERNOULLI_NORMCDF):
        y = (rng.uniform(size=n) < expit(2.0 * f)).astype(np.float64)
    elif lik == o.LIK_POISSON_EXP:
        y = rng.poisson(np.exp(f)).astype(np.float64)
    else:
        y = rng.gamma(2.0, np.exp(f) / 2.0) + 1e-3
    return x.astype(dtype), y.astype(dtype)
