"""float64 numpy restatement of the predictive distribution of the OBSERVATION (csrc/lik.hpp: predictive_logdensity_point,
predictive_moments_point; csrc/predictive.hip), for latent marginals N(mu_i, v_i):

    lpd_i   = log p(y_i | D) = log int p(y_i | f) N(f; mu_i, v_i) df
    ymean_i = E[y_i],  yvar_i = Var[y_i]

The marginals come from oracle/svgp_oracle.py's posterior (mean_and_var, plus the 1e-18 of marginals()), the quadrature rule is
svgp_oracle.gausshermite - the rule the library's svgp_gausshermite is tested against.  tests/test_predictive_cpu.py pins this
restatement against adaptive quadrature, Monte Carlo and normalisation, independently of the device."""
import math

import numpy as np
from scipy.special import log_ndtr, logsumexp, ndtr

import svgp_oracle as o

DEFAULT_GH = 20
LIKS = (o.LIK_GAUSSIAN, o.LIK_BERNOULLI_LOGISTIC, o.LIK_POISSON_EXP, o.LIK_EXPONENTIAL_EXP, o.LIK_GAMMA_EXP, o.LIK_BERNOULLI_NORMCDF)


def predictive_gh(lik: int, quadrature_n: int = 0) -> int:
    """The predictive rule: quadrature_n > 0 forces GH-n; 0 = closed form (returned as 0) for the Gaussian and the normcdf Bernoulli,
    GH-20 for everything else - Poisson, Exponential and Gamma have a closed-form ELBO term but no closed-form predictive density."""
    if quadrature_n > 0:
        return int(quadrature_n)
    return 0 if lik in (o.LIK_GAUSSIAN, o.LIK_BERNOULLI_NORMCDF) else DEFAULT_GH


def _rule(n):
    xs, ws = o.gausshermite(n)
    return np.asarray(xs, dtype=np.float64), np.asarray(ws, dtype=np.float64) / math.sqrt(math.pi)


def lpd(lik, mu, v, y, param=1.0, quadrature_n=0):
    """log p(y_i | D) per point; v >= 0 (v = 0: the quadrature collapses to log p(y | mu))."""
    mu, v, y = (np.asarray(a, dtype=np.float64) for a in (mu, v, y))
    n = predictive_gh(lik, quadrature_n)
    if n == 0:
        if lik == o.LIK_GAUSSIAN:
            t = v + param
            return -0.5 * (math.log(2.0 * math.pi) + np.log(t) + (y - mu) ** 2 / t)
        z = mu / np.sqrt(1.0 + v)
        return log_ndtr(np.where(y > 0.5, z, -z))
    xs, ws = _rule(n)
    keep = ws > 0.0                                  # weights that underflowed at high orders are skipped
    f = mu[None, :] + np.sqrt(2.0 * v)[None, :] * xs[keep, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log(ws[keep])[:, None] + o.loglik(lik, f, y[None, :], param)
    return logsumexp(t, axis=0)


def moments(lik, mu, v, param=1.0, quadrature_n=0):
    """(E[y_i], Var[y_i]) per point: closed forms wherever they exist, Gauss-Hermite of the sigmoid for the logistic Bernoulli."""
    mu, v = np.asarray(mu, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if lik == o.LIK_GAUSSIAN:
        return mu.copy(), v + param
    if lik == o.LIK_BERNOULLI_NORMCDF:
        p = ndtr(mu / np.sqrt(1.0 + v))
        return p, p * (1.0 - p)
    if lik == o.LIK_BERNOULLI_LOGISTIC:
        xs, ws = _rule(predictive_gh(lik, quadrature_n))
        f = mu[None, :] + np.sqrt(2.0 * v)[None, :] * xs[:, None]
        with np.errstate(over="ignore"):
            p = (ws[:, None] / (1.0 + np.exp(-f))).sum(axis=0)
        return p, p * (1.0 - p)
    e1 = np.exp(mu + 0.5 * v)
    spread = np.expm1(v) * e1 * e1
    e2 = np.exp(2.0 * mu + 2.0 * v)
    if lik == o.LIK_POISSON_EXP:
        return e1, e1 + spread
    if lik == o.LIK_EXPONENTIAL_EXP:
        return e1, e2 + spread
    if lik == o.LIK_GAMMA_EXP:
        return param * e1, param * e2 + param * param * spread
    raise ValueError("unknown likelihood")


def from_marginals(lik, mu, v, y=None, param=1.0, quadrature_n=0, clamp=False):
    """The outputs of svgp_lik_predictive / the point stage of svgp_predictive for marginals (mu, v), v including the 1e-18: a dict of
    lpd, ymean, yvar (NaN at the points with v < 0 unless clamp, which evaluates them at v = 0), sum_lpd, sum_sq_err, n_points,
    n_neg_var.  Without y: ymean and yvar only."""
    mu, v = np.asarray(mu, dtype=np.float64), np.asarray(v, dtype=np.float64)
    neg = v < 0.0
    vv = np.where(neg, 0.0, v)
    ok = np.ones(mu.shape, dtype=bool) if clamp else ~neg
    ym, yv = moments(lik, mu, vv, param, quadrature_n)
    out = {"ymean": np.where(ok, ym, np.nan), "yvar": np.where(ok, yv, np.nan), "n_neg_var": int(neg.sum()), "n_points": int(ok.sum())}
    if y is not None:
        y = np.asarray(y, dtype=np.float64)
        lp = lpd(lik, mu, vv, y, param, quadrature_n)
        out["lpd"] = np.where(ok, lp, np.nan)
        out["sum_lpd"] = float(lp[ok].sum())
        out["sum_sq_err"] = float(((y - ym)[ok] ** 2).sum())
    return out


def latent_marginals(sva, x, mux=None):
    """(mu, v + 1e-18) of the oracle's posterior at x (no DomainError: the caller decides about negative variances); mux: prior mean
    offsets of a NonCentered model without offsets at z, which enter the mean by one addition."""
    mu, v = o.mean_and_var(o.posterior(sva), x)
    mu = np.asarray(mu, dtype=np.float64)
    if mux is not None:
        assert not sva.centered
        mu = mu + np.asarray(mux, dtype=np.float64)
    return mu, np.asarray(v, dtype=np.float64) + o.DEFAULT_SIGMA2


def predictive(sva, x, y, lik, param=1.0, quadrature_n=0, mux=None, clamp=False):
    """svgp_predictive restated: the oracle's marginals at x, then from_marginals."""
    mu, v = latent_marginals(sva, x, mux)
    return from_marginals(lik, mu, v, y, param, quadrature_n, clamp)


def expected_loglik_points(lik, mu, v, y, param=1.0, quadrature_n=0):
    """E_q[log p(y_i | f_i)] per point (the ELBO's term, svgp_oracle.expected_loglik one point at a time): what Jensen puts below lpd."""
    mu, v, y = (np.asarray(a, dtype=np.float64) for a in (mu, v, y))
    sd = np.sqrt(v)
    return np.array([o.expected_loglik(lik, mu[i:i + 1], sd[i:i + 1], y[i:i + 1], param, quadrature_n) for i in range(mu.shape[0])])
