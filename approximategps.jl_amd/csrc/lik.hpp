// lik.hpp — likelihood device functions shared by expect_kernel (strip.hip) and the gradient path (grad.hip):
// log p(y|f), its expectation under N(mu, v) and the derivatives of that expectation  [GPLikelihoods].
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace svgp {


__device__ __forceinline__ double softplus_d(double s) { return fmax(s, 0.0) + log1p(exp(-fabs(s))); }

// log Phi(x) and the hazard phi(x) / Phi(x) of the standard normal (the NormalCDFLink Bernoulli), through the scaled
// complementary error function on the negative side: no underflow and no cancellation in either tail
__device__ __forceinline__ double log_ndtr_d(double x) {
  const double u = -0.70710678118654752440 * x;   // Phi(x) = erfc(u) / 2
  return u > 0.0 ? log(0.5 * erfcx(u)) - u * u : log1p(-0.5 * erfc(-u));
}
__device__ __forceinline__ double ndtr_hazard_d(double x) {
  const double u = -0.70710678118654752440 * x;
  return u > 0.0 ? 0.79788456080286535588 / erfcx(u) : 0.39894228040143267794 * exp(-u * u) / (1.0 - 0.5 * erfc(-u));
}

// digamma: recurrence up to x >= 6, then the asymptotic series (|error| < 1e-14)
__host__ __device__ inline double digamma_d(double x) {
  double r = 0.0;
  while (x < 6.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  return r + log(x) - 0.5 / x -
         f * (1.0 / 12.0 - f * (1.0 / 120.0 - f * (1.0 / 252.0 - f * (1.0 / 240.0 - f * (1.0 / 132.0)))));
}

// log p(y | f)  [GPLikelihoods]
__device__ __forceinline__ double loglik_point(int lik, double f, double y, double sigma2, double log_sigma2) {
  if (lik == 0) {
    const double r = y - f;
    return -0.5 * (1.8378770664093453 + log_sigma2 + r * r / sigma2);
  }
  if (lik == 1) return -softplus_d(y > 0.5 ? -f : f);
  if (lik == 2) return y * f - exp(f) - lgamma(y + 1.0);
  if (lik == 3) return -f - y * exp(-f);                                         // Exponential(scale e^f) = Gamma(1, scale e^f)
  if (lik == 5) return log_ndtr_d(y > 0.5 ? f : -f);                             // Bernoulli(Phi(f)): log Phi(+-f)
  return (sigma2 - 1.0) * log(y) - y * exp(-f) - sigma2 * f - lgamma(sigma2);    // Gamma(alpha = sigma2, scale e^f)
}

// E_{N(mu, v)}[log p(y|f)]: closed form (gh_n == 0) or Gauss-Hermite  [GPLikelihoods.expected_loglikelihood]
__device__ __forceinline__ double expected_loglik_point(const LikParams& lp, double mu, double v, double y,
                                                        double log_sigma2) {
  if (lp.gh_n == 0) {
    if (lp.lik == 0) {
      const double r = y - mu;
      return -0.5 * (1.8378770664093453 + log_sigma2 + (r * r + v) / lp.sigma2);
    }
    if (lp.lik == 2) return y * mu - exp(mu + 0.5 * v) - lgamma(y + 1.0);  // Poisson, exp link
    if (lp.lik == 3) return -mu - y * exp(0.5 * v - mu);                   // Exponential (scale), exp link
    return (lp.sigma2 - 1.0) * log(y) - y * exp(0.5 * v - mu) - lp.sigma2 * mu - lgamma(lp.sigma2);  // Gamma, exp link
  }
  const double s = 1.4142135623730951 * sqrt(v);
  double acc = 0.0;
  for (int q = 0; q < lp.gh_n; ++q) acc += lp.gh_w[q] * loglik_point(lp.lik, s * lp.gh_x[q] + mu, y, lp.sigma2, log_sigma2);
  return acc;  // weights are pre-divided by sqrt(pi)
}

// ---- the predictive distribution of the OBSERVATION (predictive.hip: svgp_predictive / svgp_lik_predictive) -----------------------
// For both functions lp.gh_n is the PREDICTIVE rule (api_predictive.hip: predictive_gh): 0 = closed form, which exists for the Gaussian and the
// normcdf Bernoulli only; every other likelihood arrives with a Gauss-Hermite rule (GH-20 when the model's quadrature_n is 0).
// Poisson, Exponential and Gamma have a closed-form ELBO expectation (expected_loglik_point) but NO closed-form predictive density:
// E[exp(-e^f)] of a log-normal has none.  They take the quadrature here.

// log p(y | D) = log int p(y | f) N(f; mu, v) df, a different quantity from E_q[log p(y | f)] above (which bounds it from below, Jensen).
//   Gaussian            log N(y; mu, v + sigma2)
//   Bernoulli(Phi(f))   log Phi(+-mu / sqrt(1 + v))
//   otherwise, and every likelihood with lp.gh_n > 0:  logsumexp_q(log w_q + log p(y | f_q)),  f_q = mu + sqrt(2 v) x_q, in ONE pass
//   with a running maximum (a plain log(sum w_q exp(.)) underflows for a Poisson count of a few hundred).  Weights that underflowed to 0
//   (the high orders) and terms at -inf are skipped.  v = 0 (a clamped point) collapses to loglik_point(mu).
// log p(y | f) = loglik_f_part + loglik_y_part: the terms that depend on f, and the rest (lgamma, log y, the normalisations), which the
// quadrature below adds once per point instead of once per node
__device__ __forceinline__ double loglik_f_part(int lik, double f, double y, double sigma2) {
  if (lik == 0) {
    const double r = y - f;
    return -0.5 * r * r / sigma2;
  }
  if (lik == 1) return -softplus_d(y > 0.5 ? -f : f);
  if (lik == 2) return y * f - exp(f);
  if (lik == 3) return -f - y * exp(-f);
  if (lik == 5) return log_ndtr_d(y > 0.5 ? f : -f);
  return -y * exp(-f) - sigma2 * f;
}
// (not inlined, and static so that a translation unit that does not use it emits nothing: lgamma's double-precision code is what
// pushes expect_kernel to one wave per SIMD; behind a call predictive_kernel stays at 158 VGPRs without spills)
static __device__ __noinline__ double loglik_y_part(int lik, double y, double sigma2) {
  if (lik == 0) return -0.5 * (1.8378770664093453 + log(sigma2));
  if (lik == 2) return -lgamma(y + 1.0);
  if (lik == 4) return (sigma2 - 1.0) * log(y) - lgamma(sigma2);
  return 0.0;
}

__device__ __forceinline__ double predictive_logdensity_point(const LikParams& lp, double mu, double v, double y) {
  if (lp.gh_n == 0) {
    if (lp.lik == 0) {
      const double r = y - mu, t = v + lp.sigma2;
      return -0.5 * (1.8378770664093453 + log(t) + r * r / t);
    }
    const double z = mu / sqrt(1.0 + v);
    return log_ndtr_d(y > 0.5 ? z : -z);
  }
  const double s = 1.4142135623730951 * sqrt(v);
  double mx = -INFINITY, acc = 0.0;   // sum_q exp(t_q) = exp(mx) acc
#pragma unroll 1
  for (int q = 0; q < lp.gh_n; ++q) {
    const double w = lp.gh_w[q];      // pre-divided by sqrt(pi)
    if (!(w > 0.0)) continue;
    const double t = log(w) + loglik_f_part(lp.lik, s * lp.gh_x[q] + mu, y, lp.sigma2);
    if (t == -INFINITY) continue;
    if (t > mx) {
      acc = acc * exp(mx - t) + 1.0;
      mx = t;
    } else {
      acc += exp(t - mx);             // a NaN t lands here and stays
    }
  }
  return mx + log(acc) + loglik_y_part(lp.lik, y, lp.sigma2);
}

// (E[y], Var[y]) under the same marginal; no y needed.  Closed forms wherever they exist, whatever lp.gh_n is.  With e1 = exp(mu + v/2):
//   Gaussian            (mu, v + sigma2)
//   Bernoulli           p = E[link(f)], (p, p (1 - p));  p = Phi(mu / sqrt(1 + v)) for normcdf, Gauss-Hermite of the sigmoid for logistic
//   Poisson(e^f)        (e1, e1 + expm1(v) e1^2)
//   Exponential(e^f)    (e1, exp(2 mu + 2 v) + expm1(v) e1^2)
//   Gamma(alpha, e^f)   (alpha e1, alpha exp(2 mu + 2 v) + alpha^2 expm1(v) e1^2)
__device__ __forceinline__ void predictive_moments_point(const LikParams& lp, double mu, double v, double& ymean, double& yvar) {
  if (lp.lik == 0) {
    ymean = mu;
    yvar = v + lp.sigma2;
    return;
  }
  if (lp.lik == 1 || lp.lik == 5) {
    double p = 0.0;
    if (lp.lik == 5) {
      p = 0.5 * erfc(-0.70710678118654752440 * mu / sqrt(1.0 + v));
    } else {
      const double s = 1.4142135623730951 * sqrt(v);
#pragma unroll 1
      for (int q = 0; q < lp.gh_n; ++q) p += lp.gh_w[q] / (1.0 + exp(-(s * lp.gh_x[q] + mu)));
    }
    ymean = p;
    yvar = p * (1.0 - p);
    return;
  }
  const double e1 = exp(mu + 0.5 * v), spread = expm1(v) * e1 * e1, e2 = exp(2.0 * mu + 2.0 * v);
  if (lp.lik == 2) {
    ymean = e1;
    yvar = e1 + spread;
  } else if (lp.lik == 3) {
    ymean = e1;
    yvar = e2 + spread;
  } else {
    ymean = lp.sigma2 * e1;
    yvar = lp.sigma2 * e2 + lp.sigma2 * lp.sigma2 * spread;
  }
}


// d log p(y|f) / df
__device__ __forceinline__ double dloglik_point(int lik, double f, double y, double sigma2) {
  if (lik == 0) return (y - f) / sigma2;
  if (lik == 1) return y - 1.0 / (1.0 + exp(-f));
  if (lik == 2) return y - exp(f);
  if (lik == 3) return y * exp(-f) - 1.0;
  if (lik == 5) return y > 0.5 ? ndtr_hazard_d(f) : -ndtr_hazard_d(-f);
  return y * exp(-f) - sigma2;
}

// d2 log p(y|f) / df2 and d3 log p(y|f) / df3 (the Laplace approximation: W = -d2, the gradient's s2 = -diag(Sigma) d3 / 2).
// All six are log-concave in f, so d2 <= 0.  Probit: with sg = +-1 for y = 1 / 0, t = sg f and h = phi(t) / Phi(t),
// dll = sg h, d2 = h' = -h (t + h), d3 = sg h'' with h'' = -h' (t + h) - h (1 + h').
__device__ __forceinline__ void d23loglik_point(int lik, double f, double y, double sigma2, double& d2, double& d3) {
  if (lik == 0) {
    d2 = -1.0 / sigma2;
    d3 = 0.0;
  } else if (lik == 1) {
    const double s = 1.0 / (1.0 + exp(-f)), v = s * (1.0 - s);
    d2 = -v;
    d3 = -v * (1.0 - 2.0 * s);
  } else if (lik == 2) {
    d2 = -exp(f);
    d3 = d2;
  } else if (lik == 5) {
    const double sg = y > 0.5 ? 1.0 : -1.0, t = sg * f, h = ndtr_hazard_d(t);
    const double h1 = -h * (t + h);
    d2 = h1;
    d3 = sg * (-h1 * (t + h) - h * (1.0 + h1));
  } else {   // Exponential and Gamma with the exp link (scale e^f): the f-dependence is -y e^-f in both
    d3 = y * exp(-f);
    d2 = -d3;
  }
}

// (dE/dmu, dE/dv, dE/dsigma2) of expected_loglik_point: closed forms, or Gauss-Hermite with
// dE/dmu = sum w g'(f_q), dE/dv = sum w g'(f_q) x_q / sqrt(2 v)
__device__ __forceinline__ void expected_loglik_grad_point(const LikParams& lp, double mu, double v, double y, double& gmu,
                                                           double& gv, double& gs2) {
  gs2 = 0.0;
  if (lp.gh_n == 0) {
    if (lp.lik == 0) {
      const double r = y - mu;
      gmu = r / lp.sigma2;
      gv = -0.5 / lp.sigma2;
      gs2 = -0.5 * (1.0 / lp.sigma2 - (r * r + v) / (lp.sigma2 * lp.sigma2));
    } else if (lp.lik == 2) {
      const double e = exp(mu + 0.5 * v);
      gmu = y - e;
      gv = -0.5 * e;
    } else if (lp.lik == 3) {
      const double e = y * exp(0.5 * v - mu);
      gmu = e - 1.0;
      gv = -0.5 * e;
    } else {
      const double e = y * exp(0.5 * v - mu);
      gmu = e - lp.sigma2;
      gv = -0.5 * e;
      gs2 = log(y) - mu - lp.digamma_alpha;      // d/d alpha
    }
    return;
  }
  const double s = 1.4142135623730951 * sqrt(v);
  const double inv_s = s > 0.0 ? 1.0 / s : 0.0;
  gmu = 0.0;
  gv = 0.0;
  for (int q = 0; q < lp.gh_n; ++q) {
    const double f = s * lp.gh_x[q] + mu;
    const double dl = dloglik_point(lp.lik, f, y, lp.sigma2);
    gmu += lp.gh_w[q] * dl;
    gv += lp.gh_w[q] * dl * lp.gh_x[q] * inv_s;
    if (lp.lik == 0) gs2 += lp.gh_w[q] * (-0.5 / lp.sigma2 + 0.5 * (y - f) * (y - f) / (lp.sigma2 * lp.sigma2));
    if (lp.lik == 4) gs2 += lp.gh_w[q] * (log(y) - f - lp.digamma_alpha);
  }
}

}  // namespace svgp
