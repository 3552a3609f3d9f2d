// api_predictive.hip — the predictive distribution of the observation: svgp_predictive, svgp_lik_predictive (predictive.hip, lik.hpp
// hold the kernel).  Host orchestration only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"

using namespace svgp;

// ---- the predictive distribution of the observation (predictive.hip, lik.hpp) -----------------------------------------------------
// svgp_predictive: the forward data pass svgp_elbo runs (elbo_enqueue: prep + strips, beside each other where svgp_elbo overlaps
// them), then predictive_kernel where svgp_elbo has expect_kernel.  svgp_lik_predictive: the same point stage on a caller's
// marginals.  Both are local: no collective.
namespace {
// the predictive rule: quadrature_n > 0 forces GH-n; 0 = closed form where one exists (Gaussian, normcdf Bernoulli), else GH-20.
// Not effective_gh: the ELBO's closed forms (Poisson, Exponential, Gamma) have no predictive counterpart, the normcdf Bernoulli's
// predictive density is closed where its ELBO term is not.
int predictive_gh(int lik, int quadrature_n) {
  if (quadrature_n > 0) return quadrature_n;
  return (lik == SVGP_LIK_GAUSSIAN || lik == SVGP_LIK_BERNOULLI_NORMCDF) ? 0 : 20;
}

// the rule on the device (ctx->pred_gh: nodes | weights / sqrt(pi)), kept between calls.  Every call that reads it has synchronised
// the stream before it returned, so replacing it here races with nothing
int ensure_predictive_rule(svgp_ctx* ctx, int gh) {
  if (gh == 0 || gh == ctx->pred_gh_n) return SVGP_OK;
  std::vector<double> xw(2 * size_t(gh));
  if (gauss_hermite(gh, xw.data(), xw.data() + gh) != SVGP_OK) return fail(ctx, SVGP_INVALID_ARG, "Gauss-Hermite rule failed to converge");
  for (int q = 0; q < gh; ++q) xw[gh + q] /= 1.7724538509055160273;
  ctx->pred_gh_n = 0;
  const int rc = ctx->pred_gh.reserve(ctx, xw.size() * sizeof(double), "the predictive Gauss-Hermite rule");
  if (rc) return rc;
  HIPC(ctx, hipMemcpyAsync(ctx->pred_gh.p, xw.data(), xw.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  ctx->pred_gh_n = gh;
  return SVGP_OK;
}

LikParams predictive_lik_params(const svgp_ctx* ctx, int lik, double param, int gh, bool clamp, double mean_const) {
  LikParams lp{};
  lp.lik = lik;
  lp.gh_n = gh;
  lp.sigma2 = (lik == SVGP_LIK_GAUSSIAN || lik == SVGP_LIK_GAMMA_EXP) ? param : 1.0;
  lp.digamma_alpha = 0.0;
  lp.gh_x = ctx->pred_gh.as<double>();
  lp.gh_w = ctx->pred_gh.as<double>() + gh;
  lp.clamp_neg_var = clamp ? 1 : 0;
  lp.mean_const = mean_const;
  return lp;
}

struct PredWant {
  bool lpd = false, ymean = false, yvar = false;
};

// the buffers of the point stage, before anything is enqueued
int reserve_predictive(svgp_ctx* ctx, int64_t len, const PredWant& w) {
  int rc = ctx->pred_part.reserve(ctx, (1024 * 3 + 4) * sizeof(double), "the predictive kernel's block sums");
  if (rc == SVGP_OK && (w.lpd || w.ymean || w.yvar)) rc = ctx->pred_out.reserve(ctx, 3 * size_t(len) * sizeof(double), "the predictive outputs");
  return rc;
}

// predictive_kernel + its reduce on the context's stream, and the copies of what was asked for (asynchronous: the caller synchronises)
int enqueue_predictive(svgp_ctx* ctx, int dtype, const LikParams& lp, const double* mom_mu, const double* mom_var, const void* y, int64_t off,
                       int64_t len, double var_shift, double sums3[3], double* lpd_out, double* ymean_out, double* yvar_out) {
  hipStream_t s = ctx->stream;
  double* part = ctx->pred_part.as<double>();
  double* dsum = part + 1024 * 3;
  double* po = ctx->pred_out.as<double>();
  double* d_lpd = (lpd_out && y) ? po : nullptr;
  double* d_ym = ymean_out ? po + len : nullptr;
  double* d_yv = yvar_out ? po + 2 * len : nullptr;
  launch_predictive(dtype, s, lp, mom_mu, mom_var, y, off, len, var_shift, part, dsum, d_lpd, d_ym, d_yv);
  KCHECK(ctx, "predictive");
  HIPC(ctx, hipMemcpyAsync(sums3, dsum, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (d_lpd) HIPC(ctx, hipMemcpyAsync(lpd_out, d_lpd, size_t(len) * 8, hipMemcpyDeviceToHost, s));
  if (d_ym) HIPC(ctx, hipMemcpyAsync(ymean_out, d_ym, size_t(len) * 8, hipMemcpyDeviceToHost, s));
  if (d_yv) HIPC(ctx, hipMemcpyAsync(yvar_out, d_yv, size_t(len) * 8, hipMemcpyDeviceToHost, s));
  return SVGP_OK;
}

void fill_pred_summary(svgp_pred_summary* out, const double sums3[3], int64_t len, bool clamp) {
  if (!out) return;
  out->sum_lpd = sums3[0];
  out->sum_sq_err = sums3[1];
  out->n_neg_var = int64_t(sums3[2]);
  out->n_points = len - (clamp ? 0 : out->n_neg_var);   // a clamped point counts, a bad one is left out of both sums
}
}  // namespace

extern "C" int32_t svgp_predictive(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, const svgp_point_mean* pm,
                                   svgp_pred_summary* summary_out, double* lpd_out, double* ymean_out, double* yvar_out) {
  int rc = check_batch(ctx, m, data, off, len, false);
  if (rc) return rc;
  const bool need_y = summary_out || lpd_out;
  if (need_y && !data->y.p) return fail(ctx, SVGP_INVALID_ARG, "data has no observations y: summary_out and lpd_out must be NULL");
  if (!summary_out && !lpd_out && !ymean_out && !yvar_out) return fail(ctx, SVGP_INVALID_ARG, "no output requested");
  rc = check_point_mean(ctx, pm);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  HIPC(ctx, hipSetDevice(ctx->device));
  const int gh = predictive_gh(m->desc.likelihood, m->desc.quadrature_n);
  rc = ensure_predictive_rule(ctx, gh);
  PredWant want{lpd_out != nullptr, ymean_out != nullptr, yvar_out != nullptr};
  if (rc == SVGP_OK) rc = reserve_predictive(ctx, len, want);
  const void* mux = nullptr;
  if (rc == SVGP_OK && pm) rc = stage_point_mean(ctx, pm, size_t(len) * m->es, &mux);
  if (rc) return rc;
  rc = elbo_enqueue(ctx, m, data, off, len, mux, true);
  if (rc) return rc;
  const bool clamp = m->desc.neg_var_policy == SVGP_NEGVAR_CLAMP;
  const LikParams lp = predictive_lik_params(ctx, m->desc.likelihood, m->desc.lik_sigma2, gh, clamp, m->desc.mean_const);
  double sums3[3] = {0, 0, 0};
  rc = enqueue_predictive(ctx, m->dtype, lp, ctx->mom_mu(), ctx->mom_var(), need_y ? data->y.p : nullptr, off, len, kDefaultSigma2, sums3,
                          lpd_out, ymean_out, yvar_out);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  TREC(ctx, ctx->ev[3], s);
  PrepScalars ps;
  HIPC(ctx, hipMemcpyAsync(ps.scal, m->scal.as<double>(), sizeof(ps.scal), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(&ps.info, m->info.as<int>(), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  finish_prep(m, ps);
  float t01 = 0, t12 = 0, t23 = 0, tch = 0;
  (void)elapsed_ms(ctx, &t01, ctx->ev[0], ctx->ev[1]);
  (void)elapsed_ms(ctx, &t12, ctx->ev[1], ctx->ev[2]);
  (void)elapsed_ms(ctx, &t23, ctx->ev[2], ctx->ev[3]);
  (void)elapsed_ms(ctx, &tch, ctx->ev_chol[0], ctx->ev_chol[1]);
  ctx->timing.ms_prep = t01;
  ctx->timing.ms_strip = t12;
  ctx->timing.ms_expect = t23;
  ctx->timing.ms_total = t01 + t12 + t23;
  ctx->timing.ms_kuf = 0;
  ctx->timing.ms_chol = tch;
  ctx->timing.ms_overlap = 0;
  if (ctx->overlapped) {
    float tov = 0;
    if (elapsed_ms(ctx, &tov, ctx->ev_ov[1], ctx->ev[1]) == hipSuccess && tov > 0) ctx->timing.ms_overlap = tov;
  }
  fill_pred_summary(summary_out, sums3, len, clamp);
  return status_of(ctx, m, sums3[2]);
}

extern "C" int32_t svgp_lik_predictive(svgp_ctx* ctx, int32_t likelihood, double lik_param_, int32_t quadrature_n, int64_t n, const double* mu,
                                       const double* var, const double* y, svgp_pred_summary* summary_out, double* lpd_out,
                                       double* ymean_out, double* yvar_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (likelihood < 0 || likelihood > SVGP_LIK_BERNOULLI_NORMCDF) return fail(ctx, SVGP_UNSUPPORTED, "unsupported likelihood");
  if (quadrature_n < 0 || quadrature_n > 512) return fail(ctx, SVGP_INVALID_ARG, "quadrature_n must be in 0..512");
  if (n < 1) return fail(ctx, SVGP_INVALID_ARG, "n must be >= 1");
  if (!mu || !var) return fail(ctx, SVGP_INVALID_ARG, "null marginals");
  if ((likelihood == SVGP_LIK_GAUSSIAN || likelihood == SVGP_LIK_GAMMA_EXP) && !(lik_param_ > 0))
    return fail(ctx, SVGP_INVALID_ARG, "the Gaussian likelihood needs sigma2 > 0, the Gamma likelihood a shape alpha > 0");
  if (!y && (summary_out || lpd_out)) return fail(ctx, SVGP_INVALID_ARG, "no observations y: summary_out and lpd_out must be NULL");
  if (!summary_out && !lpd_out && !ymean_out && !yvar_out) return fail(ctx, SVGP_INVALID_ARG, "no output requested");
  hipStream_t s = ctx->stream;
  HIPC(ctx, hipSetDevice(ctx->device));
  const int gh = predictive_gh(likelihood, quadrature_n);
  int rc = ensure_predictive_rule(ctx, gh);
  PredWant want{lpd_out != nullptr, ymean_out != nullptr, yvar_out != nullptr};
  if (rc == SVGP_OK) rc = reserve_predictive(ctx, n, want);
  if (rc == SVGP_OK) rc = ctx->pred_in.reserve(ctx, 3 * size_t(n) * sizeof(double), "the caller's marginals");
  if (rc) return rc;
  double* in = ctx->pred_in.as<double>();
  HIPC(ctx, hipMemcpyAsync(in, mu, size_t(n) * 8, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(in + n, var, size_t(n) * 8, hipMemcpyHostToDevice, s));
  if (y) HIPC(ctx, hipMemcpyAsync(in + 2 * n, y, size_t(n) * 8, hipMemcpyHostToDevice, s));
  TREC(ctx, ctx->ev[2], s);
  const LikParams lp = predictive_lik_params(ctx, likelihood, lik_param_, gh, false, 0.0);
  double sums3[3] = {0, 0, 0};
  rc = enqueue_predictive(ctx, SVGP_F64, lp, in, in + n, y ? in + 2 * n : nullptr, 0, n, 0.0, sums3, lpd_out, ymean_out, yvar_out);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  TREC(ctx, ctx->ev[3], s);
  HIPC(ctx, hipStreamSynchronize(s));
  float t23 = 0;
  (void)elapsed_ms(ctx, &t23, ctx->ev[2], ctx->ev[3]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_expect = t23;
  ctx->timing.ms_total = t23;
  fill_pred_summary(summary_out, sums3, n, false);
  if (sums3[2] > 0) {
    char buf[160];
    snprintf(buf, sizeof buf, "%lld predictive variances were negative (DomainError in sqrt)", (long long)sums3[2]);
    return fail(ctx, SVGP_NEG_VARIANCE, buf);
  }
  return SVGP_OK;
}
