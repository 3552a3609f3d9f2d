// predict_grad_api.hip — the predictive mean and variance with their input gradients: svgp_predictor_create / _eval / _state / _free
// (predict_grad.hip: the kernels).  Host orchestration only.
//   mu(x) = mean(x) + k(x, z) beta,     v(x) = k(x, x) + k(x, z) G k(z, x) + 1e-18,     G = Kuu^-1 (S_u - Kuu) Kuu^-1 = Lk^-T (S^ - I) Lk^-1
//   NonCentered: S^ = Lq Lq', beta = Lk^-T m;     Centered: S^ = Lk^-1 Lq Lq' Lk^-T, beta = Kuu^-1 (m - mean_const - muz)
// create: the model's usual prep (its status is svgp_elbo's), then the M-sized stage in fp64 for both dtypes - Kuu and its factor are
// built again in fp64 exactly as svgp_sampler_create builds them (sample_api.hip: an fp32 Lk's error is amplified by Kuu^-1), the
// explicit inverse factor by launch_linv, then with W = Lk^-T Lk^-1 and P = Lq' Lk^-1 (NonCentered) or Lq' W (Centered)
//   G = P' P - W
// which is exactly symmetric, and beta by two triangular solves.  G and beta are rounded once to the model dtype.
// eval: one launch of predict_grad_kernel per block of coordinates over the window.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>
#include <new>
#include <vector>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"
#include "predict_grad.hpp"

using namespace svgp;

extern "C" int32_t svgp_predictor_create(svgp_ctx* ctx, svgp_model* m, svgp_predictor** out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!out) return fail(ctx, SVGP_INVALID_ARG, "null out pointer");
  *out = nullptr;
  if (!m) return fail(ctx, SVGP_INVALID_ARG, "null model");
  HIPC(ctx, hipSetDevice(ctx->device));
  int rc = ensure_prepared(ctx, m);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const int dt = m->dtype, d = m->d;
  const int64_t M = m->M, Mp = m->Mp;
  const size_t es = m->es;
  std::unique_ptr<svgp_predictor> pp(new (std::nothrow) svgp_predictor());
  if (!pp) return SVGP_OOM;
  pp->dtype = dt;
  pp->d = d;
  pp->family = m->desc.kernel;
  pp->device = ctx->device;
  pp->es = es;
  pp->M = M;
  pp->Mp = Mp;
  pp->variance = m->desc.variance;
  pp->mean_const = m->desc.mean_const;
  // the inverse lengthscales the data stage uses, widened: an fp32 model rounds them to fp32 first (api.hip: upload_params)
  std::vector<double> invl64(size_t(d), 0.0);
  for (int f = 0; f < d; ++f) invl64[f] = dt == SVGP_F64 ? m->invl_host[f] : double(float(m->invl_host[f]));
  DevBuf d_invl64, zs64, K64, T64, info, LinvRM, LinvCM, Ytmp, Lq64, W64, P64;
  const size_t mm = size_t(Mp) * size_t(Mp) * 8;
  struct { DevBuf* b; size_t bytes; } req[] = {
      {&pp->invl, size_t(d) * es}, {&pp->rows, size_t(d) * size_t(Mp) * es}, {&pp->bias, size_t(Mp) * es}, {&pp->G, size_t(Mp) * size_t(Mp) * es},
      {&pp->beta, size_t(Mp) * es}, {&pp->G64, mm}, {&pp->beta64, size_t(Mp) * 8}, {&d_invl64, size_t(d) * 8},
      {&zs64, size_t(d) * size_t(Mp) * 8}, {&K64, mm}, {&T64, mm}, {&info, info_bytes(Mp)}, {&LinvRM, mm}, {&LinvCM, mm}, {&Ytmp, mm},
      {&Lq64, mm}, {&W64, mm}, {&P64, mm}};
  for (auto& r : req)
    if ((rc = r.b->reserve(ctx, r.bytes, "the predictor")) != SVGP_OK) return rc;
  HIPC(ctx, hipMemcpyAsync(d_invl64.p, invl64.data(), size_t(d) * 8, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(pp->invl.p, m->invl.p, size_t(d) * es, hipMemcpyDeviceToDevice, s));
  HIPC(ctx, hipMemsetAsync(T64.p, 0, mm, s));   // launch_potrf's contract: T zero above the diagonal
  HIPC(ctx, hipMemsetAsync(info.p, 0, info_bytes(Mp), s));
  HIPC(ctx, hipMemsetAsync(LinvRM.p, 0, mm, s));   // launch_linv writes the lower block triangle alone
  HIPC(ctx, hipMemsetAsync(LinvCM.p, 0, mm, s));
  // Kuu = Lk Lk' in fp64
  launch_sample_widen_z(dt, s, m->z_raw.p, m->desc.layout_z, d, M, Mp, d_invl64.as<double>(), zs64.as<double>());
  KernelParams kp;
  kp.family = m->desc.kernel;
  kp.d = d;
  kp.variance = m->desc.variance;
  kp.invl = d_invl64.p;
  launch_kuu(SVGP_F64, s, kp, zs64.p, M, Mp, m->desc.jitter, K64.p);
  launch_potrf(SVGP_F64, s, K64.p, T64.p, Mp, info.as<int>(), reinterpret_cast<unsigned*>(info.as<int>() + 1), ctx->num_cus);
  KCHECK(ctx, "predictor (Kuu, its factor)");
  launch_linv(SVGP_F64, s, K64.p, T64.p, Mp, LinvRM.p, LinvCM.p, Ytmp.p);
  KCHECK(ctx, "predictor (the inverse factor)");
  const int centered = m->desc.parametrization == SVGP_CENTERED ? 1 : 0;
  double* b64 = pp->beta64.as<double>();
  launch_pg_widen_q(dt, s, m->Lq_raw.p, m->m_raw.p, m->mu_z.p, M, Mp, centered, m->desc.mean_const, Lq64.as<double>(), b64);
  const double* Linv = LinvCM.as<double>();
  launch_pg_atb(s, Linv, Linv, nullptr, Mp, -1, 1, 1, W64.as<double>());                                            // W = Lk^-T Lk^-1
  launch_pg_atb(s, Lq64.as<double>(), centered ? W64.as<double>() : Linv, nullptr, Mp, -1, 1, centered ? 0 : 1, P64.as<double>());
  launch_pg_atb(s, P64.as<double>(), P64.as<double>(), W64.as<double>(), Mp, M, 0, 0, pp->G64.as<double>());       // G = P' P - W
  KCHECK(ctx, "predictor (G)");
  if (centered) launch_trsv2(SVGP_F64, s, K64.p, T64.p, Mp, 0, b64);
  launch_trsv2(SVGP_F64, s, K64.p, T64.p, Mp, 1, b64);
  launch_pg_round(dt, s, pp->G64.as<double>(), b64, Mp, pp->G.p, pp->beta.p);
  launch_sample_rows(dt, s, zs64.as<double>(), m->z_raw.p, m->desc.layout_z, M, nullptr, nullptr, d, 0, 0, Mp, pp->rows.p, pp->bias.p);
  KCHECK(ctx, "predictor (beta, rows)");
  int chol = 0;
  HIPC(ctx, hipMemcpyAsync(&chol, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));   // the workspace goes with this scope
  if (chol != 0) {
    char buf[160];
    snprintf(buf, sizeof buf, "Kuu is not positive definite: leading minor of order %d (PosDefException)", chol);
    return fail(ctx, SVGP_NOT_POSDEF, buf);
  }
  *out = pp.release();
  return SVGP_OK;
}

extern "C" int32_t svgp_predictor_eval(svgp_ctx* ctx, const svgp_predictor* pp, const svgp_data* data, int64_t off, int64_t len,
                                       const svgp_point_mean* pm, void* mean_out, void* var_out, void* mean_grad_out, void* var_grad_out,
                                       int64_t ldg, int32_t out_on_device) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!pp || !data) return fail(ctx, SVGP_INVALID_ARG, "null predictor or data");
  if (!mean_out && !var_out && !mean_grad_out && !var_grad_out) return fail(ctx, SVGP_INVALID_ARG, "no output requested");
  if (pp->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the predictor lives on another device than the context");
  if (data->dtype != pp->dtype) return fail(ctx, SVGP_INVALID_ARG, "data and predictor dtypes differ");
  if (data->d != pp->d) return fail(ctx, SVGP_INVALID_ARG, "data and predictor input dimensions differ");
  if (off < 0 || len < 1 || off + len > data->n) return fail(ctx, SVGP_INVALID_ARG, "window outside the data");
  if (ldg < len) return fail(ctx, SVGP_INVALID_ARG, "ldg must be >= len");
  if (out_on_device != 0 && out_on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "out_on_device must be 0 or 1");
  int rc = check_point_mean(ctx, pm);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t es = pp->es, row = size_t(len) * es, d = size_t(pp->d);
  // a host-output call's results on the device: mean | var | mean_grad [d][len] | var_grad [d][len]
  DevBuf& stage = ctx->smp_grad;
  if (!out_on_device && (rc = stage.reserve(ctx, (2 + 2 * d) * row, "the predictions")) != SVGP_OK) return rc;
  const void* mux = nullptr;
  if (mean_out && pm && (rc = stage_point_mean(ctx, pm, row, &mux)) != SVGP_OK) return rc;
  char* st = stage.as<char>();
  PredictGradArgs a{};
  a.rows = pp->rows.p;
  a.bias = pp->bias.p;
  a.G = pp->G.p;
  a.beta = pp->beta.p;
  a.invl = pp->invl.p;
  a.x = data->x.p;
  a.mux = mux;
  a.mean = !mean_out ? nullptr : out_on_device ? mean_out : st;
  a.var = !var_out ? nullptr : out_on_device ? var_out : st + row;
  a.mgrad = !mean_grad_out ? nullptr : out_on_device ? mean_grad_out : st + 2 * row;
  a.vgrad = !var_grad_out ? nullptr : out_on_device ? var_grad_out : st + (2 + d) * row;
  a.ldx = data->ldx;
  a.off = off;
  a.len = len;
  a.ldg = out_on_device ? ldg : len;
  a.Mp = pp->Mp;
  a.family = pp->family;
  a.d = pp->d;
  a.variance = pp->variance;
  a.mean_const = pp->mean_const;
  TREC(ctx, ctx->ev[0], s);
  launch_predict_grad(pp->dtype, s, a);
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "predict_grad");
  if (!out_on_device) {
    if (mean_out) HIPC(ctx, hipMemcpyAsync(mean_out, a.mean, row, hipMemcpyDeviceToHost, s));
    if (var_out) HIPC(ctx, hipMemcpyAsync(var_out, a.var, row, hipMemcpyDeviceToHost, s));
    if (mean_grad_out) HIPC(ctx, hipMemcpy2DAsync(mean_grad_out, size_t(ldg) * es, a.mgrad, row, row, d, hipMemcpyDeviceToHost, s));
    if (var_grad_out) HIPC(ctx, hipMemcpy2DAsync(var_grad_out, size_t(ldg) * es, a.vgrad, row, row, d, hipMemcpyDeviceToHost, s));
  }
  HIPC(ctx, hipStreamSynchronize(s));
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_strip = t;
  ctx->timing.ms_total = t;
  return SVGP_OK;
}

extern "C" int32_t svgp_predictor_state(svgp_ctx* ctx, const svgp_predictor* pp, double* beta_out, double* G_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!pp) return fail(ctx, SVGP_INVALID_ARG, "null predictor");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t row = size_t(pp->M) * 8;
  if (beta_out) HIPC(ctx, hipMemcpyAsync(beta_out, pp->beta64.p, row, hipMemcpyDeviceToHost, s));
  if (G_out) HIPC(ctx, hipMemcpy2DAsync(G_out, row, pp->G64.p, size_t(pp->Mp) * 8, row, size_t(pp->M), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

extern "C" int32_t svgp_predictor_free(svgp_ctx* ctx, svgp_predictor* pp) {
  if (!pp) return SVGP_OK;
  if (ctx) (void)hipSetDevice(ctx->device);
  delete pp;
  return SVGP_OK;
}
