// sample_api.hip — pathwise posterior function samples: svgp_sampler_create / _eval / _eval_grad / _state / _free (sample.hip, sample_grad.hip: the kernels).
// Host orchestration only.
//   f_s(.) = mean(.) + Phi(.) w_s + k(., z) V_s,     V_s = Kuu^-1 (u_s - mean(z) - Phi(z) w_s),     u_s ~ q(u) from the caller's eps_s
// create: the model's usual prep (its status is svgp_elbo's), then the M-sized stage in fp64 for both dtypes - Kuu and its factor are
// built again in fp64 from the widened z and parameters (the dtype-0 launchers of prep.hip), never taken from an fp32 Lk, whose error
// Kuu^-1 amplifies into the sample.  eval: one launch of sample_eval_kernel per block of <= 64 samples over the window.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <memory>
#include <new>
#include <vector>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"

using namespace svgp;

namespace {
// a host array of the basis on the device (model dtype), behind the stream
int upload(svgp_ctx* ctx, DevBuf& b, const void* host, size_t bytes, const char* what) {
  if (bytes == 0) return SVGP_OK;
  const int rc = b.reserve(ctx, bytes, what);
  if (rc) return rc;
  HIPC(ctx, hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return SVGP_OK;
}
}  // namespace

extern "C" int32_t svgp_sampler_create(svgp_ctx* ctx, svgp_model* m, const svgp_sample_basis* basis, svgp_sampler** out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!out) return fail(ctx, SVGP_INVALID_ARG, "null out pointer");
  *out = nullptr;
  if (!m || !basis) return fail(ctx, SVGP_INVALID_ARG, "null model or sample basis");
  const int64_t L = basis->n_features, S = basis->n_samples;
  if (S < 1) return fail(ctx, SVGP_INVALID_ARG, "n_samples must be >= 1");
  if (L < 0) return fail(ctx, SVGP_INVALID_ARG, "n_features must be >= 0");
  if (!basis->eps) return fail(ctx, SVGP_INVALID_ARG, "null eps");
  if (L > 0 && (!basis->omega || !basis->tau || !basis->w)) return fail(ctx, SVGP_INVALID_ARG, "null omega, tau or w with n_features > 0");
  HIPC(ctx, hipSetDevice(ctx->device));
  int rc = ensure_prepared(ctx, m);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const int dt = m->dtype, d = m->d;
  const int64_t M = m->M, Mp = m->Mp;
  const size_t es = m->es;
  std::unique_ptr<svgp_sampler> sp(new (std::nothrow) svgp_sampler());
  if (!sp) return SVGP_OOM;
  sp->dtype = dt;
  sp->d = d;
  sp->family = m->desc.kernel;
  sp->device = ctx->device;
  sp->es = es;
  sp->M = M;
  sp->Mp = Mp;
  sp->L = L;
  sp->Lp = (L + 31) / 32 * 32;
  sp->S = S;
  sp->Sp = (S + 15) / 16 * 16;
  sp->variance = m->desc.variance;
  sp->mean_const = m->desc.mean_const;
  const int64_t Lp = sp->Lp, Sp = sp->Sp, Kp = Lp + Mp;
  // the inverse lengthscales the data stage uses, widened: an fp32 model rounds them to fp32 first (api.hip: upload_params)
  std::vector<double> invl64(size_t(d), 0.0);
  for (int f = 0; f < d; ++f) invl64[f] = dt == SVGP_F64 ? m->invl_host[f] : double(float(m->invl_host[f]));
  DevBuf d_invl64, zs64, K64, T64, info, tmp, d_omega, d_tau, d_w, d_eps;
  const size_t mm = size_t(Mp) * size_t(Mp) * 8;
  struct { DevBuf* b; size_t bytes; } req[] = {
      {&sp->invl, size_t(d) * es}, {&sp->rows, size_t(d) * size_t(Kp) * es}, {&sp->bias, size_t(Kp) * es},
      {&sp->panel, size_t(Kp) * size_t(Sp) * es}, {&sp->u, size_t(S) * size_t(M) * 8}, {&sp->V, size_t(S) * size_t(Mp) * 8},
      {&d_invl64, size_t(d) * 8}, {&zs64, size_t(d) * size_t(Mp) * 8}, {&K64, mm}, {&T64, mm}, {&info, info_bytes(Mp)},
      {&tmp, size_t(S) * size_t(Mp) * 8}};
  for (auto& r : req)
    if ((rc = r.b->reserve(ctx, r.bytes, "the sampler")) != SVGP_OK) return rc;
  if ((rc = upload(ctx, d_omega, basis->omega, size_t(L) * size_t(d) * es, "the sampler's frequencies")) != SVGP_OK) return rc;
  if ((rc = upload(ctx, d_tau, basis->tau, size_t(L) * es, "the sampler's phases")) != SVGP_OK) return rc;
  if ((rc = upload(ctx, d_w, basis->w, size_t(S) * size_t(L) * es, "the sampler's feature weights")) != SVGP_OK) return rc;
  if ((rc = upload(ctx, d_eps, basis->eps, size_t(S) * size_t(M) * es, "the sampler's draws for q(u)")) != SVGP_OK) return rc;
  HIPC(ctx, hipMemcpyAsync(d_invl64.p, invl64.data(), size_t(d) * 8, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipMemcpyAsync(sp->invl.p, m->invl.p, size_t(d) * es, hipMemcpyDeviceToDevice, s));
  HIPC(ctx, hipMemsetAsync(T64.p, 0, mm, s));   // launch_potrf's contract: T zero above the diagonal
  HIPC(ctx, hipMemsetAsync(info.p, 0, info_bytes(Mp), s));
  // Kuu = Lk Lk' in fp64
  launch_sample_widen_z(dt, s, m->z_raw.p, m->desc.layout_z, d, M, Mp, d_invl64.as<double>(), zs64.as<double>());
  KernelParams kp;
  kp.family = m->desc.kernel;
  kp.d = d;
  kp.variance = m->desc.variance;
  kp.invl = d_invl64.p;
  launch_kuu(SVGP_F64, s, kp, zs64.p, M, Mp, m->desc.jitter, K64.p);
  launch_potrf(SVGP_F64, s, K64.p, T64.p, Mp, info.as<int>(), reinterpret_cast<unsigned*>(info.as<int>() + 1), ctx->num_cus);
  KCHECK(ctx, "sampler (Kuu, its factor)");
  // u_s - mean(z), then minus Phi(z) w_s, then V_s = Lk^-T Lk^-1 of it, one right-hand side after the other (a fixed order)
  const double amp = L > 0 ? std::sqrt(2.0 * m->desc.variance / double(L)) : 0.0;
  double* V = sp->V.as<double>();
  launch_sample_u(dt, s, m->m_raw.p, m->Lq_raw.p, d_eps.p, m->mu_z.p, K64.as<double>(), M, Mp, S, m->desc.parametrization == SVGP_CENTERED ? 1 : 0,
                  m->desc.mean_const, tmp.as<double>(), V, sp->u.as<double>());
  launch_sample_phiz(dt, s, zs64.as<double>(), d_omega.p, d_tau.p, d_w.p, d, M, L, S, Mp, amp, V);
  KCHECK(ctx, "sampler (u, Phi(z) w)");
  for (int64_t j = 0; j < S; ++j) {
    launch_trsv2(SVGP_F64, s, K64.p, T64.p, Mp, 0, V + j * Mp);
    launch_trsv2(SVGP_F64, s, K64.p, T64.p, Mp, 1, V + j * Mp);
  }
  KCHECK(ctx, "sampler (V)");
  launch_sample_rows(dt, s, zs64.as<double>(), m->z_raw.p, m->desc.layout_z, M, d_omega.p, d_tau.p, d, L, Lp, Mp, sp->rows.p, sp->bias.p);
  launch_sample_panel(dt, s, d_w.p, V, L, Lp, M, Mp, S, Sp, amp, sp->panel.p);
  KCHECK(ctx, "sampler (panel)");
  int chol = 0;
  HIPC(ctx, hipMemcpyAsync(&chol, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));   // the caller's host arrays may be released; the workspace goes with this scope
  if (chol != 0) {
    char buf[160];
    snprintf(buf, sizeof buf, "Kuu is not positive definite: leading minor of order %d (PosDefException)", chol);
    return fail(ctx, SVGP_NOT_POSDEF, buf);
  }
  *out = sp.release();
  return SVGP_OK;
}

extern "C" int32_t svgp_sampler_eval(svgp_ctx* ctx, const svgp_sampler* sp, const svgp_data* data, int64_t off, int64_t len,
                                     const svgp_point_mean* pm, void* out, int64_t ldo, int32_t out_on_device) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!sp || !data) return fail(ctx, SVGP_INVALID_ARG, "null sampler or data");
  if (!out) return fail(ctx, SVGP_INVALID_ARG, "null output");
  if (sp->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the sampler lives on another device than the context");
  if (data->dtype != sp->dtype) return fail(ctx, SVGP_INVALID_ARG, "data and sampler dtypes differ");
  if (data->d != sp->d) return fail(ctx, SVGP_INVALID_ARG, "data and sampler input dimensions differ");
  if (off < 0 || len < 1 || off + len > data->n) return fail(ctx, SVGP_INVALID_ARG, "window outside the data");
  if (ldo < len) return fail(ctx, SVGP_INVALID_ARG, "ldo must be >= len");
  if (out_on_device != 0 && out_on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "out_on_device must be 0 or 1");
  int rc = check_point_mean(ctx, pm);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t es = sp->es;
  if (!out_on_device && (rc = ctx->smp_out.reserve(ctx, size_t(sp->S) * size_t(len) * es, "the samples")) != SVGP_OK) return rc;
  const void* mux = nullptr;
  if (pm && (rc = stage_point_mean(ctx, pm, size_t(len) * es, &mux)) != SVGP_OK) return rc;
  SampleEvalArgs a{};
  a.rows = sp->rows.p;
  a.bias = sp->bias.p;
  a.panel = sp->panel.p;
  a.invl = sp->invl.p;
  a.x = data->x.p;
  a.mux = mux;
  a.out = out_on_device ? out : ctx->smp_out.p;
  a.ldx = data->ldx;
  a.off = off;
  a.len = len;
  a.ldo = out_on_device ? ldo : len;
  a.Lp = sp->Lp;
  a.Mp = sp->Mp;
  a.S = sp->S;
  a.Sp = sp->Sp;
  a.family = sp->family;
  a.d = sp->d;
  a.variance = sp->variance;
  a.mean_const = sp->mean_const;
  TREC(ctx, ctx->ev[0], s);
  launch_sample_eval(sp->dtype, s, a);
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "sample_eval");
  if (!out_on_device)
    HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * es, ctx->smp_out.p, size_t(len) * es, size_t(len) * es, size_t(sp->S), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_strip = t;
  ctx->timing.ms_total = t;
  return SVGP_OK;
}

// the values (optional) and the input gradient of the samples over a window: the launches of sample_grad.hip, one per 16 samples and
// 8 coordinates; the values are written by the first coordinate block of each column block, through svgp_sampler_eval's own chain
extern "C" int32_t svgp_sampler_eval_grad(svgp_ctx* ctx, const svgp_sampler* sp, const svgp_data* data, int64_t off, int64_t len,
                                          const svgp_point_mean* pm, void* out, int64_t ldo, void* grad_out, int64_t ldg,
                                          int32_t out_on_device) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!sp || !data) return fail(ctx, SVGP_INVALID_ARG, "null sampler or data");
  if (!grad_out) return fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  if (sp->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the sampler lives on another device than the context");
  if (data->dtype != sp->dtype) return fail(ctx, SVGP_INVALID_ARG, "data and sampler dtypes differ");
  if (data->d != sp->d) return fail(ctx, SVGP_INVALID_ARG, "data and sampler input dimensions differ");
  if (off < 0 || len < 1 || off + len > data->n) return fail(ctx, SVGP_INVALID_ARG, "window outside the data");
  if (out && ldo < len) return fail(ctx, SVGP_INVALID_ARG, "ldo must be >= len");
  if (ldg < len) return fail(ctx, SVGP_INVALID_ARG, "ldg must be >= len");
  if (out_on_device != 0 && out_on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "out_on_device must be 0 or 1");
  int rc = check_point_mean(ctx, pm);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t es = sp->es;
  const size_t grows = size_t(sp->S) * size_t(sp->d);   // rows of the gradient: (s, c)
  if (!out_on_device) {
    if (out && (rc = ctx->smp_out.reserve(ctx, size_t(sp->S) * size_t(len) * es, "the samples")) != SVGP_OK) return rc;
    if ((rc = ctx->smp_grad.reserve(ctx, grows * size_t(len) * es, "the samples' gradients")) != SVGP_OK) return rc;
  }
  const void* mux = nullptr;
  if (out && pm && (rc = stage_point_mean(ctx, pm, size_t(len) * es, &mux)) != SVGP_OK) return rc;
  SampleGradArgs g{};
  SampleEvalArgs& a = g.v;
  a.rows = sp->rows.p;
  a.bias = sp->bias.p;
  a.panel = sp->panel.p;
  a.invl = sp->invl.p;
  a.x = data->x.p;
  a.mux = mux;
  a.out = !out ? nullptr : out_on_device ? out : ctx->smp_out.p;
  a.ldx = data->ldx;
  a.off = off;
  a.len = len;
  a.ldo = out_on_device ? ldo : len;
  a.Lp = sp->Lp;
  a.Mp = sp->Mp;
  a.S = sp->S;
  a.Sp = sp->Sp;
  a.family = sp->family;
  a.d = sp->d;
  a.variance = sp->variance;
  a.mean_const = sp->mean_const;
  g.grad = out_on_device ? grad_out : ctx->smp_grad.p;
  g.ldg = out_on_device ? ldg : len;
  TREC(ctx, ctx->ev[0], s);
  launch_sample_grad(sp->dtype, s, g);
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "sample_grad");
  if (!out_on_device) {
    if (out)
      HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * es, ctx->smp_out.p, size_t(len) * es, size_t(len) * es, size_t(sp->S), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipMemcpy2DAsync(grad_out, size_t(ldg) * es, ctx->smp_grad.p, size_t(len) * es, size_t(len) * es, grows, hipMemcpyDeviceToHost, s));
  }
  HIPC(ctx, hipStreamSynchronize(s));
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_strip = t;
  ctx->timing.ms_total = t;
  return SVGP_OK;
}

extern "C" int32_t svgp_sampler_state(svgp_ctx* ctx, const svgp_sampler* sp, double* u_out, double* V_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!sp) return fail(ctx, SVGP_INVALID_ARG, "null sampler");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t row = size_t(sp->M) * 8;
  if (u_out) HIPC(ctx, hipMemcpyAsync(u_out, sp->u.p, size_t(sp->S) * row, hipMemcpyDeviceToHost, s));
  if (V_out) HIPC(ctx, hipMemcpy2DAsync(V_out, row, sp->V.p, size_t(sp->Mp) * 8, row, size_t(sp->S), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

extern "C" int32_t svgp_sampler_free(svgp_ctx* ctx, svgp_sampler* sp) {
  if (!sp) return SVGP_OK;
  if (ctx) (void)hipSetDevice(ctx->device);
  delete sp;
  return SVGP_OK;
}
