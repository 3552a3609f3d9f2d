// api_qopt.hip — the calls that put the optimal or a natural-gradient q(u) on the model: svgp_collapsed_bound / _q / _grad and
// svgp_natgrad_step / _ext.  They share the fp64 workspace and the M-sized tail (collapsed.hip / natgrad.hip hold the kernels).
// Host orchestration only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"

using namespace svgp;

// ================================================================================================
// The collapsed (Titsias 2009) bound of sparse GP regression and the optimal q(u): svgp_collapsed_bound / _q / _grad.
// With Kuu = Lk Lk', A = Lk \ Kuf, r = y - mean_const:  C = A A', b = A r, t = tr C, rr = r'r (sums over the batch window),
//   B = I + C / sigma^2 = LB LB',  c = LB \ b / sigma^2,
//   bound = -n/2 log(2 pi sigma^2) - sum log diag LB - rr / (2 sigma^2) + c'c / 2 - (n variance - t) / (2 sigma^2)
//   whitened optimum: m_w = LB' \ c, S_w = B^-1 (Lq_w = its lower Cholesky factor); centered: m = mean_const + Lk m_w, Lq = Lk Lq_w.
// Schedule: the model's own prep (Kuu, Lk, the T panels), then per chunk of <= 65 536 points (the gradient's chunking and workspace):
// phase 1 of the strips alone (strip.hip: trsm_pm_kernel) leaves A point-major and sum A^2 per point, the uniform-weight SYRK
// accumulates C in the gradient's slice buffer, collapsed_reduce_kernel accumulates b, rr, t from the resident chunk.  Only that chunk
// of A lives in HBM.  The M-sized tail runs in fp64 whatever the model's dtype (collapsed.hip).
// svgp_collapsed_*_with_noise (CollapsedExt): per-point noise variances sigma_j^2 = sigma^2 + s_j and prior mean offsets mux, muz.
//   w_j = 1 / sigma_j^2, r_j = y_j - mean_const - mux_j, C = sum w_j a_j a_j', b = sum w_j a_j r_j, rr = sum w_j r_j^2,
//   t_w = sum w_j |a_j|^2, sw = sum w_j, ld = sum log sigma_j^2, B = I + C, c = LB \ b
//   bound = -n/2 log(2 pi) - ld / 2 - sum log diag LB - rr / 2 + c'c / 2 - (variance sw - t_w) / 2;  Centered m += muz
// Schedule with s: one launch writes the window's weights (and counts sigma_j^2 <= 0, read with the pivot check's status: nothing of
// the data pass runs on a bad vector), the chunk's C comes from the weighted SYRK of the non-Gaussian value-and-gradient
// (launch_gemm_pm with w), b / rr / t_w / sw / ld from collapsed_reduce_w_kernel; the tail is the same with sigma^2 = 1.  With mux
// alone the SYRK stays the uniform one and only the reduction changes.  Without either, the launches and their arguments are the
// plain calls'.
namespace {

// what a _with_noise call adds: the window's offsets and noise variances ON THE DEVICE (NULL: absent), muz of the model into the Centered m
struct CollapsedExt {
  const void* mux = nullptr;
  const void* sv = nullptr;
  bool muz = false;
};

int collapsed_workspace(svgp_ctx* ctx, int64_t Mp, CollapsedWs** out) {
  CollapsedWs* c = ctx->cws;
  if (c && c->Mp == Mp) { *out = c; return SVGP_OK; }
  if (c) (void)hipStreamSynchronize(ctx->stream);
  delete c;
  ctx->cws = nullptr;
  c = new (std::nothrow) CollapsedWs();
  if (!c) return SVGP_OOM;
  c->Mp = Mp;
  const size_t mm = size_t(Mp) * size_t(Mp) * 8;
  struct { DevBuf* p; size_t b; } req[] = {
      {&c->Bm, mm}, {&c->TB, mm}, {&c->LinvRM, mm}, {&c->LinvCM, mm}, {&c->Ytmp, mm}, {&c->Sinv, mm},
      {&c->cvec, size_t(Mp) * 8}, {&c->mw, size_t(Mp) * 8}, {&c->bpart, size_t(kCollapsedSplit) * size_t(Mp) * 8},
      {&c->spart, size_t(kCollapsedSplit) * 2 * 8}, {&c->spart2, size_t(kCollapsedSplit) * 2 * 8}, {&c->scal, 64}, {&c->info_b, info_bytes(Mp)}, {&c->info_s, info_bytes(Mp)},
      {&c->gemv_part, size_t(Mp / 128) * size_t(Mp) * 8}};
  for (auto& r : req)
    if (r.p->alloc(r.b) != hipSuccess) {
      delete c;
      return alloc_failed(ctx, "for the collapsed bound's workspace");
    }
  // launch_potrf's contract: T zero above the diagonal; launch_linv writes the block-lower part only (the rest must be finite)
  for (void* p : {c->TB.p, c->LinvRM.p, c->LinvCM.p})
    if (hipMemsetAsync(p, 0, mm, ctx->stream) != hipSuccess) {
      delete c;
      return fail(ctx, SVGP_HIP_ERROR, "memset failed");
    }
  ctx->cws = c;
  *out = c;
  return SVGP_OK;
}

// argument checks of the three calls, before anything is enqueued
int collapsed_check(svgp_ctx* ctx, const svgp_model* m, const svgp_data* data, int64_t off, int64_t len, bool allow_muz = false) {
  int rc = check_batch(ctx, m, data, off, len, true);
  if (rc) return rc;
  if (m->desc.likelihood != SVGP_LIK_GAUSSIAN)
    return fail(ctx, SVGP_INVALID_ARG, "the collapsed bound needs the Gaussian likelihood (SVGP_LIK_GAUSSIAN)");
  if (ctx->comm) return fail(ctx, SVGP_UNSUPPORTED, "the collapsed bound is not collective: detach the communicator");
  if (m->mu_z.p && !allow_muz) return fail(ctx, SVGP_UNSUPPORTED, "the collapsed bound takes no prior mean offsets (svgp_model_set_mean_z)");
  return SVGP_OK;
}

void collapsed_terms_clear(svgp_collapsed_terms* t) {
  if (!t) return;
  *t = svgp_collapsed_terms{};
  t->bound = t->fit = t->trace = t->logdet_B = t->logdet_kuu = NAN;
}

// S = Linv' Linv = inv(L L') in fp64 from the explicit inverse of the lower-triangular L (whose inverted diagonal blocks are in c->TB),
// into c->Sinv; with info_s, also its lower Cholesky factor in place (info_s cleared first; c->TB then holds THAT factor's panels).
// (L^-T is UPPER triangular: not the factor.)
int inverse_product_factor(svgp_ctx* ctx, CollapsedWs* c, const void* L, int* info_s) {
  hipStream_t s = ctx->stream;
  const int64_t Mp = c->Mp;
  launch_linv(SVGP_F64, s, L, c->TB.p, Mp, c->LinvRM.p, c->LinvCM.p, c->Ytmp.p);
  launch_gemm_pm(SVGP_F64, s, c->LinvRM.p, c->LinvRM.p, nullptr, 1.0, Mp, Mp, Mp, 1, c->Sinv.p, 1, kMmFull | kMmXLow | kMmYLow);
  if (!info_s) return SVGP_OK;
  HIPC(ctx, hipMemsetAsync(info_s, 0, info_bytes(Mp), s));
  launch_potrf(SVGP_F64, s, c->Sinv.p, c->TB.p, Mp, info_s, reinterpret_cast<unsigned*>(info_s + 1), ctx->num_cus);
  return SVGP_OK;
}

// the model's device-resident m / Lq (what a call of this unit has just written) into the caller's host arrays, each nullable
int read_back_q(svgp_ctx* ctx, const svgp_model* m, void* m_out, void* Lq_out) {
  if (m_out) HIPC(ctx, hipMemcpyAsync(m_out, m->m_raw.p, size_t(m->M) * m->es, hipMemcpyDeviceToHost, ctx->stream));
  if (Lq_out) HIPC(ctx, hipMemcpyAsync(Lq_out, m->Lq_raw.p, size_t(m->M) * size_t(m->M) * m->es, hipMemcpyDeviceToHost, ctx->stream));
  if (m_out || Lq_out) HIPC(ctx, hipStreamSynchronize(ctx->stream));
  return SVGP_OK;
}

// prep + data pass + tail (+ the optimal q into the model's m / Lq when want_q) + read-back
int collapsed_run(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, bool want_q, double* bound_out,
                  svgp_collapsed_terms* terms_out, const CollapsedExt* ext = nullptr) {
  collapsed_terms_clear(terms_out);
  if (bound_out) *bound_out = NAN;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  int rc = ensure_prepared(ctx, m);
  if (terms_out) terms_out->chol_info = m->chol_info;
  if (rc) return rc;
  GradWs* w = nullptr;
  rc = grad_workspace(ctx, m, len, &w);
  if (rc) return rc;
  CollapsedWs* c = nullptr;
  rc = collapsed_workspace(ctx, m->Mp, &c);
  if (rc) return rc;
  const int dt = m->dtype;
  const int64_t Mp = m->Mp, M = m->M;
  const void* mux = ext ? ext->mux : nullptr;
  const void* sv = ext ? ext->sv : nullptr;
  const bool weighted = sv != nullptr, reduce_w = mux || sv;
  const int64_t len128 = (len + 127) / 128 * 128;
  int* nbad_dev = nullptr;
  if (weighted) {   // the window's weights, once (+ 256 bytes: the SYRK's weight DMA reads 256 B at a time)
    if ((rc = ctx->pn_w.reserve(ctx, size_t(len128) * m->es + 256, "the per-point weights")) != SVGP_OK) return rc;
    if ((rc = ctx->pn_wd.reserve(ctx, size_t(len128) * 8 + 256, "the per-point weights")) != SVGP_OK) return rc;
    nbad_dev = reinterpret_cast<int*>(ctx->pn_wd.as<double>() + len128);
    HIPC(ctx, hipMemsetAsync(nbad_dev, 0, sizeof(int), s));
    launch_collapsed_weights(dt, s, sv, m->desc.lik_sigma2, len, len128, ctx->pn_w.p, ctx->pn_wd.as<double>(), nbad_dev);
    KCHECK(ctx, "collapsed weights");
  }
  {
    // cholesky(Kuu) reports pivots <= 0 only (LAPACK's rule, every existing call's); A = Lk \ Kuf on a pivot that is rounding noise - an
    // exactly repeated inducing point at jitter 0 - is noise itself, so here such a pivot counts as non-positive too
    int first_bad = 0;
    launch_collapsed_pivot_check(dt, s, m->L.p, M, Mp, m->desc.variance + m->desc.jitter, c->info_s.as<int>());
    KCHECK(ctx, "collapsed pivot check");
    HIPC(ctx, hipMemcpyAsync(&first_bad, c->info_s.p, sizeof(int), hipMemcpyDeviceToHost, s));
    int nbad = 0;
    if (weighted) HIPC(ctx, hipMemcpyAsync(&nbad, nbad_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    if (first_bad != 0) {
      if (terms_out) terms_out->chol_info = first_bad;
      char buf[200];
      snprintf(buf, sizeof buf, "Kuu is not positive definite to working precision: pivot %d is at or below its rounding noise (PosDefException)", first_bad);
      return fail(ctx, SVGP_NOT_POSDEF, buf);
    }
    if (nbad != 0) {
      char buf[200];
      snprintf(buf, sizeof buf, "the noise covariance is not positive definite: %d of the variances lik_sigma2 + s_j are <= 0 (PosDefException)", nbad);
      return fail(ctx, SVGP_NOT_POSDEF, buf);
    }
  }
  const size_t es = m->es;
  const int64_t nc = std::min<int64_t>(w->nc, grad_chunk_points(Mp, es, len));   // the chunking is a function of the call (as the gradient's)
  const int ns_syrk = std::min(w->nslices, syrk_slices(ctx, m, nc));
  rc = ensure_scratch(ctx, chunk_work_bytes(ctx, dt, Mp, len, nc), size_t(nc));
  if (rc) return rc;
  double* bpart = c->bpart.as<double>();
  double* spart = c->spart.as<double>();
  double* scal = c->scal.as<double>();
  for (int64_t c0 = 0; c0 < len; c0 += nc) {
    const int64_t clen = (len - c0 < nc) ? len - c0 : nc;
    const int64_t ncp = (clen + 127) / 128 * 128;
    const SinglePlan p = single_plan(dt, Mp, clen, ctx->num_cus);
    StripArgs a = strip_args(ctx, m, data->x.p, data->ldx, off + c0, clen);
    a.At_out = w->At.p;
    HIPC(ctx, hipMemsetAsync(a.counter, 0, sizeof(unsigned), s));
    launch_trsm_point_major(dt, s, a, p.nt, p.grid, p.nstrips);
    KCHECK(ctx, "strip (phase 1, point-major A)");
    // columns of the chunk's last strip beyond its last point hold the replicated last point: zero them up to the SYRK's k-step boundary
    const int64_t n16 = (clen + 15) / 16 * 16;
    if (n16 > clen) HIPC(ctx, hipMemsetAsync(static_cast<char*>(w->At.p) + size_t(clen) * size_t(Mp) * es, 0, size_t(n16 - clen) * size_t(Mp) * es, s));
    const int64_t sl = ((ncp + ns_syrk - 1) / ns_syrk + 15) / 16 * 16;
    if (!weighted) {
      launch_syrk_uniform(dt, s, w->At.p, 1.0, 1.0, nullptr, 0.0, 1.0, Mp, n16, sl, ns_syrk, w->G1.p, c0 == 0 ? 1 : 0);   // C (+)= A A'
    } else {
      // C (+)= A diag(w) A': the weighted loop runs over the chunk padded to 128 points against zero weights - and zero rows of A
      if (ncp > n16) HIPC(ctx, hipMemsetAsync(static_cast<char*>(w->At.p) + size_t(n16) * size_t(Mp) * es, 0, size_t(ncp - n16) * size_t(Mp) * es, s));
      launch_gemm_pm(dt, s, w->At.p, w->At.p, ctx->pn_w.as<char>() + size_t(c0) * es, 1.0, Mp, ncp, sl, ns_syrk, w->G1.p, c0 == 0 ? 1 : 0);
    }
    KCHECK(ctx, "syrk (C = A A')");
    if (!reduce_w) {
      launch_collapsed_reduce(dt, s, w->At.p, data->y.p, a.mom_var, Mp, off + c0, clen, m->desc.mean_const, c0 == 0 ? 1 : 0, bpart, spart);
    } else {
      launch_collapsed_reduce_w(dt, s, w->At.p, data->y.p, mux ? static_cast<const char*>(mux) + size_t(c0) * es : nullptr,
                                sv ? static_cast<const char*>(sv) + size_t(c0) * es : nullptr, weighted ? ctx->pn_wd.as<double>() + c0 : nullptr,
                                a.mom_var, Mp, off + c0, clen, m->desc.mean_const, m->desc.lik_sigma2, c0 == 0 ? 1 : 0, bpart, spart,
                                c->spart2.as<double>());
    }
    KCHECK(ctx, "collapsed reduce (b, rr, t)");
  }
  // ---- M-sized tail, fp64 ----
  const double sigma2 = m->desc.lik_sigma2;
  int* info_b = c->info_b.as<int>();
  int* info_s = c->info_s.as<int>();
  // (with per-point noise the weights are inside C and b already: no 1 / sigma^2 scaling)
  launch_collapsed_form_b(dt, s, w->G1.p, ns_syrk, Mp, weighted ? 1.0 : sigma2, bpart, spart, c->Bm.as<double>(), c->cvec.as<double>(), scal);
  if (weighted) launch_collapsed_extra(s, c->spart2.as<double>(), scal);
  HIPC(ctx, hipMemsetAsync(info_b, 0, info_bytes(Mp), s));
  launch_potrf(SVGP_F64, s, c->Bm.p, c->TB.p, Mp, info_b, reinterpret_cast<unsigned*>(info_b + 1), ctx->num_cus);
  launch_trsv2(SVGP_F64, s, c->Bm.p, c->TB.p, Mp, 0, c->cvec.p);   // c = LB \ b / sigma^2
  KCHECK(ctx, "collapsed tail (cholesky(B), c)");
  if (!want_q) {
    launch_collapsed_scal(s, c->Bm.as<double>(), c->cvec.as<double>(), Mp, info_b, nullptr, scal);
  } else {
    HIPC(ctx, hipMemcpyAsync(c->mw.p, c->cvec.p, size_t(Mp) * 8, hipMemcpyDeviceToDevice, s));
    launch_trsv2(SVGP_F64, s, c->Bm.p, c->TB.p, Mp, 1, c->mw.p);   // m_w = LB' \ c
    launch_collapsed_scal(s, c->Bm.as<double>(), c->cvec.as<double>(), Mp, info_b, nullptr, scal);   // (reads LB before its T panels are reused)
    // B^-1 = LBinv' LBinv from the explicit triangular inverse; Lq_w = its lower Cholesky factor (LB^-T is UPPER triangular: not it)
    rc = inverse_product_factor(ctx, c, c->Bm.p, info_s);
    if (rc) return rc;
    launch_collapsed_scal(s, c->Bm.as<double>(), c->cvec.as<double>(), Mp, info_b, info_s, scal);
    KCHECK(ctx, "collapsed tail (B^-1, its factor)");
    // device to device into the model's own m / Lq (nothing is written when a factorisation failed); the model is prepared again, lazily
    launch_collapsed_write_q(dt, s, c->Sinv.as<double>(), c->mw.as<double>(), m->L.p, M, Mp, m->desc.parametrization == SVGP_CENTERED ? 1 : 0,
                             m->desc.mean_const, scal, info_b, info_s, (ext && ext->muz) ? m->mu_z.p : nullptr, m->m_raw.p, m->Lq_raw.p);
    KCHECK(ctx, "collapsed q");
    m->prepared = false;
  }
  double h[8] = {};
  HIPC(ctx, hipMemcpyAsync(h, scal, (weighted ? 8 : 6) * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  const double rr = h[0], t = h[1], sld = h[2], cc = h[3];
  const bool nan_in = std::isnan(rr) || std::isnan(t);   // a NaN coordinate / observation: NaN results, SVGP_OK (the rule of svgp_elbo)
  const int ib = nan_in ? 0 : int(h[4]), is = nan_in ? 0 : int(h[5]);
  const double n = double(len);
  double fit = -0.5 * n * std::log(2.0 * M_PI * sigma2) - sld - rr / (2.0 * sigma2) + 0.5 * cc;
  double trace = -(n * m->desc.variance - t) / (2.0 * sigma2);
  if (weighted) {   // rr, t carry the weights; h[6] = sum log sigma_j^2, h[7] = sum w_j
    fit = -0.5 * n * std::log(2.0 * M_PI) - 0.5 * h[6] - sld - 0.5 * rr + 0.5 * cc;
    trace = -0.5 * (m->desc.variance * h[7] - t);
  }
  const bool bad = ib != 0 || is != 0;
  if (terms_out) {
    terms_out->n_points = len;
    terms_out->logdet_kuu = m->logdet_kuu;
    terms_out->chol_info_b = ib ? ib : is;
    if (!bad) {
      terms_out->bound = nan_in ? NAN : fit + trace;
      terms_out->fit = nan_in ? NAN : fit;
      terms_out->trace = nan_in ? NAN : trace;
      terms_out->logdet_B = nan_in ? NAN : 2.0 * sld;
    }
  }
  if (bad) {
    char buf[200];
    snprintf(buf, sizeof buf, "%s is not positive definite: leading minor of order %d (PosDefException)",
             ib ? (weighted ? "B = I + A diag(1 / sigma_j^2) A'" : "B = I + A A' / sigma^2") : "inv(B) of the optimal q", ib ? ib : is);
    return fail(ctx, SVGP_NOT_POSDEF, buf);
  }
  if (bound_out) *bound_out = nan_in ? NAN : fit + trace;
  return SVGP_OK;
}

}  // namespace

extern "C" int32_t svgp_collapsed_bound(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double* bound_out,
                                        svgp_collapsed_terms* terms_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  const int rc = collapsed_check(ctx, m, data, off, len);
  if (rc) return rc;
  return collapsed_run(ctx, m, data, off, len, false, bound_out, terms_out);
}

extern "C" int32_t svgp_collapsed_q(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, void* m_out, void* Lq_out,
                                    double* bound_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = collapsed_check(ctx, m, data, off, len);
  if (rc) return rc;
  rc = collapsed_run(ctx, m, data, off, len, true, bound_out, nullptr);
  if (rc) return rc;
  return read_back_q(ctx, m, m_out, Lq_out);
}

extern "C" int32_t svgp_collapsed_grad(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double* bound_out,
                                       svgp_collapsed_terms* terms_out, svgp_grads* g, const svgp_input_grad* gx) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = collapsed_check(ctx, m, data, off, len);
  if (rc) return rc;
  if (!g) return fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  if (g->m || g->Lq) return fail(ctx, SVGP_INVALID_ARG, "svgp_collapsed_grad: grads_out->m and grads_out->Lq must be NULL (zero at the optimal q)");
  if (gx && (rc = check_input_grad(ctx, data, len, gx)) != SVGP_OK) return rc;
  double bound = NAN;
  rc = collapsed_run(ctx, m, data, off, len, true, &bound, terms_out);
  if (rc) return rc;
  // d elbo / d q = 0 at the optimal q: the ELBO's partial derivatives in the hyperparameters and z there are the bound's total ones
  double elbo2 = NAN;
  GradRequest rq;   // scale 1, KL weight 1, local
  rq.num_data = double(len);
  rq.gx = gx;
  rc = elbo_grad_impl(ctx, m, data, off, len, rq, &elbo2, nullptr, g);
  if (rc) return rc;
  if (bound_out) *bound_out = bound;
  return SVGP_OK;
}

// ---- svgp_collapsed_*_with_noise -----------------------------------------------------------------------------------------------
namespace {

int check_point_noise(svgp_ctx* ctx, const svgp_point_noise* pn) {
  if (!pn) return SVGP_OK;
  if (!pn->s) return fail(ctx, SVGP_INVALID_ARG, "null per-point noise variances");
  if ((pn->on_device != 0 && pn->on_device != 1) || pn->reserved != 0)
    return fail(ctx, SVGP_INVALID_ARG, "per-point noise: on_device must be 0 or 1 and reserved 0");
  return SVGP_OK;
}

// (before anything is enqueued; device destinations must not overlap the data, x_bar or mux_bar)
int check_point_noise_grad(svgp_ctx* ctx, const svgp_data* data, int64_t len, const svgp_input_grad* gx, const svgp_point_mean_grad* gpm,
                           const svgp_point_noise_grad* gpn) {
  if (!gpn) return SVGP_OK;
  if (!gpn->s_bar) return fail(ctx, SVGP_INVALID_ARG, "null per-point noise gradient output");
  if ((gpn->on_device != 0 && gpn->on_device != 1) || gpn->reserved != 0)
    return fail(ctx, SVGP_INVALID_ARG, "per-point noise gradient: on_device must be 0 or 1 and reserved 0");
  if (gpn->on_device && data && len >= 1) {
    const size_t es = data->dtype == SVGP_F64 ? 8 : 4;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(gpn->s_bar), a1 = a0 + size_t(len) * es;
    auto hits = [&](const void* p, size_t bytes) {
      const uintptr_t b0 = reinterpret_cast<uintptr_t>(p), b1 = b0 + bytes;
      return p && a0 < b1 && b0 < a1;
    };
    if (data->d >= 1 && hits(data->x.p, (size_t(data->d - 1) * size_t(data->ldx) + size_t(data->n)) * es))
      return fail(ctx, SVGP_INVALID_ARG, "per-point noise gradient output overlaps the data's x");
    if (hits(data->y.p, size_t(data->n) * es)) return fail(ctx, SVGP_INVALID_ARG, "per-point noise gradient output overlaps the data's y");
    if (gx && gx->on_device && data->d >= 1 && hits(gx->x, (size_t(data->d - 1) * size_t(gx->ld) + size_t(len)) * es))
      return fail(ctx, SVGP_INVALID_ARG, "per-point noise gradient output overlaps the input-gradient output");
    if (gpm && gpm->on_device && hits(gpm->mu_bar, size_t(len) * es))
      return fail(ctx, SVGP_INVALID_ARG, "per-point noise gradient output overlaps the prior-mean gradient output");
  }
  return SVGP_OK;
}

// the checks the three calls share, then mux and s onto the device: pointers as they are, host memory by one copy each into
// ctx->pm_x / ctx->pn_x
int collapsed_ext_begin(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, const svgp_point_mean* pm,
                        const svgp_point_noise* pn, CollapsedExt* ext) {
  int rc = collapsed_check(ctx, m, data, off, len, true);
  if (rc == SVGP_OK) rc = check_point_mean(ctx, pm);
  if (rc == SVGP_OK) rc = check_point_noise(ctx, pn);
  if (rc) return rc;
  ext->muz = m->mu_z.p != nullptr;
  return SVGP_OK;
}
int collapsed_ext_stage(svgp_ctx* ctx, const svgp_model* m, int64_t len, const svgp_point_mean* pm, const svgp_point_noise* pn,
                        CollapsedExt* ext) {
  if (!pm && !pn) return SVGP_OK;
  HIPC(ctx, hipSetDevice(ctx->device));
  const size_t bytes = size_t(len) * m->es;
  if (pm) {
    const int rc = stage_point_mean(ctx, pm, bytes, &ext->mux);
    if (rc) return rc;
  }
  if (pn) {
    if (pn->on_device) {
      ext->sv = pn->s;
    } else {
      const int rc = ctx->pn_x.reserve(ctx, bytes, "the per-point noise variances");
      if (rc) return rc;
      HIPC(ctx, hipMemcpyAsync(ctx->pn_x.p, pn->s, bytes, hipMemcpyHostToDevice, ctx->stream));
      ext->sv = ctx->pn_x.p;
    }
  }
  return SVGP_OK;
}

}  // namespace

extern "C" int32_t svgp_collapsed_bound_with_noise(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                                   const svgp_point_mean* pm, const svgp_point_noise* pn, double* bound_out,
                                                   svgp_collapsed_terms* terms_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  CollapsedExt ext;
  int rc = collapsed_ext_begin(ctx, m, data, off, len, pm, pn, &ext);
  if (rc == SVGP_OK) rc = collapsed_ext_stage(ctx, m, len, pm, pn, &ext);
  if (rc) return rc;
  return collapsed_run(ctx, m, data, off, len, false, bound_out, terms_out, &ext);
}

extern "C" int32_t svgp_collapsed_q_with_noise(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                               const svgp_point_mean* pm, const svgp_point_noise* pn, void* m_out, void* Lq_out,
                                               double* bound_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  CollapsedExt ext;
  int rc = collapsed_ext_begin(ctx, m, data, off, len, pm, pn, &ext);
  if (rc == SVGP_OK) rc = collapsed_ext_stage(ctx, m, len, pm, pn, &ext);
  if (rc) return rc;
  rc = collapsed_run(ctx, m, data, off, len, true, bound_out, nullptr, &ext);
  if (rc) return rc;
  return read_back_q(ctx, m, m_out, Lq_out);
}

extern "C" int32_t svgp_collapsed_grad_with_noise(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                                  const svgp_point_mean* pm, const svgp_point_noise* pn, double* bound_out,
                                                  svgp_collapsed_terms* terms_out, svgp_grads* g, const svgp_input_grad* gx,
                                                  svgp_point_mean_grad* gpm, svgp_point_noise_grad* gpn) {
  if (!ctx) return SVGP_INVALID_ARG;
  CollapsedExt ext;
  int rc = collapsed_ext_begin(ctx, m, data, off, len, pm, pn, &ext);
  if (rc) return rc;
  if (!g) return fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  if (g->m || g->Lq) return fail(ctx, SVGP_INVALID_ARG, "svgp_collapsed_grad_with_noise: grads_out->m and grads_out->Lq must be NULL (zero at the optimal q)");
  if (gx && (rc = check_input_grad(ctx, data, len, gx)) != SVGP_OK) return rc;
  if ((rc = check_point_mean_grad(ctx, data, len, gx, gpm)) != SVGP_OK) return rc;
  if ((rc = check_point_noise_grad(ctx, data, len, gx, gpm, gpn)) != SVGP_OK) return rc;
  if ((rc = collapsed_ext_stage(ctx, m, len, pm, pn, &ext)) != SVGP_OK) return rc;
  double bound = NAN;
  rc = collapsed_run(ctx, m, data, off, len, true, &bound, terms_out, &ext);
  if (rc) return rc;
  // d elbo / d q = 0 at the optimal q (svgp_collapsed_grad); the point stage evaluates point j with sigma_j^2 and hands back s_bar, mux_bar
  double elbo2 = NAN;
  GradRequest rq;   // scale 1, KL weight 1, local
  rq.num_data = double(len);
  rq.gx = gx;
  const svgp_point_mean pm_dev{ext.mux, 1, 0};   // staged above: on the device wherever the caller's lives
  if (ext.mux) rq.pm = &pm_dev;
  rq.gpm = gpm;
  rq.noise = ext.sv;
  if (gpn) {   // host destination: point_grad_kernel writes ctx->pn_g, one copy brings it over
    if (gpn->on_device) rq.noise_bar = gpn->s_bar;
    else if ((rc = ctx->pn_g.reserve(ctx, size_t(len) * m->es, "the per-point noise variances' gradient")) == SVGP_OK) rq.noise_bar = ctx->pn_g.p;
    if (rc) return rc;
  }
  rc = elbo_grad_impl(ctx, m, data, off, len, rq, &elbo2, nullptr, g);
  if (rc) return rc;
  if (gpn && !gpn->on_device) {
    HIPC(ctx, hipMemcpyAsync(gpn->s_bar, ctx->pn_g.p, size_t(len) * m->es, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (bound_out) *bound_out = bound;
  return SVGP_OK;
}

// ================================================================================================
// One natural-gradient step on q(u): svgp_natgrad_step / _ext (natgrad.hip has the formulas and the kernels).  The launches of
// svgp_elbo_grad, unchanged, then the M-sized fp64 tail on the same stream: the value-and-gradient's read-back (grad_finish) follows the
// tail's enqueue, so the two overlap and the call synchronises once more only for the tail's 64 status bytes.
namespace svgp {

int natgrad_enqueue(svgp_ctx* ctx, svgp_model* m, GradCall& gc, NatgradCall& ng) {
  hipStream_t s = ctx->stream;
  GradWs* w = gc.w;
  CollapsedWs* c = ng.c;
  const int dt = m->dtype;
  const int64_t Mp = m->Mp, M = m->M;
  const double gamma = ng.gamma;
  const bool full = gamma == 1.0;   // Lambda' = I + W: Lambda is neither formed nor read
  double* Wm = c->Wm.as<double>();
  double* Bw = full ? nullptr : c->Bw.as<double>();
  double* mw = c->mw.as<double>();
  double* scal = c->scal.as<double>();
  int* info_b = c->info_b.as<int>();
  int* info_s = c->info_s.as<int>();
  int* info_q = c->info_q.as<int>();
  // the prep of this very call left the whitened q on the model: m->mp = m_w, m->U = B' (both parametrisations)
  launch_natgrad_widen(dt, s, m->U.p, m->mp.p, M, Mp, Bw, mw);
  const double* Lam = nullptr;
  if (!full) {
    // Lambda = B^-T B^-1 from the explicit inverse of the triangular B (never inv(B B'): that squares cond(B))
    launch_natgrad_diag_check(s, Bw, M, Mp, info_q);
    launch_natgrad_diag_inv(s, Bw, Mp, c->TB.as<double>());
    (void)inverse_product_factor(ctx, c, Bw, nullptr);   // (no factor: nothing in it can fail)
    Lam = c->Sinv.as<double>();
    KCHECK(ctx, "natgrad tail (Lambda)");
  }
  launch_natgrad_form(s, Lam, Wm, Mp, gamma, c->Bm.as<double>());
  launch_natgrad_rhs(s, c->Bm.as<double>(), mw, w->avec.as<double>(), Mp, gamma, c->cvec.as<double>());
  HIPC(ctx, hipMemsetAsync(info_b, 0, info_bytes(Mp), s));
  launch_potrf(SVGP_F64, s, c->Bm.p, c->TB.p, Mp, info_b, reinterpret_cast<unsigned*>(info_b + 1), ctx->num_cus);
  launch_trsv2(SVGP_F64, s, c->Bm.p, c->TB.p, Mp, 0, c->cvec.p);
  HIPC(ctx, hipMemcpyAsync(c->mw.p, c->cvec.p, size_t(Mp) * 8, hipMemcpyDeviceToDevice, s));
  launch_trsv2(SVGP_F64, s, c->Bm.p, c->TB.p, Mp, 1, c->mw.p);   // m_w' = Lambda'^-1 rhs
  KCHECK(ctx, "natgrad tail (cholesky(Lambda'), m_w)");
  // S_w' = inv(Lambda') = L^-T L^-1 from the explicit triangular inverse; Lq_w = its lower Cholesky factor (the collapsed bound's tail)
  const int rci = inverse_product_factor(ctx, c, c->Bm.p, info_s);
  if (rci) return rci;
  launch_natgrad_status(s, Wm, w->avec.as<double>(), Mp, info_b, info_s, full ? nullptr : info_q, m->info.as<int>(), w->sums,
                        m->desc.neg_var_policy == SVGP_NEGVAR_ERROR ? 1 : 0, scal);
  KCHECK(ctx, "natgrad tail (inv(Lambda'), its factor)");
  // device to device into the model's own m / Lq; nothing is written when a factorisation failed or the value-and-gradient itself fails
  launch_collapsed_write_q(dt, s, c->Sinv.as<double>(), mw, m->L.p, M, Mp, m->desc.parametrization == SVGP_CENTERED ? 1 : 0,
                           m->desc.mean_const, scal, info_b, info_s, nullptr, m->m_raw.p, m->Lq_raw.p);
  KCHECK(ctx, "natgrad q");
  return SVGP_OK;
}

// after grad_finish returned SVGP_OK: the tail's status; the model is prepared again, lazily, once q was written
int natgrad_finish(svgp_ctx* ctx, svgp_model* m, NatgradCall& ng) {
  double h[8] = {};
  HIPC(ctx, hipMemcpyAsync(h, ng.c->scal.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  const bool nan_in = std::isnan(h[0]) || std::isnan(h[1]);   // a NaN coordinate / observation: q is written NaN, SVGP_OK (the rule of svgp_collapsed_q)
  if (!nan_in) {
    const int ib = int(h[4]), is = int(h[5]), iq = int(h[6]);
    char buf[240];
    if (iq != 0) {
      snprintf(buf, sizeof buf, "the whitened Cholesky factor of q has a non-positive diagonal entry: leading minor of order %d (PosDefException); q is unchanged", iq);
      return fail(ctx, SVGP_NOT_POSDEF, buf);
    }
    if (ib != 0 || is != 0) {
      snprintf(buf, sizeof buf, "%s is not positive definite: leading minor of order %d (PosDefException); q is unchanged",
               ib ? "the precision of the natural-gradient step, (1 - gamma) inv(S_w) + gamma (I + W)," : "the covariance of the natural-gradient step", ib ? ib : is);
      return fail(ctx, SVGP_NOT_POSDEF, buf);
    }
    if (h[7] != 0.0) return SVGP_OK;   // (unreachable behind an SVGP_OK of grad_finish: q was not written)
  }
  m->prepared = false;
  return SVGP_OK;
}

}  // namespace svgp

namespace {

int natgrad_step_impl(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double num_data, double gamma, bool ext,
                      double sum_e, const double* g_mu, const double* g_v, double* elbo_out, svgp_terms* terms_out, svgp_grads* g,
                      void* m_out, void* Lq_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!(gamma > 0.0 && gamma <= 1.0)) return fail(ctx, SVGP_INVALID_ARG, "svgp_natgrad_step: the step length gamma must lie in (0, 1]");
  if (ext && (!g_mu || !g_v)) return fail(ctx, SVGP_INVALID_ARG, "null point gradients");
  int rc = check_batch(ctx, m, data, off, len, !ext);
  if (rc) return rc;
  if (ctx->comm) return fail(ctx, SVGP_UNSUPPORTED, "the natural-gradient step is not collective: detach the communicator");
  if (m->mu_z.p) return fail(ctx, SVGP_UNSUPPORTED, "the natural-gradient step takes no prior mean offsets (svgp_model_set_mean_z)");
  HIPC(ctx, hipSetDevice(ctx->device));
  NatgradCall ng;
  ng.gamma = gamma;
  rc = collapsed_workspace(ctx, m->Mp, &ng.c);
  if (rc) return rc;
  const size_t mm = size_t(m->Mp) * size_t(m->Mp) * 8;
  if ((rc = ng.c->Wm.reserve(ctx, mm, "the natural-gradient step's workspace")) != SVGP_OK) return rc;
  if (gamma != 1.0 && (rc = ng.c->Bw.reserve(ctx, mm, "the natural-gradient step's workspace")) != SVGP_OK) return rc;
  if ((rc = ng.c->info_q.reserve(ctx, 256, "the natural-gradient step's workspace")) != SVGP_OK) return rc;
  svgp_grads none{};   // the gradient is computed whether or not it is wanted: grads_out NULL reads none of its blocks back
  const double scale = (num_data > 0 ? num_data : double(len)) / double(len);
  GradRequest rq;   // local: no collective
  rq.scale = scale;
  rq.num_data = num_data;
  if (ext) { rq.ext_gmu = g_mu; rq.ext_gv = g_v; rq.ext_sum_e = sum_e; }
  rq.ng = &ng;
  rc = elbo_grad_impl(ctx, m, data, off, len, rq, elbo_out, terms_out, g ? g : &none);
  if (rc) return rc;
  return read_back_q(ctx, m, m_out, Lq_out);
}

}  // namespace

extern "C" int32_t svgp_natgrad_step(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double num_data,
                                     double gamma, double* elbo_out, svgp_terms* terms_out, svgp_grads* g, void* m_out, void* Lq_out) {
  return natgrad_step_impl(ctx, m, data, off, len, num_data, gamma, false, 0.0, nullptr, nullptr, elbo_out, terms_out, g, m_out, Lq_out);
}

extern "C" int32_t svgp_natgrad_step_ext(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double num_data,
                                         double gamma, double sum_e, const double* g_mu, const double* g_v, double* elbo_out,
                                         svgp_terms* terms_out, svgp_grads* g, void* m_out, void* Lq_out) {
  return natgrad_step_impl(ctx, m, data, off, len, num_data, gamma, true, sum_e, g_mu, g_v, elbo_out, terms_out, g, m_out, Lq_out);
}
