// cg_sampler_api.hip — svgp_cg_sampler_create / _eval / _eval_grad / _state / _plan / _free: pathwise function samples of the exact GP
// (cg_sample.hip: the kernels) - one batched solve of the S right-hand sides delta - Phi(X) w_s - sigma eps_s, then every evaluation
// is one data-sized pass.  Host orchestration only; cg_host.hpp holds the sampler.
#include <memory>
#include <new>

#include "cg_host.hpp"

using namespace svgp;

namespace {

// the launches of one evaluation over the points [off, off + len) of x (feature-major, ld ldx): out / grad are device pointers (grad
// NULL: the value form).  feat_only: the Fourier part alone, Phi(x) w (the right-hand sides of create)
int cgs_launch(svgp_ctx* ctx, const svgp_cg_sampler* sp, const void* x, int64_t ldx, int64_t off, int64_t len, void* out, int64_t ldo, void* grad,
               int64_t ldg, bool feat_only) {
  CgSampleArgs a{};
  a.frows = sp->frows.p;
  a.fbias = sp->fbias.p;
  a.W = sp->W.p;
  a.rows = sp->rows.p;
  a.bias = sp->bias.p;
  a.V = sp->V.p;
  a.invl = sp->invl.p;
  a.x = x;
  a.out = out;
  a.grad = grad;
  a.ldx = ldx;
  a.off = off;
  a.len = len;
  a.ldo = ldo;
  a.ldg = ldg;
  a.Lp = sp->Lp;
  a.S = sp->S;
  a.family = sp->family;
  a.d = sp->d;
  a.variance = sp->variance;
  if (feat_only) {
    cg_sample_plan(0, &a.seg_rows, &a.nseg, &a.round);
  } else {
    a.N = sp->N;
    a.Np = sp->Np;
    a.seg_rows = sp->seg_rows;
    a.nseg = sp->nseg;
    a.round = sp->round;
    a.mean_const = sp->mean_const;
  }
  const int64_t rnd = cg_sample_round(a.round, grad != nullptr), pts = len < rnd ? len : rnd;
  // the scratch is the context's: the sampler itself is read-only in every evaluation
  const int rc = ctx->cgs_part.reserve(ctx, size_t(a.nseg) * size_t(grad ? 144 : 64) * size_t(pts) * sp->es, "the samples' partial sums");
  if (rc) return rc;
  a.part = ctx->cgs_part.p;
  launch_cg_sample(sp->dtype, ctx->stream, a);
  return SVGP_OK;
}

int cgs_eval_checks(svgp_ctx* ctx, const svgp_cg_sampler* sp, const svgp_data* data, int64_t off, int64_t len, int32_t out_on_device) {
  if (sp->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the sampler lives on another device than the context");
  if (data->dtype != sp->dtype) return fail(ctx, SVGP_INVALID_ARG, "data and sampler dtypes differ");
  if (data->d != sp->d) return fail(ctx, SVGP_INVALID_ARG, "data and sampler input dimensions differ");
  if (off < 0 || len < 1 || off + len > data->n) return fail(ctx, SVGP_INVALID_ARG, "window outside the data");
  if (out_on_device != 0 && out_on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "out_on_device must be 0 or 1");
  return SVGP_OK;
}

}  // namespace

extern "C" {

int32_t svgp_cg_sampler_create(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, const svgp_sample_basis* basis,
                               svgp_cg_sampler** out, svgp_cg_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!out) return fail(ctx, SVGP_INVALID_ARG, "null out pointer");
  *out = nullptr;
  if (!cg || !basis) return fail(ctx, SVGP_INVALID_ARG, "null CG handle or sample basis");
  int rc = common_checks(ctx, cg, desc);
  if (rc) return rc;
  const int64_t L = basis->n_features, S = basis->n_samples;
  if (S < 1) return fail(ctx, SVGP_INVALID_ARG, "n_samples must be >= 1");
  if (L < 0) return fail(ctx, SVGP_INVALID_ARG, "n_features must be >= 0");
  if (!basis->eps) return fail(ctx, SVGP_INVALID_ARG, "null eps");
  if (L > 0 && (!basis->omega || !basis->tau || !basis->w)) return fail(ctx, SVGP_INVALID_ARG, "null omega, tau or w with n_features > 0");
  if (!delta && !cg->data->y.p) return fail(ctx, SVGP_INVALID_ARG, "the data handle has no y and no delta was given");
  if (cg->pc.k > 0 && (rc = check_precond_desc(ctx, cg, desc)) != SVGP_OK) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype, d = cg->d;
  const int64_t N = cg->N;
  const size_t es = cg->es, col = size_t(N) * es;
  const CgPar par = par_of(desc);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::unique_ptr<svgp_cg_sampler> sp(new (std::nothrow) svgp_cg_sampler());
  if (!sp) return SVGP_OOM;
  sp->dtype = dt;
  sp->d = d;
  sp->family = par.family;
  sp->device = ctx->device;
  sp->es = es;
  sp->N = N;
  sp->Np = cg->Np;
  sp->L = L;
  sp->Lp = (L + 31) / 32 * 32;
  sp->S = S;
  sp->variance = par.variance;
  sp->mean_const = par.mean_const;
  cg_sample_plan(N, &sp->seg_rows, &sp->nseg, &sp->round);
  const int64_t Lp = sp->Lp;
  DevBuf d_omega, d_tau, d_w, d_eps, dvec, phi, B;
  const char* what = "the sampler";   // (L = 0: the rows of 0 bytes ask for nothing)
  rc = reserve_all(ctx, {{&sp->invl, size_t(SVGP_MAX_D) * 8, what}, {&sp->rows, size_t(d) * size_t(cg->Np) * es, what},
                         {&sp->bias, size_t(cg->Np) * es, what}, {&sp->frows, size_t(d) * size_t(Lp) * es, what}, {&sp->fbias, size_t(Lp) * es, what},
                         {&sp->W, size_t(Lp) * size_t(S) * es, what}, {&sp->V, col * size_t(S), what}, {&d_omega, size_t(L) * size_t(d) * es, what},
                         {&d_tau, size_t(L) * es, what}, {&d_w, size_t(S) * size_t(L) * es, what}, {&d_eps, col * size_t(S), what}, {&dvec, col, what},
                         {&phi, L > 0 ? col * size_t(S) : 0, what}, {&B, col * size_t(S), what}, {&cg->f64tmp, size_t(N) * 8, what},
                         {&cg->res, size_t(S) * 8, what}});
  if (rc) return rc;
  if ((rc = ensure_solver(ctx, cg, S, false, par.maxiter)) != SVGP_OK) return rc;
  if ((rc = noise_check(ctx, cg, desc, cg->pc.k > 0)) == SVGP_OK) rc = set_params(ctx, cg, par);
  if (rc != SVGP_OK) {   // SVGP_NOT_POSDEF: the preconditioner did not factor, or a bad noise variance - no sampler
    if (rc == SVGP_NOT_POSDEF && info) *info = nan_info();
    return rc;
  }
  // the snapshot: the parameter set and the prepared rows of this call, the basis in the kernel's layout
  HIPC(ctx, hipMemcpyAsync(sp->invl.p, cg->invl.p, size_t(d) * es, hipMemcpyDeviceToDevice, s));
  HIPC(ctx, hipMemcpyAsync(sp->rows.p, cg->rows.p, size_t(d) * size_t(cg->Np) * es, hipMemcpyDeviceToDevice, s));
  HIPC(ctx, hipMemcpyAsync(sp->bias.p, cg->bias.p, size_t(cg->Np) * es, hipMemcpyDeviceToDevice, s));
  if (L > 0) {
    HIPC(ctx, hipMemcpyAsync(d_omega.p, basis->omega, size_t(L) * size_t(d) * es, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(d_tau.p, basis->tau, size_t(L) * es, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(d_w.p, basis->w, size_t(S) * size_t(L) * es, hipMemcpyHostToDevice, s));
  }
  HIPC(ctx, hipMemcpyAsync(d_eps.p, basis->eps, col * size_t(S), hipMemcpyHostToDevice, s));
  const double amp = L > 0 ? std::sqrt(2.0 * par.variance / double(L)) : 0.0;
  launch_cg_sample_basis(dt, s, d_omega.p, d_tau.p, d_w.p, d, L, Lp, S, amp, sp->frows.p, sp->fbias.p, sp->W.p);
  if ((rc = stage_delta(ctx, cg, par, delta, dvec.p)) != SVGP_OK) return rc;   // rounded once, as svgp_cg_fit rounds it
  // Phi(X) w through the evaluation kernel over the features alone, then one affine pass: B_s = delta - Phi(X) w_s - sigma eps_s
  if (L > 0 && (rc = cgs_launch(ctx, sp.get(), cg->data->x.p, cg->data->ldx, 0, N, phi.p, N, nullptr, 0, true)) != SVGP_OK) return rc;
  const double sigma = std::sqrt(dt == SVGP_F64 ? par.diag : double(float(par.diag)));
  launch_cg_sample_rhs(dt, s, dvec.p, L > 0 ? phi.p : nullptr, d_eps.p, sigma, N, S, B.p, cg->have_noise ? cg->sig2.p : nullptr);
  launch_cg_dot(dt, s, B.p, N, B.p, N, N, S, cg->partial.as<double>());
  launch_cg_colsum(s, cg->partial.as<double>(), N, S, cg->res.as<double>());
  KCHECK(ctx, "cg sampler (right-hand sides)");
  std::vector<double> bb(size_t(S), 0.0);
  HIPC(ctx, hipMemcpyAsync(bb.data(), cg->res.p, size_t(S) * 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));   // (the caller's host arrays may be released from here on)
  bool finite = true;
  for (double v : bb) finite = finite && std::isfinite(v);
  sp->iters.assign(size_t(S), 0);
  sp->relres.assign(size_t(S), nan);
  svgp_cg_info oi{};
  if (finite) {
    rc = solve_core(ctx, cg, par, S, B.p, N, sp->V.p, N, sp->iters.data(), sp->relres.data(), &oi, nullptr);
    if (rc) {
      if (info) *info = oi;
      return rc;
    }
  } else {   // non-finite inputs: non-finite samples, SVGP_OK
    launch_cg_affine(dt, s, sp->V.p, 0, N, N, S, 0.0, nan, sp->V.p, N);
    KCHECK(ctx, "cg sampler (NaN outputs)");
    HIPC(ctx, hipStreamSynchronize(s));
    oi = nan_info();
    oi.n_unconverged = int32_t(S < 2147483647 ? S : 2147483647);
  }
  if (info) *info = oi;
  *out = sp.release();
  return SVGP_OK;
}

int32_t svgp_cg_sampler_eval(svgp_ctx* ctx, const svgp_cg_sampler* sp, const svgp_data* data, int64_t off, int64_t len, void* out, int64_t ldo,
                             int32_t out_on_device) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!sp || !data) return fail(ctx, SVGP_INVALID_ARG, "null sampler or data");
  if (!out) return fail(ctx, SVGP_INVALID_ARG, "null output");
  int rc = cgs_eval_checks(ctx, sp, data, off, len, out_on_device);
  if (rc) return rc;
  if (ldo < len) return fail(ctx, SVGP_INVALID_ARG, "ldo must be >= len");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t es = sp->es;
  if (!out_on_device && (rc = ctx->smp_out.reserve(ctx, size_t(sp->S) * size_t(len) * es, "the samples")) != SVGP_OK) return rc;
  TREC(ctx, ctx->ev[0], s);
  if ((rc = cgs_launch(ctx, sp, data->x.p, data->ldx, off, len, out_on_device ? out : ctx->smp_out.p, out_on_device ? ldo : len, nullptr, 0, false)) !=
      SVGP_OK)
    return rc;
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "cg_sample");
  if (!out_on_device)
    HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * es, ctx->smp_out.p, size_t(len) * es, size_t(len) * es, size_t(sp->S), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  cg_timing(ctx);
  return SVGP_OK;
}

int32_t svgp_cg_sampler_eval_grad(svgp_ctx* ctx, const svgp_cg_sampler* sp, const svgp_data* data, int64_t off, int64_t len, void* out, int64_t ldo,
                                  void* grad_out, int64_t ldg, int32_t out_on_device) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!sp || !data) return fail(ctx, SVGP_INVALID_ARG, "null sampler or data");
  if (!grad_out) return fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  int rc = cgs_eval_checks(ctx, sp, data, off, len, out_on_device);
  if (rc) return rc;
  if (out && ldo < len) return fail(ctx, SVGP_INVALID_ARG, "ldo must be >= len");
  if (ldg < len) return fail(ctx, SVGP_INVALID_ARG, "ldg must be >= len");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t es = sp->es;
  const size_t grows = size_t(sp->S) * size_t(sp->d);   // rows of the gradient: (s, c)
  if (!out_on_device) {
    if (out && (rc = ctx->smp_out.reserve(ctx, size_t(sp->S) * size_t(len) * es, "the samples")) != SVGP_OK) return rc;
    if ((rc = ctx->smp_grad.reserve(ctx, grows * size_t(len) * es, "the samples' gradients")) != SVGP_OK) return rc;
  }
  TREC(ctx, ctx->ev[0], s);
  if ((rc = cgs_launch(ctx, sp, data->x.p, data->ldx, off, len, !out ? nullptr : out_on_device ? out : ctx->smp_out.p, out_on_device ? ldo : len,
                       out_on_device ? grad_out : ctx->smp_grad.p, out_on_device ? ldg : len, false)) != SVGP_OK)
    return rc;
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "cg_sample (gradient)");
  if (!out_on_device) {
    if (out)
      HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * es, ctx->smp_out.p, size_t(len) * es, size_t(len) * es, size_t(sp->S), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipMemcpy2DAsync(grad_out, size_t(ldg) * es, ctx->smp_grad.p, size_t(len) * es, size_t(len) * es, grows, hipMemcpyDeviceToHost, s));
  }
  HIPC(ctx, hipStreamSynchronize(s));
  cg_timing(ctx);
  return SVGP_OK;
}

int32_t svgp_cg_sampler_state(svgp_ctx* ctx, const svgp_cg_sampler* sp, void* V_out, int32_t* iters_out, double* relres_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!sp) return fail(ctx, SVGP_INVALID_ARG, "null sampler");
  if (sp->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the sampler lives on another device than the context");
  HIPC(ctx, hipSetDevice(ctx->device));
  if (V_out) {
    HIPC(ctx, hipMemcpyAsync(V_out, sp->V.p, size_t(sp->N) * size_t(sp->S) * sp->es, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
  }
  for (int64_t j = 0; j < sp->S; ++j) {
    if (iters_out) iters_out[j] = sp->iters[size_t(j)];
    if (relres_out) relres_out[j] = sp->relres[size_t(j)];
  }
  return SVGP_OK;
}

int32_t svgp_cg_sampler_plan(int64_t N, int64_t* seg_rows, int32_t* n_segments, int64_t* round_points) {
  if (N < 0 || !seg_rows || !n_segments || !round_points) return SVGP_INVALID_ARG;
  int ns = 1;
  cg_sample_plan(N, seg_rows, &ns, round_points);
  *n_segments = ns;
  return SVGP_OK;
}

int32_t svgp_cg_sampler_free(svgp_ctx* ctx, svgp_cg_sampler* sp) {
  if (!sp) return SVGP_OK;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  delete sp;
  return SVGP_OK;
}

}  // extern "C"
