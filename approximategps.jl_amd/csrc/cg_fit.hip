// cg_fit.hip — the exact GP by conjugate gradients, the fit and its gradients: svgp_cg_fit / _lml_grad / _fit_precond / _lml_grad_precond /
// _lml_grad_inputs / _lml_grad_noise / _alpha / _predict (cg.hip: the kernels; cg_xgrad.hip: the input gradient's).  Host orchestration
// only: one FitRequest per entry point, run through the stages of fit_impl.
#include "cg_host.hpp"

using namespace svgp;

namespace {

constexpr int64_t kCgMaxPredict = int64_t(1) << 28;   // n N elements of the predictive variance's right-hand sides in one call

struct DataHold {   // test inputs uploaded for one call
  svgp_ctx* ctx;
  svgp_data* D = nullptr;
  ~DataHold() { if (D) svgp_data_free(ctx, D); }
};

// what one fit is asked for, beyond the handle and its descriptor
struct FitRequest {
  const double* delta = nullptr;   // host, N; NULL: y - mean_const
  int32_t T = 0;                   // probes
  const double* probes = nullptr;     // host, N x T
  const double* probes_k = nullptr;   // host, k x T: the preconditioner's part
  bool precond_call = false;       // the entry point takes probes_k
  // grad: the gradient {d_variance, d_inv_lengthscale[d], d_diag, d_mean_const} is asked for (the first two must be non-null)
  bool grad = false;
  double *d_variance = nullptr, *d_inv_lengthscale = nullptr, *d_diag = nullptr, *d_mean_const = nullptr;
  const svgp_input_grad* gx = nullptr;           // where d lml / d x goes (NULL: not requested)
  const svgp_point_noise_grad* gpn = nullptr;    // where d lml / d sigma_i^2 goes (NULL: not requested)
  double* lml_out = nullptr;
  svgp_cg_info* info = nullptr;
};

struct FitRun {   // what the stages of one fit share
  svgp_ctx* ctx;
  svgp_cg* cg;
  const FitRequest& rq;
  CgPar par;
  bool pc, want_sbar;   // a preconditioner is set; s_bar is needed (with a vector set d_variance needs sum_i sigma_i^2 s_bar_i)
  int64_t N, S;         // S = T + 1 columns: [delta, z_1 .. z_T]
  size_t col;
  CgHist hist;
  svgp_cg_info out{};
};

// 1. the argument checks, in the order that decides a doubly-wrong call's message
int fit_check(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds, const FitRequest& rq) {
  int rc = common_checks(ctx, cg, ds);
  if (rc) return rc;
  const bool pc = cg->pc.k > 0;
  const int32_t T = rq.T;
  if (rq.precond_call && !pc) return fail(ctx, SVGP_INVALID_ARG, "no preconditioner is set on this handle (svgp_cg_set_preconditioner)");
  if (pc && (rc = check_precond_desc(ctx, cg, ds)) != SVGP_OK) return rc;
  if (pc && T > 0 && !rq.precond_call)
    return fail(ctx, SVGP_INVALID_ARG, "a preconditioner is set: the probes need their k x T part (svgp_cg_fit_precond / svgp_cg_lml_grad_precond)");
  if (pc && T > 0 && !rq.probes_k) return fail(ctx, SVGP_INVALID_ARG, "null probes_k with T > 0");
  if (!rq.delta && !cg->data->y.p) return fail(ctx, SVGP_INVALID_ARG, "the data handle has no y and no delta was given");
  if (T < 0) return fail(ctx, SVGP_INVALID_ARG, "the number of probes must be >= 0");
  if (T > 0 && !rq.probes) return fail(ctx, SVGP_INVALID_ARG, "null probes with T > 0");
  if (rq.grad && (!rq.d_variance || !rq.d_inv_lengthscale)) return fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  if (rq.gx && (rc = check_input_grad(ctx, cg->data, cg->N, rq.gx)) != SVGP_OK) return rc;
  if (rq.gpn && !rq.gpn->s_bar) return fail(ctx, SVGP_INVALID_ARG, "null noise-gradient output");
  if (rq.gpn && rq.gpn->on_device != 0 && rq.gpn->on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  if (rq.gpn && rq.gpn->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved must be 0");
  return SVGP_OK;
}

// 2. the handle's buffers of this fit
int fit_reserve(FitRun& f) {
  svgp_cg* cg = f.cg;
  const FitRequest& rq = f.rq;
  const size_t T = size_t(rq.T), S = size_t(f.S), S2 = 2 * T + 1, d = size_t(cg->d), N = size_t(f.N), col = f.col;
  const bool xg = rq.gx && rq.T > 0;
  const int rc = ensure_solver(f.ctx, cg, f.S, true, f.par.maxiter);
  if (rc) return rc;
  return reserve_all(f.ctx, {{&cg->fitB, col * S, "the CG right-hand sides"},
                             {&cg->fitX, col * S, "the CG solutions"},
                             {&cg->f64tmp, N * (T > 0 ? T : 1) * 8, "the probes"},
                             {&cg->res, ((d + 2) * S + 8) * 8, "the CG results"},
                             {&cg->gout, rq.grad ? col * S : 0, "the gradient's products"},
                             {&cg->sbar, f.want_sbar ? col : 0, "the noise gradient"},
                             {&cg->xL, xg ? col * S2 : 0, "the input gradient's panels"},
                             {&cg->xR, xg ? col * S2 : 0, "the input gradient's panels"},
                             {&cg->xpart, xg ? ((S2 + 15) / 16) * d * N * 8 : 0, "the input gradient's partial sums"},
                             {&cg->xout, xg && !rq.gx->on_device ? col * d : 0, "the input gradient"}});
}

// a failed set_params or solve: its info and value out; SVGP_NOT_POSDEF: NaN in the input and noise gradients as well, the status and
// its message kept
int fit_failed(FitRun& f, int status, const svgp_cg_info& bad) {
  const FitRequest& rq = f.rq;
  if (rq.info) *rq.info = bad;
  if (rq.lml_out) *rq.lml_out = bad.lml;
  if ((rq.gx || rq.gpn) && status == SVGP_NOT_POSDEF) {
    const ErrKeep keep(f.ctx);
    if (rq.gx) (void)nan_fill(f.ctx, f.cg->dtype, rq.gx->x, rq.gx->ld, f.N, f.cg->d, rq.gx->on_device);
    if (rq.gpn) (void)nan_fill(f.ctx, f.cg->dtype, rq.gpn->s_bar, f.N, f.N, 1, rq.gpn->on_device);
  }
  return status;
}

// 3. the right-hand sides [delta, z_1 .. z_T] into fitB, each entry rounded once to the data dtype.  With a preconditioner the probes
// are z_t = sigma eps_t + Z Lu^-T xi_t (E z z' = P): eps rounded into fitX (the solve overwrites it), Lu^-T xi into pc.v
int fit_rhs(FitRun& f) {
  svgp_ctx* ctx = f.ctx;
  svgp_cg* cg = f.cg;
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype;
  const int32_t T = f.rq.T;
  const int64_t N = f.N;
  int rc = stage_delta(ctx, cg, f.par, f.rq.delta, cg->fitB.p);
  if (rc) return rc;
  if (T > 0 && !f.pc) {
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, f.rq.probes, size_t(N) * size_t(T) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, T, 1.0, 0.0, cg->fitB.as<char>() + f.col, N);
  }
  if (T > 0 && f.pc) {
    CgPrecond& P = cg->pc;
    rc = reserve_all(ctx, {{&P.xi, size_t(P.k) * size_t(T) * 8, "the probes"},
                           {&P.v, size_t(P.kp) * size_t(T) * cg->es, "the preconditioner's products"}});
    if (rc) return rc;
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, f.rq.probes, size_t(N) * size_t(T) * 8, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(P.xi.p, f.rq.probes_k, size_t(P.k) * size_t(T) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, T, 1.0, 0.0, cg->fitX.as<char>() + f.col, N);
    launch_cg_pc_mm(dt, s, P.LinvRM.as<double>(), P.Mp, P.k, P.xi.p, 1, P.k, T, 1.0, P.v.p, P.kp, P.kp);
    pc_expand(ctx, cg, f.par, P.v.p, T, cg->fitX.as<char>() + f.col, N, std::sqrt(P.s2), cg->fitB.as<char>() + f.col, N,
              cg->have_noise ? cg->ssig2.p : nullptr);   // per-point noise: z_t = D^1/2 eps_t + Z Lu^-T xi_t
  }
  KCHECK(ctx, "cg (right-hand sides)");
  return SVGP_OK;
}

// 5. the value: quad = delta' alpha, log det Khat = (log det P +) (1 / T) sum_t (z_t' P^-1 z_t) e_1' log(T_t) e_1, lml
int fit_value(FitRun& f) {
  svgp_ctx* ctx = f.ctx;
  svgp_cg* cg = f.cg;
  hipStream_t s = ctx->stream;
  const int32_t T = f.rq.T;
  const int64_t N = f.N;
  double* partial = cg->partial.as<double>();
  double* res = cg->res.as<double>();
  launch_cg_dot(cg->dtype, s, cg->fitB.p, N, cg->fitX.p, N, N, 1, partial);
  launch_cg_colsum(s, partial, N, 1, res);
  KCHECK(ctx, "cg (quad)");
  double quad = 0;
  HIPC(ctx, hipMemcpyAsync(&quad, res, 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double logdet = nan;
  if (T > 0) {
    logdet = 0.0;
    for (int t = 1; t <= T; ++t) {   // t ascending: a fixed order
      const auto& a = f.hist.a[size_t(t)];
      if (a.empty()) continue;   // a zero probe
      double qv = 0;
      if (lanczos_quadrature(a.data(), f.hist.b[size_t(t)].data(), int(a.size()), &qv) != SVGP_OK) qv = nan;
      logdet += f.hist.bb[size_t(t)] * qv;
    }
    logdet /= double(T);
    if (f.pc) logdet += cg->pc.logdet_p;
  }
  f.out.quad = quad;
  f.out.logdet = logdet;
  f.out.lml = -0.5 * (quad + logdet + double(N) * 1.8378770664093454836);
  cg->fit = f.par;
  cg->have_fit = true;
  return SVGP_OK;
}

// 6. the hyperparameter gradient from the panels U = fitX = [alpha, w_t] and P = fitB = [alpha, p_t] (p_t = z_t, or P^-1 z_t with a
// preconditioner: the trace terms are w_t' dKhat p_t); s_bar, where it is needed, into cg->sbar
int fit_hyper_grad(FitRun& f) {
  svgp_ctx* ctx = f.ctx;
  svgp_cg* cg = f.cg;
  const FitRequest& rq = f.rq;
  const CgPar& par = f.par;
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype, d = cg->d;
  const int32_t T = rq.T;
  const int64_t N = f.N, S = f.S;
  const size_t col = f.col;
  double* partial = cg->partial.as<double>();
  double* res = cg->res.as<double>();
  int rc;
  // the panel [alpha, z_1 .. z_T]: delta has served
  HIPC(ctx, hipMemcpyAsync(cg->fitB.p, cg->fitX.p, col, hipMemcpyDeviceToDevice, s));
  const void *U = cg->fitX.p, *P = cg->fitB.p;
  void* O = cg->gout.p;
  if (f.pc && T > 0) {   // the panel's probe columns become P^-1 z_t
    if ((rc = pc_apply(ctx, cg, par, cg->fitB.as<char>() + col, N, T, static_cast<char*>(O) + col, N)) != SVGP_OK) return rc;
    HIPC(ctx, hipMemcpyAsync(cg->fitB.as<char>() + col, static_cast<char*>(O) + col, col * size_t(T), hipMemcpyDeviceToDevice, s));
  }
  launch_cg_dot(dt, s, U, N, P, N, N, S, partial);
  launch_cg_colsum(s, partial, N, S, res);
  kmv(ctx, cg, par, cg->data->x.p, cg->data->ldx, N, P, N, S, P, N, O, N);
  launch_cg_dot(dt, s, U, N, O, N, N, S, partial);
  launch_cg_colsum(s, partial, N, S, res + S);
  for (int c = 0; c < d; ++c) {
    kmv(ctx, cg, par, cg->data->x.p, cg->data->ldx, N, P, N, S, nullptr, N, O, N, 1, c);
    launch_cg_dot(dt, s, U, N, O, N, N, S, partial);
    launch_cg_colsum(s, partial, N, S, res + int64_t(2 + c) * S);
  }
  launch_cg_affine(dt, s, O, 0, N, N, 1, 0.0, 1.0, O, N);   // ones
  launch_cg_dot(dt, s, U, N, O, N, N, 1, partial);
  launch_cg_colsum(s, partial, N, 1, res + int64_t(2 + d) * S);
  if (f.want_sbar) {   // s_bar from the panels, and sum_i sigma_i^2 s_bar_i behind the other results
    launch_cg_sbar(dt, s, U, P, N, T, cg->sbar.p);
    if (cg->have_noise) {
      launch_cg_noise_sum(dt, s, cg->sig2.p, cg->sbar.p, N, partial);
      launch_cg_colsum(s, partial, N, 1, res + int64_t(2 + d) * S + 1);
    }
  }
  KCHECK(ctx, "cg (gradient)");
  std::vector<double> h(size_t(d + 2) * size_t(S) + (cg->have_noise ? 2 : 1));
  HIPC(ctx, hipMemcpyAsync(h.data(), res, h.size() * 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  auto combine = [&](const double* v, const double* sub, double subw) {   //  1/2 v_0 - 1/(2T) sum_t v_t, t ascending
    double tr = 0.0;
    for (int t = 1; t <= T; ++t) tr += v[t] - (sub ? subw * sub[t] : 0.0);
    const double first = v[0] - (sub ? subw * sub[0] : 0.0);
    return 0.5 * first - (T > 0 ? tr / (2.0 * double(T)) : std::numeric_limits<double>::quiet_NaN());
  };
  const double dd = combine(h.data(), nullptr, 0.0);
  if (rq.d_diag) *rq.d_diag = dd;
  if (!cg->have_noise) *rq.d_variance = combine(h.data() + S, h.data(), par.diag) / par.variance;   // K v = Khat v - diag v
  else *rq.d_variance = (combine(h.data() + S, nullptr, 0.0) - h[size_t(d + 2) * size_t(S) + 1]) / par.variance;   // K v = Khat v - D v
  for (int c = 0; c < d; ++c) rq.d_inv_lengthscale[c] = combine(h.data() + size_t(2 + c) * size_t(S), nullptr, 0.0) / par.invl[c];
  if (rq.d_mean_const) *rq.d_mean_const = h[size_t(d + 2) * size_t(S)];
  return SVGP_OK;
}

// d lml / d x after fit_hyper_grad: U = fitX = [alpha, w_t], P = fitB = [alpha, p_t] on the device.
//   Lp = [alpha, w_t .., p_t ..],  Rp = [alpha, -p_t / 2T .., -w_t / 2T ..]  (each entry of Rp rounded once to the data dtype)
int xgrad_enqueue(svgp_ctx* ctx, svgp_cg* cg, const CgPar& par, int32_t T, const svgp_input_grad* gx) {
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype;
  const int64_t N = cg->N, S2 = 2 * int64_t(T) + 1;
  const size_t col = size_t(N) * cg->es;
  char *L = cg->xL.as<char>(), *R = cg->xR.as<char>();
  const char *U = cg->fitX.as<char>(), *P = cg->fitB.as<char>();
  const double w = -1.0 / (2.0 * double(T));
  HIPC(ctx, hipMemcpyAsync(L, U, col * size_t(T + 1), hipMemcpyDeviceToDevice, s));
  HIPC(ctx, hipMemcpyAsync(L + col * size_t(T + 1), P + col, col * size_t(T), hipMemcpyDeviceToDevice, s));
  HIPC(ctx, hipMemcpyAsync(R, U, col, hipMemcpyDeviceToDevice, s));
  launch_cg_affine(dt, s, P + col, 0, N, N, T, w, 0.0, R + col, N);
  launch_cg_affine(dt, s, U + col, 0, N, N, T, w, 0.0, R + col * size_t(T + 1), N);
  CgXgradArgs a{};
  a.rows = cg->rows.p;
  a.bias = cg->bias.p;
  a.invl = cg->invl.p;
  a.x = cg->data->x.p;
  a.Lp = L;
  a.Rp = R;
  a.part = cg->xpart.p;
  a.ldx = cg->data->ldx;
  a.N = N;
  a.Np = cg->Np;
  a.S = S2;
  a.family = par.family;
  a.d = cg->d;
  a.variance = par.variance;
  TREC(ctx, ctx->ev[0], s);
  launch_cg_xgrad(dt, s, a, gx->on_device ? gx->x : cg->xout.p, gx->on_device ? gx->ld : N);
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "cg (input gradient)");
  if (!gx->on_device) HIPC(ctx, hipMemcpy2DAsync(gx->x, size_t(gx->ld) * cg->es, cg->xout.p, col, col, size_t(cg->d), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  cg_timing(ctx);   // the data-sized kernels of the input gradient alone
  return SVGP_OK;
}

// 7. the noise gradient (s_bar as fit_hyper_grad left it) and the input gradient (T = 0: NaN, like the other trace blocks)
int fit_point_grads(FitRun& f) {
  svgp_ctx* ctx = f.ctx;
  svgp_cg* cg = f.cg;
  const FitRequest& rq = f.rq;
  if (rq.gpn) {
    HIPC(ctx, hipMemcpyAsync(rq.gpn->s_bar, cg->sbar.p, f.col, rq.gpn->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (!rq.gx) return SVGP_OK;
  if (rq.T > 0) return xgrad_enqueue(ctx, cg, f.par, rq.T, rq.gx);
  return nan_fill(ctx, cg->dtype, rq.gx->x, rq.gx->ld, f.N, cg->d, rq.gx->on_device);
}

int fit_impl(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* ds, const FitRequest& rq) {
  int rc = fit_check(ctx, cg, ds, rq);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  const bool pc = cg->pc.k > 0;
  FitRun f{ctx, cg, rq, par_of(ds), pc, rq.grad && (rq.gpn || cg->have_noise), cg->N, int64_t(rq.T) + 1, size_t(cg->N) * cg->es, {}, {}};
  cg->have_fit = false;
  if ((rc = fit_reserve(f)) != SVGP_OK) return rc;
  if ((rc = noise_check(ctx, cg, ds, pc)) == SVGP_OK) rc = set_params(ctx, cg, f.par);
  if (rc == SVGP_NOT_POSDEF) return fit_failed(f, rc, nan_info());
  if (rc) return rc;
  if ((rc = fit_rhs(f)) != SVGP_OK) return rc;
  rc = solve_core(ctx, cg, f.par, f.S, cg->fitB.p, f.N, cg->fitX.p, f.N, nullptr, nullptr, &f.out, &f.hist);   // 4. the solve
  if (rc) return fit_failed(f, rc, f.out);
  if ((rc = fit_value(f)) != SVGP_OK) return rc;
  if (rq.grad) {
    if ((rc = fit_hyper_grad(f)) != SVGP_OK) return rc;
    if ((rc = fit_point_grads(f)) != SVGP_OK) return rc;
  }
  if (rq.info) *rq.info = f.out;
  if (rq.lml_out) *rq.lml_out = f.out.lml;
  return SVGP_OK;
}

}  // namespace

namespace svgp {

int stage_delta(svgp_ctx* ctx, svgp_cg* cg, const CgPar& par, const double* delta, void* out) {
  const int64_t N = cg->N;
  if (delta) {
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, delta, size_t(N) * 8, hipMemcpyHostToDevice, ctx->stream));
    launch_cg_affine(cg->dtype, ctx->stream, cg->f64tmp.p, 1, N, N, 1, 1.0, 0.0, out, N);
  } else {
    launch_cg_affine(cg->dtype, ctx->stream, cg->data->y.p, 0, N, N, 1, 1.0, -par.mean_const, out, N);
  }
  return SVGP_OK;
}

}  // namespace svgp

extern "C" {

int32_t svgp_cg_fit(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes, double* lml_out,
                    svgp_cg_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  FitRequest rq;
  rq.delta = delta; rq.T = T; rq.probes = probes;
  rq.lml_out = lml_out; rq.info = info;
  return fit_impl(ctx, cg, desc, rq);
}

int32_t svgp_cg_lml_grad(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                         double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale, double* d_diag,
                         double* d_mean_const) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  FitRequest rq;
  rq.delta = delta; rq.T = T; rq.probes = probes;
  rq.lml_out = lml_out; rq.info = info;
  rq.grad = true; rq.d_variance = d_variance; rq.d_inv_lengthscale = d_inv_lengthscale; rq.d_diag = d_diag; rq.d_mean_const = d_mean_const;
  return fit_impl(ctx, cg, desc, rq);
}

int32_t svgp_cg_fit_precond(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                            const double* probes_k, double* lml_out, svgp_cg_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  FitRequest rq;
  rq.delta = delta; rq.T = T; rq.probes = probes; rq.probes_k = probes_k; rq.precond_call = true;
  rq.lml_out = lml_out; rq.info = info;
  return fit_impl(ctx, cg, desc, rq);
}

int32_t svgp_cg_lml_grad_precond(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                                 const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                                 double* d_diag, double* d_mean_const) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  FitRequest rq;
  rq.delta = delta; rq.T = T; rq.probes = probes; rq.probes_k = probes_k; rq.precond_call = true;
  rq.lml_out = lml_out; rq.info = info;
  rq.grad = true; rq.d_variance = d_variance; rq.d_inv_lengthscale = d_inv_lengthscale; rq.d_diag = d_diag; rq.d_mean_const = d_mean_const;
  return fit_impl(ctx, cg, desc, rq);
}

int32_t svgp_cg_lml_grad_inputs(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                                const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                                double* d_diag, double* d_mean_const, const svgp_input_grad* gx) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!gx || !gx->x) return fail(ctx, SVGP_INVALID_ARG, "null input-gradient output");
  const bool pc = cg->pc.k > 0;
  if (!pc && probes_k) return fail(ctx, SVGP_INVALID_ARG, "probes_k without a preconditioner on this handle (svgp_cg_set_preconditioner)");
  FitRequest rq;
  rq.delta = delta; rq.T = T; rq.probes = probes; rq.probes_k = probes_k; rq.precond_call = pc;
  rq.lml_out = lml_out; rq.info = info;
  rq.grad = true; rq.d_variance = d_variance; rq.d_inv_lengthscale = d_inv_lengthscale; rq.d_diag = d_diag; rq.d_mean_const = d_mean_const;
  rq.gx = gx;
  return fit_impl(ctx, cg, desc, rq);
}

int32_t svgp_cg_lml_grad_noise(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                               const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                               double* d_diag, double* d_mean_const, const svgp_input_grad* gx, svgp_point_noise_grad* gpn) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (gx && !gx->x) return fail(ctx, SVGP_INVALID_ARG, "null input-gradient output");
  if (!gpn || !gpn->s_bar) return fail(ctx, SVGP_INVALID_ARG, "null noise-gradient output");
  const bool pc = cg->pc.k > 0;
  if (!pc && probes_k) return fail(ctx, SVGP_INVALID_ARG, "probes_k without a preconditioner on this handle (svgp_cg_set_preconditioner)");
  FitRequest rq;
  rq.delta = delta; rq.T = T; rq.probes = probes; rq.probes_k = probes_k; rq.precond_call = pc;
  rq.lml_out = lml_out; rq.info = info;
  rq.grad = true; rq.d_variance = d_variance; rq.d_inv_lengthscale = d_inv_lengthscale; rq.d_diag = d_diag; rq.d_mean_const = d_mean_const;
  rq.gx = gx; rq.gpn = gpn;
  return fit_impl(ctx, cg, desc, rq);
}

int32_t svgp_cg_alpha(svgp_ctx* ctx, svgp_cg* cg, void* alpha_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg || !alpha_out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!cg->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_cg_fit on this handle yet");
  HIPC(ctx, hipSetDevice(ctx->device));
  HIPC(ctx, hipMemcpyAsync(alpha_out, cg->fitX.p, size_t(cg->N) * cg->es, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  return SVGP_OK;
}

int32_t svgp_cg_predict(svgp_ctx* ctx, svgp_cg* cg, int32_t layout, int64_t n, const void* x_host, void* mean_out, void* var_out,
                        svgp_cg_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg || !x_host) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!mean_out && !var_out) return fail(ctx, SVGP_INVALID_ARG, "null argument: neither mean nor var is asked for");
  if (cg->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the CG handle lives on another device than the context");
  if (!cg->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_cg_fit on this handle yet");
  if (n < 1) return fail(ctx, SVGP_INVALID_ARG, "no test points");
  if (var_out && cg->pc.k > 0 && !cg->have_noise && !(cg->fit.diag > 0)) return fail(ctx, SVGP_INVALID_ARG, "a preconditioner is set: the fit's diag must be > 0");
  if (var_out && (n > kCgMaxPredict || n * cg->N > kCgMaxPredict))
    return fail(ctx, SVGP_UNSUPPORTED, "the predictive variance of more than 2^28 / N test points in one call");
  if (n > kCgMaxPredict) return fail(ctx, SVGP_UNSUPPORTED, "more than 2^28 test points in one call");
  DataHold h{ctx};
  int rc = svgp_data_upload(ctx, cg->dtype, layout, cg->d, n, x_host, nullptr, &h.D);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype;
  const int64_t N = cg->N;
  const size_t es = cg->es, col = size_t(N) * es;
  const CgPar& par = cg->fit;
  DevBuf mv, Bk, Xk, vres;
  rc = reserve_all(ctx, {{&mv, size_t(n) * es, "the predictions"},
                         {&Bk, var_out ? col * size_t(n) : 0, "k(X, x*)"},
                         {&Xk, var_out ? col * size_t(n) : 0, "Khat^-1 k(X, x*)"},
                         {&vres, var_out ? size_t(n) * 8 : 0, "the predictive variances"}});
  if (rc) return rc;
  if (var_out && (rc = ensure_solver(ctx, cg, n, false, par.maxiter)) != SVGP_OK) return rc;
  if ((rc = set_params(ctx, cg, par, var_out != nullptr)) != SVGP_OK) return rc;   // (the mean needs no preconditioner)
  svgp_cg_info out{};
  out.converged = 1;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  out.quad = out.logdet = out.lml = nan;
  if (mean_out) {
    kmv(ctx, cg, par, h.D->x.p, h.D->ldx, n, cg->fitX.p, N, 1, nullptr, n, mv.p, n);
    launch_cg_affine(dt, s, mv.p, 0, n, n, 1, 1.0, par.mean_const, mv.p, n);
    KCHECK(ctx, "cg (predictive mean)");
    HIPC(ctx, hipMemcpyAsync(mean_out, mv.p, size_t(n) * es, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
  }
  int status = SVGP_OK;
  if (var_out) {
    launch_cg_kcols(dt, s, cg->data->x.p, cg->data->ldx, N, h.D->x.p, h.D->ldx, n, cg->invl.p, cg->d, par.family, par.variance, Bk.p, N);
    KCHECK(ctx, "cg (k(X, x*))");
    status = solve_core(ctx, cg, par, n, Bk.p, N, Xk.p, N, nullptr, nullptr, &out, nullptr);
    if (status != SVGP_OK && status != SVGP_NOT_POSDEF) return status;
    launch_cg_dot(dt, s, Bk.p, N, Xk.p, N, N, n, cg->partial.as<double>());
    launch_cg_colsum(s, cg->partial.as<double>(), N, n, vres.as<double>());
    launch_cg_affine(dt, s, vres.p, 1, n, n, 1, -1.0, par.variance, mv.p, n);   // k** - k*' Khat^-1 k*
    KCHECK(ctx, "cg (predictive variance)");
    HIPC(ctx, hipMemcpyAsync(var_out, mv.p, size_t(n) * es, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));   // (SVGP_NOT_POSDEF: NaN variances, its message kept - nothing above writes one unless it fails)
  }
  if (info) *info = out;
  return status;
}

}  // extern "C"
