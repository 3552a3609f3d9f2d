// cg_solve.hip — the exact GP by matrix-free conjugate gradients, the handle and its solver: svgp_cg_create / _free / _matvec / _solve /
// _set_noise and the host-only svgp_lanczos_logdet (cg.hip: the kernels).  Host orchestration only; cg_host.hpp holds the handle.
// Batched CG over column blocks of 64: per iteration one kmv product (the only O(N^2) work), two column dots, two masked axpy passes;
// the per-column scalars and the CG coefficients of every column stay on the device, the host reads the block's 64 activity flags (and
// one failure flag) per iteration.  log det Khat by stochastic Lanczos quadrature from the caller's probe vectors: the Lanczos
// tridiagonal of a column is rebuilt from its CG coefficients, its eigen-decomposition runs in fp64 on the host.
// Per-point noise variances: Khat = K + diag(sigma^2) with sigma_i^2 = T(diag) + s_i - the vector is handle state, its minimum is
// reduced on the device at set time and every call tests it on the host before its data pass; kmv's epilogue reads sigma^2 per output
// point, the preconditioner's D^-1 scalings are streaming passes around its two products.
#include <memory>
#include <new>

#include "cg_host.hpp"

using namespace svgp;

namespace {

int check_desc(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds) {
  if (!ds) return fail(ctx, SVGP_INVALID_ARG, "null descriptor");
  if (ds->dtype != cg->dtype) return fail(ctx, SVGP_INVALID_ARG, "descriptor and data dtypes differ");
  if (ds->d != cg->d) return fail(ctx, SVGP_INVALID_ARG, "descriptor and data input dimensions differ");
  if (ds->kernel < 0 || ds->kernel > 2) return fail(ctx, SVGP_INVALID_ARG, "unknown kernel family");
  if (!ds->inv_lengthscale) return fail(ctx, SVGP_INVALID_ARG, "null inv_lengthscale");
  if (ds->maxiter < 1) return fail(ctx, SVGP_INVALID_ARG, "maxiter must be >= 1");
  if (!(ds->tol > 0)) return fail(ctx, SVGP_INVALID_ARG, "tol must be > 0");
  if (!(ds->diag >= 0)) return fail(ctx, SVGP_INVALID_ARG, "diag must be >= 0");
  if (!(ds->variance > 0)) return fail(ctx, SVGP_INVALID_ARG, "variance must be > 0");
  if (ds->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved must be 0");
  return SVGP_OK;
}

}  // namespace

namespace svgp {

int common_checks(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds) {
  if (cg->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the CG handle lives on another device than the context");
  return check_desc(ctx, cg, ds);
}

int check_precond_desc(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds) {
  if (cg->have_noise) return SVGP_OK;   // the variances are diag + s_i: noise_check answers for them (SVGP_NOT_POSDEF)
  if (!(ds->diag > 0)) return fail(ctx, SVGP_INVALID_ARG, "a preconditioner is set: diag must be > 0 (P = Z Kuu^-1 Z' + diag I)");
  return SVGP_OK;
}

int noise_check(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds, bool precond) {
  if (!cg->have_noise) return SVGP_OK;
  const double lo = cg->dtype == SVGP_F64 ? ds->diag + cg->noise_min : double(float(ds->diag) + float(cg->noise_min));
  if (lo != lo) return fail(ctx, SVGP_NOT_POSDEF, "per-point noise: a variance diag + s_i is NaN");
  if (lo < 0) return fail(ctx, SVGP_NOT_POSDEF, "per-point noise: a variance diag + s_i is negative");
  if (precond && !(lo > 0)) return fail(ctx, SVGP_NOT_POSDEF, "per-point noise: a variance diag + s_i is zero with a preconditioner set (P = Z Kuu^-1 Z' + D)");
  return SVGP_OK;
}

CgPar par_of(const svgp_cg_desc* ds) {
  CgPar p;
  p.family = ds->kernel;
  p.maxiter = ds->maxiter;
  p.variance = ds->variance;
  p.diag = ds->diag;
  p.mean_const = ds->mean_const;
  p.tol = ds->tol;
  p.invl.assign(ds->inv_lengthscale, ds->inv_lengthscale + ds->d);
  return p;
}

int set_params(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, bool precond) {
  hipStream_t s = ctx->stream;
  const int d = cg->d;
  int rc = reserve_all(ctx, {{&cg->invl, size_t(SVGP_MAX_D) * 8, "the CG handle"},
                             {&cg->rows, size_t(d) * size_t(cg->Np) * cg->es, "the CG handle's rows"},
                             {&cg->bias, size_t(cg->Np) * cg->es, "the CG handle's bias"}});
  if (rc) return rc;
  double il64[SVGP_MAX_D];
  float il32[SVGP_MAX_D];
  for (int f = 0; f < d; ++f) {
    il64[f] = p.invl[f];
    il32[f] = float(p.invl[f]);
  }
  HIPC(ctx, hipMemcpyAsync(cg->invl.p, cg->dtype == SVGP_F64 ? (const void*)il64 : (const void*)il32, size_t(d) * cg->es, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipStreamSynchronize(s));   // the staging arrays are this frame's
  launch_kmv_prep(cg->dtype, s, cg->data->x.p, cg->data->ldx, cg->invl.p, d, cg->N, cg->Np, cg->rows.p, cg->bias.p);
  KCHECK(ctx, "kmv_prep");
  if (cg->have_noise) {
    const size_t nb = size_t(cg->N) * cg->es;
    const char* what = "the noise variances";
    rc = reserve_all(ctx, {{&cg->sig2, nb, what}, {&cg->isig2, nb, what}, {&cg->ssig2, nb, what}, {&cg->isig64, size_t(cg->N) * 8, what}});
    if (rc) return rc;
    launch_cg_noise_prep(cg->dtype, s, cg->noise_s.p, cg->N, p.diag, cg->sig2.p, cg->isig2.p, cg->ssig2.p, cg->isig64.as<double>());
    KCHECK(ctx, "cg (noise variances)");
  }
  if (precond && cg->pc.k > 0) return pc_setup(ctx, cg, p);
  return SVGP_OK;
}

void kmv(svgp_ctx* ctx, const svgp_cg* cg, const CgPar& p, const void* px, int64_t ldp, int64_t n, const void* V, int64_t ldv, int64_t S,
         const void* addv, int64_t lda, void* out, int64_t ldo, int profile, int coord) {
  KmvArgs a = kmv_args(cg, p);
  a.px = px;
  a.V = V;
  a.addv = addv;
  a.dvec = (addv && cg->have_noise) ? cg->sig2.p : nullptr;   // Khat = K + diag(sig2); addv is only ever passed with the data as the points
  a.out = out;
  a.ldp = ldp;
  a.n = n;
  a.ldv = ldv;
  a.lda = lda;
  a.ldo = ldo;
  a.S = S;
  a.profile = profile;
  a.coord = coord;
  a.self = (px == cg->data->x.p && n == cg->N) ? 1 : 0;
  a.diag = p.diag;
  launch_kmv(cg->dtype, ctx->stream, a);
}

int ensure_solver(svgp_ctx* ctx, svgp_cg* cg, int64_t dot_cols, bool want_hist, int maxiter) {
  const int64_t cols = dot_cols < 64 ? 64 : dot_cols;
  return reserve_all(ctx, {{&cg->ws, size_t(cg->pc.k > 0 ? 6 : 5) * size_t(cg->N) * 64 * cg->es, "the CG workspace"},   // (z = P^-1 r)
                           {&cg->st, size_t(CgState::WORDS) * 8, "the CG state"},
                           {&cg->partial, size_t(cols) * size_t(cg_dot_blocks(cg->N)) * 8, "the CG dot partials"},
                           {&cg->hist, want_hist ? size_t(2) * size_t(maxiter) * 64 * 8 : 0, "the CG coefficient history"}});
}

// (cg_host.hpp: the contract.)  With a preconditioner set (pc.k > 0)
// the recurrence is the preconditioned one: z = P^-1 r, rho = r'z, a = rho / p'q, beta = rho_new / rho, p = z + beta p; the stopping
// test stays on the true residual, and a, beta rebuild the Lanczos tridiagonal of P^-1/2 Khat P^-1/2 started at P^-1/2 b.
int solve_core(svgp_ctx* ctx, svgp_cg* cg, const CgPar& par, int64_t S, const void* B, int64_t ldb, void* X, int64_t ldx, int32_t* iters_out,
               double* relres_out, svgp_cg_info* info, CgHist* hist) {
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype;
  const int64_t N = cg->N;
  const size_t es = cg->es, col = size_t(N) * es;
  char* w = cg->ws.as<char>();
  void *x = w, *r = w + 64 * col, *p = w + 128 * col, *q = w + 192 * col;
  const bool pc = cg->pc.k > 0;
  void* z = pc ? w + 320 * col : nullptr;
  double* rho = pc ? cg->pc.rho.as<double>() : nullptr;
  int rc;
  double* st = cg->st.as<double>();
  double* partial = cg->partial.as<double>();
  double* ha = hist ? cg->hist.as<double>() : nullptr;
  double* hb = hist ? ha + size_t(par.maxiter) * 64 : nullptr;
  const double tol2 = par.tol * par.tol;
  svgp_cg_info out{};
  out.converged = 1;
  double ms_mv = 0, ms_vec = pc ? cg->pc.ms_setup : 0;
  if (pc) cg->pc.ms_setup = 0;   // (counted once)
  bool bad = false;
  if (hist) {
    hist->a.assign(size_t(S), {});
    hist->b.assign(size_t(S), {});
    hist->bb.assign(size_t(S), 0.0);
  }
  std::vector<double> ha_h, hb_h;
  for (int64_t c0 = 0; c0 < S && !bad; c0 += 64) {
    const int nc = int(S - c0 < 64 ? S - c0 : 64);
    const char* Bc = static_cast<const char*>(B) + size_t(c0) * size_t(ldb) * es;
    HIPC(ctx, hipMemcpy2DAsync(r, col, Bc, size_t(ldb) * es, col, size_t(nc), hipMemcpyDeviceToDevice, s));
    if (!pc) HIPC(ctx, hipMemcpyAsync(p, r, col * nc, hipMemcpyDeviceToDevice, s));
    HIPC(ctx, hipMemsetAsync(x, 0, col * nc, s));
    HIPC(ctx, hipMemsetAsync(st, 0, size_t(CgState::WORDS) * 8, s));
    launch_cg_dot(dt, s, r, N, r, N, N, nc, partial);
    launch_cg_coef(s, 0, st, partial, N, nc, 0, tol2, nullptr, nullptr);
    if (pc) {
      if ((rc = pc_apply(ctx, cg, par, r, N, nc, z, N)) != SVGP_OK) return rc;
      HIPC(ctx, hipMemcpyAsync(p, z, col * nc, hipMemcpyDeviceToDevice, s));
      launch_cg_dot(dt, s, r, N, z, N, N, nc, partial);
      launch_cg_coef(s, 3, st, partial, N, nc, 0, tol2, nullptr, nullptr, rho);
    }
    KCHECK(ctx, "cg (initial norms)");
    double flags[CgState::WORDS - CgState::ACT];
    HIPC(ctx, hipMemcpyAsync(flags, st + CgState::ACT, sizeof flags, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    auto any_active = [&] {
      for (int j = 0; j < nc; ++j)
        if (flags[j] != 0.0) return true;
      return false;
    };
    int k = 0;
    bad = flags[CgState::BAD - CgState::ACT] != 0.0;
    while (!bad && k < par.maxiter && any_active()) {
      TREC(ctx, ctx->ev[0], s);
      kmv(ctx, cg, par, cg->data->x.p, cg->data->ldx, N, p, N, nc, p, N, q, N);
      TREC(ctx, ctx->ev[1], s);
      launch_cg_dot(dt, s, p, N, q, N, N, nc, partial);
      launch_cg_coef(s, 1, st, partial, N, nc, k, tol2, ha, hb, rho);
      launch_cg_update_xr(dt, s, st, N, nc, x, r, p, q);
      launch_cg_dot(dt, s, r, N, r, N, N, nc, partial);
      if (!pc) {
        launch_cg_coef(s, 2, st, partial, N, nc, k, tol2, ha, hb);
        launch_cg_update_p(dt, s, st, N, nc, r, p);
      } else {
        launch_cg_coef(s, 4, st, partial, N, nc, k, tol2, ha, hb, rho);
        if ((rc = pc_apply(ctx, cg, par, r, N, nc, z, N)) != SVGP_OK) return rc;
        launch_cg_dot(dt, s, r, N, z, N, N, nc, partial);
        launch_cg_coef(s, 5, st, partial, N, nc, k, tol2, ha, hb, rho);
        launch_cg_update_p(dt, s, st, N, nc, z, p);
      }
      TREC(ctx, ctx->ev[2], s);
      KCHECK(ctx, "cg (iteration)");
      HIPC(ctx, hipMemcpyAsync(flags, st + CgState::ACT, sizeof flags, hipMemcpyDeviceToHost, s));
      HIPC(ctx, hipStreamSynchronize(s));
      float t = 0;
      if (elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]) == hipSuccess) ms_mv += t;
      if (elapsed_ms(ctx, &t, ctx->ev[1], ctx->ev[2]) == hipSuccess) ms_vec += t;
      bad = flags[CgState::BAD - CgState::ACT] != 0.0;
      ++k;
    }
    if (bad) break;
    double sth[CgState::WORDS], rho0[64] = {0};
    HIPC(ctx, hipMemcpyAsync(sth, st, sizeof sth, hipMemcpyDeviceToHost, s));
    if (pc) HIPC(ctx, hipMemcpyAsync(rho0, rho + 64, sizeof rho0, hipMemcpyDeviceToHost, s));
    if (hist && k > 0) {
      ha_h.resize(size_t(k) * 64);
      hb_h.resize(size_t(k) * 64);
      HIPC(ctx, hipMemcpyAsync(ha_h.data(), ha, size_t(k) * 64 * 8, hipMemcpyDeviceToHost, s));
      HIPC(ctx, hipMemcpyAsync(hb_h.data(), hb, size_t(k) * 64 * 8, hipMemcpyDeviceToHost, s));
    }
    char* Xc = static_cast<char*>(X) + size_t(c0) * size_t(ldx) * es;
    HIPC(ctx, hipMemcpy2DAsync(Xc, size_t(ldx) * es, x, col, col, size_t(nc), hipMemcpyDeviceToDevice, s));
    HIPC(ctx, hipStreamSynchronize(s));
    for (int j = 0; j < nc; ++j) {
      const int it = int(sth[CgState::IT + j]);
      const double bb = sth[CgState::BB + j], rr = sth[CgState::RR + j];
      const double rel = bb > 0 ? std::sqrt(rr / bb) : 0.0;
      if (iters_out) iters_out[c0 + j] = it;
      if (relres_out) relres_out[c0 + j] = rel;
      if (it > out.iterations) out.iterations = it;
      if (sth[CgState::ACT + j] != 0.0) {
        out.converged = 0;
        ++out.n_unconverged;
      }
      if (rel > out.max_rel_residual || rel != rel) out.max_rel_residual = rel;
      if (hist) {
        hist->bb[size_t(c0 + j)] = pc ? rho0[j] : bb;
        auto& va = hist->a[size_t(c0 + j)];
        auto& vb = hist->b[size_t(c0 + j)];
        va.resize(size_t(it));
        vb.resize(size_t(it));
        for (int q2 = 0; q2 < it; ++q2) {
          va[size_t(q2)] = ha_h[size_t(q2) * 64 + j];
          vb[size_t(q2)] = hb_h[size_t(q2) * 64 + j];
        }
      }
    }
  }
  out.ms_matvec = ms_mv;
  out.ms_vector = ms_vec;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (bad) {
    if ((rc = nan_fill(ctx, dt, X, ldx, N, S, true)) != SVGP_OK) return rc;
    for (int64_t j = 0; j < S; ++j) {
      if (iters_out) iters_out[j] = 0;
      if (relres_out) relres_out[j] = nan;
    }
    if (info) *info = nan_info();
    if (pc)
      return fail(ctx, SVGP_NOT_POSDEF, "conjugate gradients: a curvature p' Khat p or a product r' P^-1 r is not positive (Khat or the applied "
                                        "preconditioner is not positive definite, or holds a NaN)");
    return fail(ctx, SVGP_NOT_POSDEF, "conjugate gradients: a curvature p' Khat p is not positive (Khat is not positive definite, or holds a NaN)");
  }
  out.quad = out.logdet = out.lml = nan;
  if (info) *info = out;
  return SVGP_OK;
}

// e1' log(T) e1 of the Lanczos tridiagonal rebuilt from the CG coefficients a[0..m), b[0..m): diagonal 1 / a_j + b_{j-1} / a_{j-1},
// off-diagonal sqrt(b_j) / a_j.  Symmetric tridiagonal QL with implicit shifts, carrying the first row of the eigenvector matrix.
int lanczos_quadrature(const double* ca, const double* cb, int m, double* out) {
  const size_t mz = static_cast<size_t>(m);
  std::vector<double> d(mz, 0.0), e(mz, 0.0), z(mz, 0.0);
  for (int j = 0; j < m; ++j) {
    d[j] = 1.0 / ca[j] + (j > 0 ? cb[j - 1] / ca[j - 1] : 0.0);
    if (j + 1 < m) e[j] = std::sqrt(cb[j]) / ca[j];
  }
  z[0] = 1.0;
  const int n = m;
  for (int l = 0; l < n; ++l) {
    int iter = 0, mm;
    do {
      for (mm = l; mm < n - 1; ++mm) {
        const double dd = std::fabs(d[mm]) + std::fabs(d[mm + 1]);
        if (!(std::fabs(e[mm]) > 2.3e-16 * dd)) break;
      }
      if (mm != l) {
        if (++iter > 300) return SVGP_INVALID_ARG;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = std::hypot(g, 1.0);
        g = d[mm] - d[l] + e[l] / (g + (g >= 0 ? r : -r));
        double sn = 1.0, cs = 1.0, p = 0.0;
        int i;
        for (i = mm - 1; i >= l; --i) {
          double f = sn * e[i];
          const double b = cs * e[i];
          r = std::hypot(f, g);
          e[i + 1] = r;
          if (r == 0.0) {
            d[i + 1] -= p;
            e[mm] = 0.0;
            break;
          }
          sn = f / r;
          cs = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * sn + 2.0 * cs * b;
          p = sn * r;
          d[i + 1] = g + p;
          g = cs * r - b;
          f = z[i + 1];
          z[i + 1] = sn * z[i] + cs * f;
          z[i] = cs * z[i] - sn * f;
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p;
        e[l] = g;
        e[mm] = 0.0;
      }
    } while (mm != l);
  }
  // sum the terms in ascending order of the eigenvalue: a fixed order
  std::vector<int> idx(static_cast<size_t>(n), 0);
  for (int i = 0; i < n; ++i) idx[i] = i;
  for (int i = 1; i < n; ++i) {
    const int kx = idx[i];
    int j = i - 1;
    while (j >= 0 && d[idx[j]] > d[kx]) {
      idx[j + 1] = idx[j];
      --j;
    }
    idx[j + 1] = kx;
  }
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double lam = d[idx[i]];
    if (!(lam > 0)) {
      *out = std::numeric_limits<double>::quiet_NaN();
      return SVGP_NOT_POSDEF;
    }
    sum += z[idx[i]] * z[idx[i]] * std::log(lam);
  }
  *out = sum;
  return SVGP_OK;
}

}  // namespace svgp

extern "C" {

int32_t svgp_lanczos_logdet(const double* a, const double* b, int32_t iters, double* out) {
  if (!a || !b || !out || iters < 1) return SVGP_INVALID_ARG;
  return lanczos_quadrature(a, b, iters, out);
}

int32_t svgp_cg_create(svgp_ctx* ctx, const svgp_data* data, svgp_cg** out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!data || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  *out = nullptr;
  if (data->n < 1) return fail(ctx, SVGP_INVALID_ARG, "empty data");
  if (data->d < 1 || data->d > SVGP_MAX_D) return fail(ctx, SVGP_UNSUPPORTED, "input dimension beyond SVGP_MAX_D");
  std::unique_ptr<svgp_cg> cg(new (std::nothrow) svgp_cg());
  if (!cg) return SVGP_OOM;
  cg->data = data;
  cg->dtype = data->dtype;
  cg->d = data->d;
  cg->device = ctx->device;
  cg->es = data->dtype == SVGP_F64 ? 8 : 4;
  cg->N = data->n;
  cg->Np = (data->n + 31) / 32 * 32;
  *out = cg.release();
  return SVGP_OK;
}

int32_t svgp_cg_free(svgp_ctx* ctx, svgp_cg* cg) {
  if (!cg) return SVGP_OK;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  delete cg;
  return SVGP_OK;
}

int32_t svgp_cg_matvec(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* V, int64_t ldv, void* out, int64_t ldo,
                       int32_t on_device) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg || !V || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  int rc = common_checks(ctx, cg, desc);
  if (rc) return rc;
  if (S < 1) return fail(ctx, SVGP_INVALID_ARG, "S must be >= 1");
  if (ldv < cg->N || ldo < cg->N) return fail(ctx, SVGP_INVALID_ARG, "ldv and ldo must be >= N");
  if (on_device != 0 && on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = cg->N;
  const CgPar par = par_of(desc);
  Panel Vp, Op;
  if ((rc = stage_panel(ctx, Vp, V, ldv, N, S, cg->es, on_device, true, "the panel")) != SVGP_OK) return rc;
  if ((rc = stage_panel(ctx, Op, out, ldo, N, S, cg->es, on_device, false, "the product")) != SVGP_OK) return rc;
  const int status = noise_check(ctx, cg, desc, false);
  if (status != SVGP_OK) {   // a bad variance: NaN outputs, the status and its message kept
    if ((rc = nan_fill(ctx, cg->dtype, Op.p, Op.ld, N, S, true)) != SVGP_OK) return rc;
    if ((rc = download_panel(ctx, Op)) != SVGP_OK) return rc;
    HIPC(ctx, hipStreamSynchronize(s));
    return status;
  }
  if ((rc = set_params(ctx, cg, par, false)) != SVGP_OK) return rc;
  TREC(ctx, ctx->ev[0], s);
  kmv(ctx, cg, par, cg->data->x.p, cg->data->ldx, N, Vp.p, Vp.ld, S, Vp.p, Vp.ld, Op.p, Op.ld);
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "kmv");
  if ((rc = download_panel(ctx, Op)) != SVGP_OK) return rc;
  HIPC(ctx, hipStreamSynchronize(s));
  cg_timing(ctx);
  return SVGP_OK;
}

int32_t svgp_cg_solve(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* B, int64_t ldb, void* X, int64_t ldx,
                      int32_t on_device, int32_t* iters_out, double* relres_out, svgp_cg_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg || !B || !X) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  int rc = common_checks(ctx, cg, desc);
  if (rc) return rc;
  if (S < 1) return fail(ctx, SVGP_INVALID_ARG, "S must be >= 1");
  if (ldb < cg->N || ldx < cg->N) return fail(ctx, SVGP_INVALID_ARG, "ldb and ldx must be >= N");
  if (on_device != 0 && on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  if (cg->pc.k > 0 && (rc = check_precond_desc(ctx, cg, desc)) != SVGP_OK) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = cg->N;
  const CgPar par = par_of(desc);
  Panel Bp, Xp;
  if ((rc = stage_panel(ctx, Bp, B, ldb, N, S, cg->es, on_device, true, "the right-hand sides")) != SVGP_OK) return rc;
  if ((rc = stage_panel(ctx, Xp, X, ldx, N, S, cg->es, on_device, false, "the solutions")) != SVGP_OK) return rc;
  if ((rc = ensure_solver(ctx, cg, 64, false, par.maxiter)) != SVGP_OK) return rc;
  int status = noise_check(ctx, cg, desc, cg->pc.k > 0);
  if (status == SVGP_OK) status = set_params(ctx, cg, par);
  if (status == SVGP_NOT_POSDEF) {   // the preconditioner did not factor, or a bad noise variance: NaN outputs, as for a bad curvature
    if ((rc = nan_fill(ctx, cg->dtype, Xp.p, Xp.ld, N, S, true)) != SVGP_OK) return rc;
    if ((rc = download_panel(ctx, Xp)) != SVGP_OK) return rc;
    HIPC(ctx, hipStreamSynchronize(s));
    for (int64_t j = 0; j < S; ++j) {
      if (iters_out) iters_out[j] = 0;
      if (relres_out) relres_out[j] = std::numeric_limits<double>::quiet_NaN();
    }
    if (info) *info = nan_info();
    return status;
  }
  if (status) return status;
  status = solve_core(ctx, cg, par, S, Bp.p, Bp.ld, Xp.p, Xp.ld, iters_out, relres_out, info, nullptr);
  if (status != SVGP_OK && status != SVGP_NOT_POSDEF) return status;
  if (!on_device) {   // (SVGP_NOT_POSDEF: the NaN columns, its message kept - nothing below writes one unless it fails itself)
    if ((rc = download_panel(ctx, Xp)) != SVGP_OK) return rc;
    HIPC(ctx, hipStreamSynchronize(s));
  }
  return status;
}
int32_t svgp_cg_set_noise(svgp_ctx* ctx, svgp_cg* cg, const svgp_point_noise* pn) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (cg->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the CG handle lives on another device than the context");
  if (pn && !pn->s) return fail(ctx, SVGP_INVALID_ARG, "null noise vector");
  if (pn && pn->on_device != 0 && pn->on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  if (pn && pn->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved must be 0");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  HIPC(ctx, hipStreamSynchronize(s));
  cg->have_fit = false;   // alpha belonged to the earlier Khat
  if (!pn) {
    cg->have_noise = false;
    return SVGP_OK;
  }
  cg->have_noise = false;   // (a failure below leaves the handle without a vector)
  const size_t nb = size_t(cg->N) * cg->es;
  int rc;
  if ((rc = cg->noise_s.reserve(ctx, nb, "the noise vector")) != SVGP_OK) return rc;
  if ((rc = cg->noise_lo.reserve(ctx, 8, "the noise vector's minimum")) != SVGP_OK) return rc;
  HIPC(ctx, hipMemcpyAsync(cg->noise_s.p, pn->s, nb, pn->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  launch_cg_noise_min(cg->dtype, s, cg->noise_s.p, cg->N, cg->noise_lo.as<double>());
  KCHECK(ctx, "cg (noise minimum)");
  double lo = 0;
  HIPC(ctx, hipMemcpyAsync(&lo, cg->noise_lo.p, 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  cg->noise_min = lo;
  cg->have_noise = true;
  return SVGP_OK;
}
}  // extern "C"
