// cg_api.hip — the exact GP by matrix-free conjugate gradients: svgp_cg_create / _matvec / _solve / _fit / _lml_grad / _alpha / _predict /
// _free and the host-only svgp_lanczos_logdet (cg.hip: the kernels).  Host orchestration only.
//   Khat = K(x, x) + diag I,  alpha = Khat^-1 delta,  lml = -1/2 (delta' alpha + log det Khat + N log 2 pi)
// Batched CG over column blocks of 64: per iteration one kmv product (the only O(N^2) work), two column dots, two masked axpy passes;
// the per-column scalars and the CG coefficients of every column stay on the device, the host reads the block's 64 activity flags (and
// one failure flag) per iteration.  log det Khat by stochastic Lanczos quadrature from the caller's probe vectors: the Lanczos
// tridiagonal of a column is rebuilt from its CG coefficients, its eigen-decomposition runs in fp64 on the host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"

using namespace svgp;

namespace {
struct CgPar {   // one parameter set, host side
  int family = 0, maxiter = 0;
  double variance = 0, diag = 0, mean_const = 0, tol = 0;
  std::vector<double> invl;
};
}  // namespace

struct svgp_cg {
  const svgp_data* data = nullptr;
  int dtype = 0, d = 0, device = 0;
  size_t es = 8;
  int64_t N = 0, Np = 0;
  DevBuf invl, rows, bias;   // the parameter set of the running call on the device (data dtype): kmv_kernel's operands
  DevBuf ws;                 // five N x 64 arrays of the solver: x, r, p, q and one of staging
  DevBuf st, partial, hist, res;   // fp64: the block's state, dot partials, CG coefficient histories [2][maxiter][64], small results
  DevBuf fitB, fitX, gout;   // N x (T + 1): [delta, z_1 .. z_T], [alpha, w_1 .. w_T] of the last fit; the gradient's products
  DevBuf f64tmp;             // fp64 staging of delta and the probes
  bool have_fit = false;
  CgPar fit;                 // the parameter set alpha belongs to
};

namespace {

constexpr int64_t kCgMaxPredict = int64_t(1) << 28;   // n N elements of the predictive variance's right-hand sides in one call

struct CgHist {   // per column: its CG coefficients and |b|^2
  std::vector<std::vector<double>> a, b;
  std::vector<double> bb;
};

struct DataHold {   // test inputs uploaded for one call
  svgp_ctx* ctx;
  svgp_data* D = nullptr;
  ~DataHold() { if (D) svgp_data_free(ctx, D); }
};

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

// the parameter set on the device: invl in the data dtype, the scaled padded rows and their bias (once per call)
int set_params(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p) {
  hipStream_t s = ctx->stream;
  const int d = cg->d;
  int rc;
  if ((rc = cg->invl.reserve(ctx, size_t(SVGP_MAX_D) * 8, "the CG handle")) != SVGP_OK) return rc;
  if ((rc = cg->rows.reserve(ctx, size_t(d) * size_t(cg->Np) * cg->es, "the CG handle's rows")) != SVGP_OK) return rc;
  if ((rc = cg->bias.reserve(ctx, size_t(cg->Np) * cg->es, "the CG handle's bias")) != SVGP_OK) return rc;
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
  return SVGP_OK;
}

// out = prof(P, X) V (+ diag addv): P the n points px (feature-major, ld ldp), X the handle's data
void kmv(svgp_ctx* ctx, const svgp_cg* cg, const CgPar& p, const void* px, int64_t ldp, int64_t n, const void* V, int64_t ldv, int64_t S,
         const void* addv, int64_t lda, void* out, int64_t ldo, int profile = 0, int coord = 0) {
  KmvArgs a{};
  a.rows = cg->rows.p;
  a.bias = cg->bias.p;
  a.invl = cg->invl.p;
  a.px = px;
  a.V = V;
  a.addv = addv;
  a.out = out;
  a.ldp = ldp;
  a.n = n;
  a.N = cg->N;
  a.Np = cg->Np;
  a.ldv = ldv;
  a.lda = lda;
  a.ldo = ldo;
  a.S = S;
  a.family = p.family;
  a.d = cg->d;
  a.profile = profile;
  a.coord = coord;
  a.self = (px == cg->data->x.p && n == cg->N) ? 1 : 0;
  a.variance = p.variance;
  a.diag = p.diag;
  launch_kmv(cg->dtype, ctx->stream, a);
}

int ensure_solver(svgp_ctx* ctx, svgp_cg* cg, int64_t dot_cols, bool want_hist, int maxiter) {
  int rc;
  if ((rc = cg->ws.reserve(ctx, size_t(5) * size_t(cg->N) * 64 * cg->es, "the CG workspace")) != SVGP_OK) return rc;
  if ((rc = cg->st.reserve(ctx, size_t(CgState::WORDS) * 8, "the CG state")) != SVGP_OK) return rc;
  const int64_t cols = dot_cols < 64 ? 64 : dot_cols;
  if ((rc = cg->partial.reserve(ctx, size_t(cols) * size_t(cg_dot_blocks(cg->N)) * 8, "the CG dot partials")) != SVGP_OK) return rc;
  if (want_hist && (rc = cg->hist.reserve(ctx, size_t(2) * size_t(maxiter) * 64 * 8, "the CG coefficient history")) != SVGP_OK) return rc;
  return SVGP_OK;
}

// X = Khat^-1 B for S columns on the device (data dtype), in blocks of 64.  iters_out / relres_out: per column, host, nullable.
// SVGP_NOT_POSDEF: every column of X is NaN.  The caller has run ensure_solver and set_params.
int solve_core(svgp_ctx* ctx, svgp_cg* cg, const CgPar& par, int64_t S, const void* B, int64_t ldb, void* X, int64_t ldx, int32_t* iters_out,
               double* relres_out, svgp_cg_info* info, CgHist* hist) {
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype;
  const int64_t N = cg->N;
  const size_t es = cg->es, col = size_t(N) * es;
  char* w = cg->ws.as<char>();
  void *x = w, *r = w + 64 * col, *p = w + 128 * col, *q = w + 192 * col;
  double* st = cg->st.as<double>();
  double* partial = cg->partial.as<double>();
  double* ha = hist ? cg->hist.as<double>() : nullptr;
  double* hb = hist ? ha + size_t(par.maxiter) * 64 : nullptr;
  const double tol2 = par.tol * par.tol;
  svgp_cg_info out{};
  out.converged = 1;
  double ms_mv = 0, ms_vec = 0;
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
    HIPC(ctx, hipMemcpyAsync(p, r, col * nc, hipMemcpyDeviceToDevice, s));
    HIPC(ctx, hipMemsetAsync(x, 0, col * nc, s));
    HIPC(ctx, hipMemsetAsync(st, 0, size_t(CgState::WORDS) * 8, s));
    launch_cg_dot(dt, s, r, N, r, N, N, nc, partial);
    launch_cg_coef(s, 0, st, partial, N, nc, 0, tol2, nullptr, nullptr);
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
      launch_cg_coef(s, 1, st, partial, N, nc, k, tol2, ha, hb);
      launch_cg_update_xr(dt, s, st, N, nc, x, r, p, q);
      launch_cg_dot(dt, s, r, N, r, N, N, nc, partial);
      launch_cg_coef(s, 2, st, partial, N, nc, k, tol2, ha, hb);
      launch_cg_update_p(dt, s, st, N, nc, r, p);
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
    double sth[CgState::WORDS];
    HIPC(ctx, hipMemcpyAsync(sth, st, sizeof sth, hipMemcpyDeviceToHost, s));
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
        hist->bb[size_t(c0 + j)] = bb;
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
    launch_cg_affine(dt, s, X, 0, ldx, N, S, 0.0, nan, X, ldx);
    KCHECK(ctx, "cg (NaN outputs)");
    HIPC(ctx, hipStreamSynchronize(s));
    for (int64_t j = 0; j < S; ++j) {
      if (iters_out) iters_out[j] = 0;
      if (relres_out) relres_out[j] = nan;
    }
    out = svgp_cg_info{};
    out.max_rel_residual = out.quad = out.logdet = out.lml = nan;
    if (info) *info = out;
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

// a host matrix (data dtype, column-major, ld) into a dense N x S device buffer and back
int upload_cols(svgp_ctx* ctx, const svgp_cg* cg, DevBuf& b, const void* host, int64_t ld, int64_t S, const char* what) {
  const size_t col = size_t(cg->N) * cg->es;
  const int rc = b.reserve(ctx, col * size_t(S), what);
  if (rc) return rc;
  if (host) HIPC(ctx, hipMemcpy2DAsync(b.p, col, host, size_t(ld) * cg->es, col, size_t(S), hipMemcpyHostToDevice, ctx->stream));
  return SVGP_OK;
}

int common_checks(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds) {
  if (cg->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the CG handle lives on another device than the context");
  return check_desc(ctx, cg, ds);
}

// svgp_cg_fit and svgp_cg_lml_grad: g non-null asks for the gradient {d_variance, d_inv_lengthscale[d], d_diag, d_mean_const}
struct FitGrad { double *dv, *dil, *dd, *dm; };
int fit_impl(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* ds, const double* delta, int32_t T, const double* probes, double* lml_out,
             svgp_cg_info* info, const FitGrad* g) {
  int rc = common_checks(ctx, cg, ds);
  if (rc) return rc;
  if (!delta && !cg->data->y.p) return fail(ctx, SVGP_INVALID_ARG, "the data handle has no y and no delta was given");
  if (T < 0) return fail(ctx, SVGP_INVALID_ARG, "the number of probes must be >= 0");
  if (T > 0 && !probes) return fail(ctx, SVGP_INVALID_ARG, "null probes with T > 0");
  if (g && (!g->dv || !g->dil)) return fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype, d = cg->d;
  const int64_t N = cg->N, S = int64_t(T) + 1;
  const size_t col = size_t(N) * cg->es;
  const CgPar par = par_of(ds);
  cg->have_fit = false;
  if ((rc = ensure_solver(ctx, cg, S, true, par.maxiter)) != SVGP_OK) return rc;
  if ((rc = cg->fitB.reserve(ctx, col * size_t(S), "the CG right-hand sides")) != SVGP_OK) return rc;
  if ((rc = cg->fitX.reserve(ctx, col * size_t(S), "the CG solutions")) != SVGP_OK) return rc;
  if ((rc = cg->f64tmp.reserve(ctx, size_t(N) * size_t(T > 0 ? T : 1) * 8, "the probes")) != SVGP_OK) return rc;
  if ((rc = cg->res.reserve(ctx, (size_t(d + 2) * size_t(S) + 8) * 8, "the CG results")) != SVGP_OK) return rc;
  if (g && (rc = cg->gout.reserve(ctx, col * size_t(S), "the gradient's products")) != SVGP_OK) return rc;
  if ((rc = set_params(ctx, cg, par)) != SVGP_OK) return rc;
  // [delta, z_1 .. z_T], each entry rounded once to the data dtype
  if (delta) {
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, delta, size_t(N) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, 1, 1.0, 0.0, cg->fitB.p, N);
  } else {
    launch_cg_affine(dt, s, cg->data->y.p, 0, N, N, 1, 1.0, -par.mean_const, cg->fitB.p, N);
  }
  if (T > 0) {
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, probes, size_t(N) * size_t(T) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, T, 1.0, 0.0, cg->fitB.as<char>() + col, N);
  }
  KCHECK(ctx, "cg (right-hand sides)");
  CgHist hist;
  svgp_cg_info out{};
  rc = solve_core(ctx, cg, par, S, cg->fitB.p, N, cg->fitX.p, N, nullptr, nullptr, &out, &hist);
  if (rc) {
    if (info) *info = out;
    if (lml_out) *lml_out = out.lml;
    return rc;
  }
  double* partial = cg->partial.as<double>();
  double* res = cg->res.as<double>();
  // quad = delta' alpha
  launch_cg_dot(dt, s, cg->fitB.p, N, cg->fitX.p, N, N, 1, partial);
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
      const auto& a = hist.a[size_t(t)];
      if (a.empty()) continue;   // a zero probe
      double qv = 0;
      if (lanczos_quadrature(a.data(), hist.b[size_t(t)].data(), int(a.size()), &qv) != SVGP_OK) qv = nan;
      logdet += hist.bb[size_t(t)] * qv;
    }
    logdet /= double(T);
  }
  out.quad = quad;
  out.logdet = logdet;
  out.lml = -0.5 * (quad + logdet + double(N) * 1.8378770664093454836);
  cg->fit = par;
  cg->have_fit = true;
  if (g) {
    // the panel [alpha, z_1 .. z_T]: delta has served
    HIPC(ctx, hipMemcpyAsync(cg->fitB.p, cg->fitX.p, col, hipMemcpyDeviceToDevice, s));
    const void *U = cg->fitX.p, *P = cg->fitB.p;
    void* O = cg->gout.p;
    launch_cg_dot(dt, s, U, N, P, N, N, S, partial);
    launch_cg_colsum(s, partial, N, S, res);
    kmv(ctx, cg, par, cg->data->x.p, cg->data->ldx, N, P, N, S, P, N, O, N);
    launch_cg_dot(dt, s, U, N, O, N, N, S, partial);
    launch_cg_colsum(s, partial, N, S, res + S);
    for (int f = 0; f < d; ++f) {
      kmv(ctx, cg, par, cg->data->x.p, cg->data->ldx, N, P, N, S, nullptr, N, O, N, 1, f);
      launch_cg_dot(dt, s, U, N, O, N, N, S, partial);
      launch_cg_colsum(s, partial, N, S, res + int64_t(2 + f) * S);
    }
    launch_cg_affine(dt, s, O, 0, N, N, 1, 0.0, 1.0, O, N);   // ones
    launch_cg_dot(dt, s, U, N, O, N, N, 1, partial);
    launch_cg_colsum(s, partial, N, 1, res + int64_t(2 + d) * S);
    KCHECK(ctx, "cg (gradient)");
    std::vector<double> h(size_t(d + 2) * size_t(S) + 1);
    HIPC(ctx, hipMemcpyAsync(h.data(), res, h.size() * 8, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    auto combine = [&](const double* v, const double* sub, double subw) {   //  1/2 v_0 - 1/(2T) sum_t v_t, t ascending
      double tr = 0.0;
      for (int t = 1; t <= T; ++t) tr += v[t] - (sub ? subw * sub[t] : 0.0);
      const double first = v[0] - (sub ? subw * sub[0] : 0.0);
      return 0.5 * first - (T > 0 ? tr / (2.0 * double(T)) : nan);
    };
    const double dd = combine(h.data(), nullptr, 0.0);
    if (g->dd) *g->dd = dd;
    *g->dv = combine(h.data() + S, h.data(), par.diag) / par.variance;   // K v = Khat v - diag v
    for (int f = 0; f < d; ++f) g->dil[f] = combine(h.data() + size_t(2 + f) * size_t(S), nullptr, 0.0) / par.invl[f];
    if (g->dm) *g->dm = h[size_t(d + 2) * size_t(S)];
  }
  if (info) *info = out;
  if (lml_out) *lml_out = out.lml;
  return SVGP_OK;
}

}  // namespace

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
  const size_t col = size_t(N) * cg->es;
  const CgPar par = par_of(desc);
  DevBuf Vd, Od;
  if (!on_device) {
    if ((rc = upload_cols(ctx, cg, Vd, V, ldv, S, "the panel")) != SVGP_OK) return rc;
    if ((rc = upload_cols(ctx, cg, Od, nullptr, N, S, "the product")) != SVGP_OK) return rc;
  }
  if ((rc = set_params(ctx, cg, par)) != SVGP_OK) return rc;
  const void* vp = on_device ? V : Vd.p;
  void* op = on_device ? out : Od.p;
  const int64_t lv = on_device ? ldv : N, lo = on_device ? ldo : N;
  TREC(ctx, ctx->ev[0], s);
  kmv(ctx, cg, par, cg->data->x.p, cg->data->ldx, N, vp, lv, S, vp, lv, op, lo);
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "kmv");
  if (!on_device) HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * cg->es, Od.p, col, col, size_t(S), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_strip = t;
  ctx->timing.ms_total = t;
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
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = cg->N;
  const size_t col = size_t(N) * cg->es;
  const CgPar par = par_of(desc);
  DevBuf Bd, Xd;
  if (!on_device) {
    if ((rc = upload_cols(ctx, cg, Bd, B, ldb, S, "the right-hand sides")) != SVGP_OK) return rc;
    if ((rc = upload_cols(ctx, cg, Xd, nullptr, N, S, "the solutions")) != SVGP_OK) return rc;
  }
  if ((rc = ensure_solver(ctx, cg, 64, false, par.maxiter)) != SVGP_OK) return rc;
  if ((rc = set_params(ctx, cg, par)) != SVGP_OK) return rc;
  rc = solve_core(ctx, cg, par, S, on_device ? B : Bd.p, on_device ? ldb : N, on_device ? X : Xd.p, on_device ? ldx : N, iters_out, relres_out,
                  info, nullptr);
  if (rc != SVGP_OK && rc != SVGP_NOT_POSDEF) return rc;
  if (!on_device) {
    const std::string keep = ctx->err;
    HIPC(ctx, hipMemcpy2DAsync(X, size_t(ldx) * cg->es, Xd.p, col, col, size_t(S), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    ctx->err = keep;
  }
  return rc;
}

int32_t svgp_cg_fit(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes, double* lml_out,
                    svgp_cg_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  return fit_impl(ctx, cg, desc, delta, T, probes, lml_out, info, nullptr);
}

int32_t svgp_cg_lml_grad(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                         double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale, double* d_diag,
                         double* d_mean_const) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  const FitGrad g{d_variance, d_inv_lengthscale, d_diag, d_mean_const};
  return fit_impl(ctx, cg, desc, delta, T, probes, lml_out, info, &g);
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
  if ((rc = mv.reserve(ctx, size_t(n) * es, "the predictions")) != SVGP_OK) return rc;
  if (var_out) {
    if ((rc = Bk.reserve(ctx, col * size_t(n), "k(X, x*)")) != SVGP_OK) return rc;
    if ((rc = Xk.reserve(ctx, col * size_t(n), "Khat^-1 k(X, x*)")) != SVGP_OK) return rc;
    if ((rc = vres.reserve(ctx, size_t(n) * 8, "the predictive variances")) != SVGP_OK) return rc;
    if ((rc = ensure_solver(ctx, cg, n, false, par.maxiter)) != SVGP_OK) return rc;
  }
  if ((rc = set_params(ctx, cg, par)) != SVGP_OK) return rc;
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
    const std::string keep = ctx->err;
    launch_cg_dot(dt, s, Bk.p, N, Xk.p, N, N, n, cg->partial.as<double>());
    launch_cg_colsum(s, cg->partial.as<double>(), N, n, vres.as<double>());
    launch_cg_affine(dt, s, vres.p, 1, n, n, 1, -1.0, par.variance, mv.p, n);   // k** - k*' Khat^-1 k*
    KCHECK(ctx, "cg (predictive variance)");
    HIPC(ctx, hipMemcpyAsync(var_out, mv.p, size_t(n) * es, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    ctx->err = keep;
  }
  if (info) *info = out;
  return status;
}

}  // extern "C"
