// cg_host.hpp — what crosses the host-only units of the exact GP by conjugate gradients (cg_solve.hip, cg_precond.hip, cg_fit.hip,
// cg_sampler_api.hip; the kernels are cg.hip, cg_sample.hip and cg_xgrad.hip): the handles, the declarations of the functions that cross
// the units, each under the unit that defines it, and the small helpers every unit repeats.  A function used by one unit only lives in
// that unit's anonymous namespace.  Not part of the C-ABI.
//   Khat = K(x, x) + diag I,  alpha = Khat^-1 delta,  lml = -1/2 (delta' alpha + log det Khat + N log 2 pi)
#pragma once
#include <cmath>
#include <initializer_list>
#include <limits>
#include <string>
#include <vector>

#include "host.hpp"

namespace svgp {
struct CgPar {   // one parameter set, host side
  int family = 0, maxiter = 0;
  double variance = 0, diag = 0, mean_const = 0, tol = 0;
  std::vector<double> invl;
};
}  // namespace svgp

// The Nystrom preconditioner P = Z Kuu^-1 Z' + sigma^2 I, Z = K(X, z_p) for k points z_p, Kuu = K(z_p, z_p) + jitter variance I = Lu Lu':
//   P^-1 r = (r - Z W Z' r) / sigma^2,  W = Lu^-T B^-1 Lu^-1 / sigma^2,  B = I + Lu^-1 (Z'Z) Lu^-T / sigma^2,  log det P = N log sigma^2 + log det B
// Z' r is the row-split product (launch_kmv_split), Z c the existing kmv_kernel with the k points as its rows, whose epilogue adds
// r / sigma^2.  The k-sized stage (Kuu, Lu, the Gram Z'Z, B, its factor, W) is fp64 for both data dtypes: the Gram is accumulated in
// fp64 from fp64 entries (in float32 accumulation B is not positive definite), so an fp32 handle widens x and z_p for the setup.
struct CgPrecond {
  int64_t k = 0, kp = 0, Mp = 0;   // points, padded to 32 (kmv's chunk) and to 128 (the factorisations' tile)
  double jitter = 0;
  svgp_data* z = nullptr;          // the points, data dtype, feature-major
  svgp::DevBuf rows, bias;               // kmv_prep of the points under the running parameter set (data dtype)
  svgp::DevBuf part, t, v;               // the split product's partials; Z' r and -W Z' r / sigma^2 (kp x S, data dtype)
  svgp::DevBuf x64, z64, invl64, rows64, bias64;   // fp32 handles: the fp64 operands of the Gram
  svgp::DevBuf zblk;                     // N x 64 fp64: a column block of Z
  svgp::DevBuf zs64, Lu, Tu, LinvRM, LinvCM, Ytmp, G, H, H2, Bm, TB, LBinvRM, LBinvCM, W, info, info_b, scal;   // fp64, Mp x Mp
  svgp::DevBuf rho, xi;                  // the solver's r'z words; the k x T probes
  bool x64_ready = false, z64_ready = false;   // x of a handle never changes; the points change with set_preconditioner
  double s2 = 0, logdet_p = 0, ms_setup = 0;
};

struct svgp_cg {
  const svgp_data* data = nullptr;
  int dtype = 0, d = 0, device = 0;
  size_t es = 8;
  int64_t N = 0, Np = 0;
  svgp::DevBuf invl, rows, bias;   // the parameter set of the running call on the device (data dtype): kmv_kernel's operands
  svgp::DevBuf ws;                 // five N x 64 arrays of the solver: x, r, p, q and one of staging
  svgp::DevBuf st, partial, hist, res;   // fp64: the block's state, dot partials, CG coefficient histories [2][maxiter][64], small results
  svgp::DevBuf fitB, fitX, gout;   // N x (T + 1): [delta, z_1 .. z_T], [alpha, w_1 .. w_T] of the last fit; the gradient's products
  svgp::DevBuf f64tmp;             // fp64 staging of delta and the probes
  svgp::DevBuf xL, xR, xpart, xout;   // d lml / d x: the N x (2T + 1) panels, the column blocks' partial sums (fp64), a host output's staging
  bool have_fit = false;
  svgp::CgPar fit;           // the parameter set alpha belongs to
  // per-point noise (svgp_cg_set_noise): the snapshot s and its min (NaN-propagating, reduced on the device at set time); per call
  // sig2 = T(diag) + s, 1 / sig2, sqrt(sig2) in the data dtype, 1 / sig2 in fp64 (the Gram's weights); d lml / d sigma_i^2
  bool have_noise = false;
  double noise_min = 0;
  svgp::DevBuf noise_s, sig2, isig2, ssig2, isig64, sbar;
  svgp::DevBuf noise_lo;           // one fp64 word: the min-reduction's result (kept, so that setting a vector every step allocates nothing)
  CgPrecond pc;              // pc.k == 0: none
  ~svgp_cg() { delete pc.z; }
};

// S function samples of the exact GP's posterior: a snapshot that owns everything its evaluations read
struct svgp_cg_sampler {
  int dtype = 0, d = 0, family = 0, device = 0;
  size_t es = 8;
  int64_t N = 0, Np = 0, L = 0, Lp = 0, S = 0;
  int64_t seg_rows = 0, round = 0;   // cg_sample_plan(N)
  int nseg = 1;
  double variance = 0, mean_const = 0;
  svgp::DevBuf invl, rows, bias;     // the parameter set and the prepared data rows (launch_kmv_prep), data dtype
  svgp::DevBuf frows, fbias, W, V;   // omega [d][Lp], tau [Lp], amp W (Lp x S), V (N x S), data dtype
  std::vector<int32_t> iters;  // per column, of the solve
  std::vector<double> relres;
};

namespace svgp {

struct CgHist {   // per column: its CG coefficients and |b|^2 (preconditioned: b' P^-1 b, the weight of its quadrature)
  std::vector<std::vector<double>> a, b;
  std::vector<double> bb;
};

// ---- cg_solve.hip -----------------------------------------------------------------------------------------------------------
// the handle's device, then the descriptor against the handle
int common_checks(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds);
int check_precond_desc(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds);   // a preconditioner is set: diag > 0
// a noise vector is set: the smallest variance T(diag) + min s of the call's descriptor, before any data pass.  SVGP_NOT_POSDEF when it
// is < 0 (<= 0 where the preconditioner divides by it) or NaN
int noise_check(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds, bool precond);
CgPar par_of(const svgp_cg_desc* ds);
// the parameter set on the device: invl in the data dtype, the scaled padded rows and their bias (once per call); precond: the
// preconditioner's setup as well, when one is set
int set_params(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, bool precond = true);
// out = prof(P, X) V (+ diag addv): P the n points px (feature-major, ld ldp), X the handle's data
void kmv(svgp_ctx* ctx, const svgp_cg* cg, const CgPar& p, const void* px, int64_t ldp, int64_t n, const void* V, int64_t ldv, int64_t S,
         const void* addv, int64_t lda, void* out, int64_t ldo, int profile = 0, int coord = 0);
int ensure_solver(svgp_ctx* ctx, svgp_cg* cg, int64_t dot_cols, bool want_hist, int maxiter);
// X = Khat^-1 B for S columns on the device (data dtype), in blocks of 64.  iters_out / relres_out: per column, host, nullable.
// SVGP_NOT_POSDEF: every column of X is NaN.  The caller has run ensure_solver and set_params.
int solve_core(svgp_ctx* ctx, svgp_cg* cg, const CgPar& par, int64_t S, const void* B, int64_t ldb, void* X, int64_t ldx, int32_t* iters_out,
               double* relres_out, svgp_cg_info* info, CgHist* hist);
// e1' log(T) e1 of the Lanczos tridiagonal rebuilt from the CG coefficients a[0..m), b[0..m)
int lanczos_quadrature(const double* ca, const double* cb, int m, double* out);

// ---- cg_precond.hip ---------------------------------------------------------------------------------------------------------
// out = K(X, z_p) V + diag addv: kmv_kernel with the k points as its rows (V: kp x S, zero on the padding rows)
void pc_expand(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* V, int64_t S, const void* addv, int64_t lda, double diag, void* out, int64_t ldo,
               const void* dvec = nullptr);
// out = P^-1 R for S columns on the device (data dtype); out must not alias R
int pc_apply(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* R, int64_t ldr, int64_t S, void* out, int64_t ldo);
// the preconditioner of one parameter set: the points' rows, Kuu = Lu Lu', the Gram Z'Z, B and its factor, W, log det P
int pc_setup(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p);

// ---- cg_fit.hip -------------------------------------------------------------------------------------------------------------
// delta into `out` (N, device), each entry rounded once to the data dtype: the caller's fp64 vector through f64tmp (reserved by the
// caller), or y - mean_const
int stage_delta(svgp_ctx* ctx, svgp_cg* cg, const CgPar& par, const double* delta, void* out);

// ---- the helpers every unit shares --------------------------------------------------------------------------------------------
inline svgp_cg_info nan_info() {   // the info of a call that returns SVGP_NOT_POSDEF
  svgp_cg_info i{};
  i.max_rel_residual = i.quad = i.logdet = i.lml = std::numeric_limits<double>::quiet_NaN();
  return i;
}

// The context's error text, put back when the scope ends: for work behind a failure whose own failures are not returned (the NaN
// outputs of a fit), so that the message stays the one of the status the call returns.  Work whose failure IS returned needs no
// guard: HIPC, KCHECK and fail() write the text only when they fail.
struct ErrKeep {
  svgp_ctx* ctx;
  std::string text;
  explicit ErrKeep(svgp_ctx* c) : ctx(c), text(c->err) {}
  ErrKeep(const ErrKeep&) = delete;
  ErrKeep& operator=(const ErrKeep&) = delete;
  ~ErrKeep() { ctx->err = text; }
};

// NaN into the rows x cols window at p (data dtype, leading dimension ld), in device memory by one launch or in host memory - the
// outputs of a call that returns SVGP_NOT_POSDEF.  The rows between `rows` and ld are not written.  The context's error text stays
// the caller's status's: only a HIP failure of the fill itself, which is returned, replaces it.
inline int nan_fill(svgp_ctx* ctx, int dtype, void* p, int64_t ld, int64_t rows, int64_t cols, bool on_device) {
  if (on_device) {
    launch_cg_affine(dtype, ctx->stream, p, 0, ld, rows, cols, 0.0, std::numeric_limits<double>::quiet_NaN(), p, ld);
    KCHECK(ctx, "cg (NaN outputs)");
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return SVGP_OK;
  }
  for (int64_t c = 0; c < cols; ++c)
    for (int64_t i = 0; i < rows; ++i) {
      if (dtype == SVGP_F64) static_cast<double*>(p)[c * ld + i] = std::numeric_limits<double>::quiet_NaN();
      else static_cast<float*>(p)[c * ld + i] = std::numeric_limits<float>::quiet_NaN();
    }
  return SVGP_OK;
}

// svgp_last_timing of a call whose data pass lies between the context's events 0 and 1; ms_prep: the preconditioner's setup before it
inline void cg_timing(svgp_ctx* ctx, double ms_prep = 0) {
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_prep = ms_prep;
  ctx->timing.ms_strip = t;
  ctx->timing.ms_total = t + ms_prep;
}

// what every product of a handle under one parameter set shares.  The kernel's rows are the data (kmv, the row-split product), or with
// point_rows the preconditioner's points (pc_expand); px, the panels, n and S are the call's
inline KmvArgs kmv_args(const svgp_cg* cg, const CgPar& p, bool point_rows = false) {
  KmvArgs a{};
  a.rows = point_rows ? cg->pc.rows.p : cg->rows.p;
  a.bias = point_rows ? cg->pc.bias.p : cg->bias.p;
  a.N = point_rows ? cg->pc.k : cg->N;
  a.Np = point_rows ? cg->pc.kp : cg->Np;
  a.invl = cg->invl.p;
  a.family = p.family;
  a.d = cg->d;
  a.variance = p.variance;
  return a;
}

// grow-only reservations in the order written, the first failure returned (DevBuf::reserve; a row of 0 bytes asks for nothing)
struct Reserve {
  DevBuf* buf;
  size_t bytes;
  const char* what;
};
inline int reserve_all(svgp_ctx* ctx, std::initializer_list<Reserve> rows) {
  for (const Reserve& r : rows) {
    const int rc = r.buf->reserve(ctx, r.bytes, r.what);
    if (rc) return rc;
  }
  return SVGP_OK;
}

// One column-major rows x S panel of an entry point in the data dtype: the caller's device memory as it stands, or for a host array
// a dense copy (ld = rows) that lives as long as this object - one call
struct Panel {
  DevBuf buf;           // the copy (host panels only)
  void* p = nullptr;    // what the launches read or write, and its leading dimension
  int64_t ld = 0;
  void* host = nullptr;   // a host panel: the caller's array and its shape, for download
  int64_t host_ld = 0, rows = 0, S = 0;
  size_t es = 8;
};
// upload: an input, copied to the device; otherwise an output, reserved only.  what: the reservation's name in an SVGP_OOM message
inline int stage_panel(svgp_ctx* ctx, Panel& P, const void* ptr, int64_t ld, int64_t rows, int64_t S, size_t es, bool on_device, bool upload,
                       const char* what) {
  P.p = const_cast<void*>(ptr);
  P.ld = ld;
  if (on_device) return SVGP_OK;
  const size_t col = size_t(rows) * es;
  const int rc = P.buf.reserve(ctx, col * size_t(S), what);
  if (rc) return rc;
  P.host = P.p;
  P.host_ld = ld;
  P.rows = rows;
  P.S = S;
  P.es = es;
  P.p = P.buf.p;
  P.ld = rows;
  if (upload) HIPC(ctx, hipMemcpy2DAsync(P.p, col, ptr, size_t(ld) * es, col, size_t(S), hipMemcpyHostToDevice, ctx->stream));
  return SVGP_OK;
}
// a host panel's copy back into the caller's array, its rows x S window only (enqueued: the caller synchronises); device memory: nothing
inline int download_panel(svgp_ctx* ctx, const Panel& P) {
  if (!P.host) return SVGP_OK;
  const size_t col = size_t(P.rows) * P.es;
  HIPC(ctx, hipMemcpy2DAsync(P.host, size_t(P.host_ld) * P.es, P.buf.p, col, col, size_t(P.S), hipMemcpyDeviceToHost, ctx->stream));
  return SVGP_OK;
}

}  // namespace svgp
