// cg_api.hip — the exact GP by matrix-free conjugate gradients: svgp_cg_create / _matvec / _solve / _fit / _lml_grad / _alpha / _predict /
// _free and the host-only svgp_lanczos_logdet (cg.hip: the kernels); svgp_cg_lml_grad_inputs (cg_xgrad.hip: its kernel).  Host orchestration only.
//   Khat = K(x, x) + diag I,  alpha = Khat^-1 delta,  lml = -1/2 (delta' alpha + log det Khat + N log 2 pi)
// Batched CG over column blocks of 64: per iteration one kmv product (the only O(N^2) work), two column dots, two masked axpy passes;
// the per-column scalars and the CG coefficients of every column stay on the device, the host reads the block's 64 activity flags (and
// one failure flag) per iteration.  log det Khat by stochastic Lanczos quadrature from the caller's probe vectors: the Lanczos
// tridiagonal of a column is rebuilt from its CG coefficients, its eigen-decomposition runs in fp64 on the host.
// svgp_cg_set_preconditioner / _precond_cross / _precond_apply / _fit_precond / _lml_grad_precond: the Nystrom preconditioner of the same
// solves (CgPrecond below), set up on the device once per call and applied with two kernel products of N k generated entries.
// svgp_cg_sampler_create / _eval / _eval_grad / _state / _free: pathwise function samples of the exact GP (cg_sample.hip: the kernels) -
// one batched solve of the S right-hand sides delta - Phi(X) w_s - sigma eps_s, then every evaluation is one data-sized pass.
// svgp_cg_set_noise / _lml_grad_noise: per-point noise variances, Khat = K + diag(sigma^2) with sigma_i^2 = T(diag) + s_i - the vector is
// handle state, its minimum is reduced on the device at set time and every call tests it on the host before its data pass; kmv's epilogue
// reads sigma^2 per output point, the preconditioner's D^-1 scalings are streaming passes around its two products.
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

// The Nystrom preconditioner P = Z Kuu^-1 Z' + sigma^2 I, Z = K(X, z_p) for k points z_p, Kuu = K(z_p, z_p) + jitter variance I = Lu Lu':
//   P^-1 r = (r - Z W Z' r) / sigma^2,  W = Lu^-T B^-1 Lu^-1 / sigma^2,  B = I + Lu^-1 (Z'Z) Lu^-T / sigma^2,  log det P = N log sigma^2 + log det B
// Z' r is the row-split product (launch_kmv_split), Z c the existing kmv_kernel with the k points as its rows, whose epilogue adds
// r / sigma^2.  The k-sized stage (Kuu, Lu, the Gram Z'Z, B, its factor, W) is fp64 for both data dtypes: the Gram is accumulated in
// fp64 from fp64 entries (in float32 accumulation B is not positive definite), so an fp32 handle widens x and z_p for the setup.
struct CgPrecond {
  int64_t k = 0, kp = 0, Mp = 0;   // points, padded to 32 (kmv's chunk) and to 128 (the factorisations' tile)
  double jitter = 0;
  svgp_data* z = nullptr;          // the points, data dtype, feature-major
  DevBuf rows, bias;               // kmv_prep of the points under the running parameter set (data dtype)
  DevBuf part, t, v;               // the split product's partials; Z' r and -W Z' r / sigma^2 (kp x S, data dtype)
  DevBuf x64, z64, invl64, rows64, bias64;   // fp32 handles: the fp64 operands of the Gram
  DevBuf zblk;                     // N x 64 fp64: a column block of Z
  DevBuf zs64, Lu, Tu, LinvRM, LinvCM, Ytmp, G, H, H2, Bm, TB, LBinvRM, LBinvCM, W, info, info_b, scal;   // fp64, Mp x Mp
  DevBuf rho, xi;                  // the solver's r'z words; the k x T probes
  bool x64_ready = false, z64_ready = false;   // x of a handle never changes; the points change with set_preconditioner
  double s2 = 0, logdet_p = 0, ms_setup = 0;
};

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
  DevBuf xL, xR, xpart, xout;   // d lml / d x: the N x (2T + 1) panels, the column blocks' partial sums (fp64), a host output's staging
  bool have_fit = false;
  CgPar fit;                 // the parameter set alpha belongs to
  // per-point noise (svgp_cg_set_noise): the snapshot s and its min (NaN-propagating, reduced on the device at set time); per call
  // sig2 = T(diag) + s, 1 / sig2, sqrt(sig2) in the data dtype, 1 / sig2 in fp64 (the Gram's weights); d lml / d sigma_i^2
  bool have_noise = false;
  double noise_min = 0;
  DevBuf noise_s, sig2, isig2, ssig2, isig64, sbar;
  DevBuf noise_lo;           // one fp64 word: the min-reduction's result (kept, so that setting a vector every step allocates nothing)
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
  DevBuf invl, rows, bias;     // the parameter set and the prepared data rows (launch_kmv_prep), data dtype
  DevBuf frows, fbias, W, V;   // omega [d][Lp], tau [Lp], amp W (Lp x S), V (N x S), data dtype
  std::vector<int32_t> iters;  // per column, of the solve
  std::vector<double> relres;
};

namespace {

constexpr int64_t kCgMaxPredict = int64_t(1) << 28;   // n N elements of the predictive variance's right-hand sides in one call

struct CgHist {   // per column: its CG coefficients and |b|^2 (preconditioned: b' P^-1 b, the weight of its quadrature)
  std::vector<std::vector<double>> a, b;
  std::vector<double> bb;
};

struct DataHold {   // test inputs uploaded for one call
  svgp_ctx* ctx;
  svgp_data* D = nullptr;
  ~DataHold() { if (D) svgp_data_free(ctx, D); }
};

// a noise vector is set: the smallest variance T(diag) + min s of the call's descriptor, before any data pass.  SVGP_NOT_POSDEF when it
// is < 0 (<= 0 where the preconditioner divides by it) or NaN
int noise_check(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds, bool precond) {
  if (!cg->have_noise) return SVGP_OK;
  const double lo = cg->dtype == SVGP_F64 ? ds->diag + cg->noise_min : double(float(ds->diag) + float(cg->noise_min));
  if (lo != lo) return fail(ctx, SVGP_NOT_POSDEF, "per-point noise: a variance diag + s_i is NaN");
  if (lo < 0) return fail(ctx, SVGP_NOT_POSDEF, "per-point noise: a variance diag + s_i is negative");
  if (precond && !(lo > 0)) return fail(ctx, SVGP_NOT_POSDEF, "per-point noise: a variance diag + s_i is zero with a preconditioner set (P = Z Kuu^-1 Z' + D)");
  return SVGP_OK;
}

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

void kmv_args(const svgp_cg* cg, const CgPar& p, KmvArgs& a) {
  a = KmvArgs{};
  a.invl = cg->invl.p;
  a.family = p.family;
  a.d = cg->d;
  a.variance = p.variance;
}

// K(z_p, X) V (k x S, ldo) by the row-split kernel, in the data dtype
int pc_cross(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* V, int64_t ldv, int64_t S, void* out, int64_t ldo) {
  CgPrecond& pc = cg->pc;
  int64_t seg_rows = 0;
  const int nseg = kmv_split_segments(cg->N, pc.k, &seg_rows);
  const int rc = pc.part.reserve(ctx, size_t(nseg) * 64 * size_t(pc.k) * cg->es, "the preconditioner's partial products");
  if (rc) return rc;
  KmvArgs a;
  kmv_args(cg, p, a);
  a.rows = cg->rows.p;
  a.bias = cg->bias.p;
  a.px = pc.z->x.p;
  a.ldp = pc.z->ldx;
  a.n = pc.k;
  a.N = cg->N;
  a.Np = cg->Np;
  a.V = V;
  a.ldv = ldv;
  a.S = S;
  a.out = out;
  a.ldo = ldo;
  launch_kmv_split(cg->dtype, ctx->stream, a, pc.part.p);
  return SVGP_OK;
}

// out = K(X, z_p) V + diag addv: kmv_kernel with the k points as its rows (V: kp x S, zero on the padding rows)
void pc_expand(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* V, int64_t S, const void* addv, int64_t lda, double diag, void* out, int64_t ldo,
               const void* dvec = nullptr) {
  const CgPrecond& pc = cg->pc;
  KmvArgs a;
  kmv_args(cg, p, a);
  a.rows = pc.rows.p;
  a.bias = pc.bias.p;
  a.px = cg->data->x.p;
  a.ldp = cg->data->ldx;
  a.n = cg->N;
  a.N = pc.k;
  a.Np = pc.kp;
  a.V = V;
  a.ldv = pc.kp;
  a.S = S;
  a.addv = addv;
  a.dvec = dvec;
  a.lda = lda;
  a.out = out;
  a.ldo = ldo;
  a.diag = diag;
  a.self = 0;   // the points are not the rows, even where they coincide with data points
  launch_kmv(cg->dtype, ctx->stream, a);
}

// out = P^-1 R for S columns on the device (data dtype); out must not alias R
int pc_apply(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* R, int64_t ldr, int64_t S, void* out, int64_t ldo) {
  CgPrecond& pc = cg->pc;
  int rc;
  if ((rc = pc.t.reserve(ctx, size_t(pc.kp) * size_t(S) * cg->es, "the preconditioner's products")) != SVGP_OK) return rc;
  if ((rc = pc.v.reserve(ctx, size_t(pc.kp) * size_t(S) * cg->es, "the preconditioner's products")) != SVGP_OK) return rc;
  if (cg->have_noise) {   // D = diag(sig2): P^-1 r = D^-1 (r - Z W Z' D^-1 r), W = Lu^-T B^-1 Lu^-1; out holds D^-1 r, then r + Z v, then the result
    launch_cg_rowscale(cg->dtype, ctx->stream, R, ldr, cg->isig2.p, cg->N, S, out, ldo);
    if ((rc = pc_cross(ctx, cg, p, out, ldo, S, pc.t.p, pc.kp)) != SVGP_OK) return rc;
    launch_cg_pc_mm(cg->dtype, ctx->stream, pc.W.as<double>(), pc.Mp, pc.k, pc.t.p, 0, pc.kp, S, -1.0, pc.v.p, pc.kp, pc.kp);
    pc_expand(ctx, cg, p, pc.v.p, S, R, ldr, 1.0, out, ldo);
    launch_cg_rowscale(cg->dtype, ctx->stream, out, ldo, cg->isig2.p, cg->N, S, out, ldo);
    return SVGP_OK;
  }
  if ((rc = pc_cross(ctx, cg, p, R, ldr, S, pc.t.p, pc.kp)) != SVGP_OK) return rc;
  launch_cg_pc_mm(cg->dtype, ctx->stream, pc.W.as<double>(), pc.Mp, pc.k, pc.t.p, 0, pc.kp, S, -1.0 / (pc.s2 * pc.s2), pc.v.p, pc.kp, pc.kp);
  pc_expand(ctx, cg, p, pc.v.p, S, R, ldr, 1.0 / pc.s2, out, ldo);
  return SVGP_OK;
}

// the preconditioner of one parameter set: the points' rows, Kuu = Lu Lu', the Gram Z'Z, B and its factor, W, log det P
int pc_setup(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p) {
  CgPrecond& pc = cg->pc;
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype, d = cg->d;
  const int64_t N = cg->N, k = pc.k, kp = pc.kp, Mp = pc.Mp;
  const size_t mm = size_t(Mp) * size_t(Mp) * 8;
  int rc;
  pc.s2 = dt == SVGP_F64 ? p.diag : double(float(p.diag));
  pc.logdet_p = std::numeric_limits<double>::quiet_NaN();
  pc.ms_setup = 0;
  struct { DevBuf* b; size_t bytes; } req[] = {
      {&pc.rows, size_t(d) * size_t(kp) * cg->es}, {&pc.bias, size_t(kp) * cg->es}, {&pc.zblk, size_t(N) * 64 * 8}, {&pc.zs64, size_t(d) * size_t(Mp) * 8},
      {&pc.Lu, mm}, {&pc.Tu, mm}, {&pc.LinvRM, mm}, {&pc.LinvCM, mm}, {&pc.Ytmp, mm}, {&pc.G, mm}, {&pc.H, mm}, {&pc.H2, mm}, {&pc.Bm, mm}, {&pc.TB, mm},
      {&pc.LBinvRM, mm}, {&pc.LBinvCM, mm}, {&pc.W, mm}, {&pc.info, info_bytes(Mp)}, {&pc.info_b, info_bytes(Mp)}, {&pc.scal, 64}, {&pc.rho, 128 * 8},
      {&cg->partial, cg->have_noise ? size_t(64) * size_t(cg_dot_blocks(N)) * 8 : 0}};   // (sum_i log sigma_i^2: ensure_solver's own minimum)
  for (auto& r : req)
    if ((rc = r.b->reserve(ctx, r.bytes, "the preconditioner")) != SVGP_OK) return rc;
  TREC(ctx, ctx->ev[2], s);
  launch_kmv_prep(dt, s, pc.z->x.p, pc.z->ldx, cg->invl.p, d, k, kp, pc.rows.p, pc.bias.p);
  // the fp64 operands of the Gram: the handle's own, or widened
  const double *x64, *z64, *invl64;
  const void *rows64, *bias64;
  int64_t ldx64, ldz64;
  if (dt == SVGP_F64) {
    x64 = cg->data->x.as<double>(); ldx64 = cg->data->ldx;
    z64 = pc.z->x.as<double>(); ldz64 = pc.z->ldx;
    invl64 = cg->invl.as<double>();
    rows64 = cg->rows.p; bias64 = cg->bias.p;
  } else {
    if ((rc = pc.x64.reserve(ctx, size_t(d) * size_t(N) * 8, "the preconditioner")) != SVGP_OK) return rc;
    if ((rc = pc.z64.reserve(ctx, size_t(d) * size_t(k) * 8, "the preconditioner")) != SVGP_OK) return rc;
    if ((rc = pc.invl64.reserve(ctx, size_t(SVGP_MAX_D) * 8, "the preconditioner")) != SVGP_OK) return rc;
    if ((rc = pc.rows64.reserve(ctx, size_t(d) * size_t(cg->Np) * 8, "the preconditioner")) != SVGP_OK) return rc;
    if ((rc = pc.bias64.reserve(ctx, size_t(cg->Np) * 8, "the preconditioner")) != SVGP_OK) return rc;
    launch_cg_widen(dt, s, cg->invl.p, d, d, 1, pc.invl64.as<double>(), d);   // the rounded inverse lengthscales the data stage uses
    if (!pc.x64_ready) launch_cg_widen(dt, s, cg->data->x.p, cg->data->ldx, N, d, pc.x64.as<double>(), N);
    if (!pc.z64_ready) launch_cg_widen(dt, s, pc.z->x.p, pc.z->ldx, k, d, pc.z64.as<double>(), k);
    pc.x64_ready = pc.z64_ready = true;
    launch_kmv_prep(SVGP_F64, s, pc.x64.p, N, pc.invl64.p, d, N, cg->Np, pc.rows64.p, pc.bias64.p);
    x64 = pc.x64.as<double>(); ldx64 = N;
    z64 = pc.z64.as<double>(); ldz64 = k;
    invl64 = pc.invl64.as<double>();
    rows64 = pc.rows64.p; bias64 = pc.bias64.p;
  }
  // launch_potrf's contract: T zero above the diagonal; launch_linv writes the block-lower part only (the rest is read by the products)
  for (DevBuf* b : {&pc.Tu, &pc.TB, &pc.LinvRM, &pc.LinvCM, &pc.LBinvRM, &pc.LBinvCM, &pc.G}) HIPC(ctx, hipMemsetAsync(b->p, 0, mm, s));
  HIPC(ctx, hipMemsetAsync(pc.info.p, 0, info_bytes(Mp), s));
  HIPC(ctx, hipMemsetAsync(pc.info_b.p, 0, info_bytes(Mp), s));
  // Kuu + jitter variance I = Lu Lu' and Lu^-1
  launch_cg_pc_scale(s, z64, ldz64, invl64, d, k, Mp, pc.zs64.as<double>());
  KernelParams kp64;
  kp64.family = p.family;
  kp64.d = d;
  kp64.variance = p.variance;
  kp64.invl = invl64;
  launch_kuu(SVGP_F64, s, kp64, pc.zs64.p, k, Mp, pc.jitter * p.variance, pc.Lu.p);
  launch_potrf(SVGP_F64, s, pc.Lu.p, pc.Tu.p, Mp, pc.info.as<int>(), reinterpret_cast<unsigned*>(pc.info.as<int>() + 1), ctx->num_cus);
  launch_linv(SVGP_F64, s, pc.Lu.p, pc.Tu.p, Mp, pc.LinvRM.p, pc.LinvCM.p, pc.Ytmp.p);
  KCHECK(ctx, "cg preconditioner (Kuu, its factor)");
  // G = Z'Z, a column block of Z at a time: the block explicitly (N x <= 64), then the row-split product with it as the panel
  {
    int64_t seg_rows = 0;
    const int nseg = kmv_split_segments(N, k, &seg_rows);
    if ((rc = pc.part.reserve(ctx, size_t(nseg) * 64 * size_t(k) * 8, "the preconditioner's partial products")) != SVGP_OK) return rc;
    KmvArgs a{};
    a.rows = rows64;
    a.bias = bias64;
    a.invl = invl64;
    a.px = z64;
    a.ldp = ldz64;
    a.n = k;
    a.N = N;
    a.Np = cg->Np;
    a.V = pc.zblk.p;
    a.ldv = N;
    a.ldo = Mp;
    a.family = p.family;
    a.d = d;
    a.variance = p.variance;
    for (int64_t j0 = 0; j0 < k; j0 += 64) {
      const int64_t nb = k - j0 < 64 ? k - j0 : 64;
      launch_cg_kcols(SVGP_F64, s, x64, ldx64, N, z64 + j0, ldz64, nb, invl64, d, p.family, p.variance, pc.zblk.p, N);
      if (cg->have_noise) launch_cg_rowscale(2, s, pc.zblk.p, N, cg->isig64.p, N, nb, pc.zblk.p, N);   // Z' D^-1 Z: the weights on the explicit block
      a.S = nb;
      a.out = pc.G.as<double>() + j0 * Mp;
      launch_kmv_split(SVGP_F64, s, a, pc.part.p);
    }
    KCHECK(ctx, "cg preconditioner (Gram)");
  }
  // B = I + Lu^-1 G Lu^-T / sigma^2 = LB LB'  (launch_gemm_pm: out = X'Y for row-major X, Y; LinvCM read row-major is Lu^-T)
  launch_gemm_pm(SVGP_F64, s, pc.G.p, pc.LinvCM.p, nullptr, 1.0, Mp, Mp, Mp, 1, pc.H.p, 1, kMmFull);     // G Lu^-T
  launch_gemm_pm(SVGP_F64, s, pc.H.p, pc.LinvCM.p, nullptr, 1.0, Mp, Mp, Mp, 1, pc.H2.p, 1, kMmFull);    // Lu^-1 G Lu^-T
  launch_cg_pc_form_b(s, pc.H2.as<double>(), Mp, cg->have_noise ? 1.0 : pc.s2, pc.Bm.as<double>());   // (the Gram carries D^-1 already)
  launch_potrf(SVGP_F64, s, pc.Bm.p, pc.TB.p, Mp, pc.info_b.as<int>(), reinterpret_cast<unsigned*>(pc.info_b.as<int>() + 1), ctx->num_cus);
  launch_cg_pc_logdet(s, pc.Bm.as<double>(), Mp, k, pc.scal.as<double>());
  if (cg->have_noise) {   // sum_i log sigma_i^2: the fixed two-stage reduction
    launch_cg_noise_sum(dt, s, cg->sig2.p, nullptr, N, cg->partial.as<double>());
    launch_cg_colsum(s, cg->partial.as<double>(), N, 1, pc.scal.as<double>() + 1);
  }
  // W sigma^2 = Lu^-T B^-1 Lu^-1, B^-1 = LB^-T LB^-1
  launch_linv(SVGP_F64, s, pc.Bm.p, pc.TB.p, Mp, pc.LBinvRM.p, pc.LBinvCM.p, pc.Ytmp.p);
  launch_gemm_pm(SVGP_F64, s, pc.LBinvRM.p, pc.LBinvRM.p, nullptr, 1.0, Mp, Mp, Mp, 1, pc.H.p, 1, kMmFull);   // B^-1
  launch_gemm_pm(SVGP_F64, s, pc.H.p, pc.LinvRM.p, nullptr, 1.0, Mp, Mp, Mp, 1, pc.H2.p, 1, kMmFull);         // B^-1 Lu^-1
  launch_gemm_pm(SVGP_F64, s, pc.LinvRM.p, pc.H2.p, nullptr, 1.0, Mp, Mp, Mp, 1, pc.W.p, 1, kMmFull);         // Lu^-T B^-1 Lu^-1
  KCHECK(ctx, "cg preconditioner (B, W)");
  TREC(ctx, ctx->ev[3], s);
  int iu = 0, ib = 0;
  double ld = 0, ldd = 0;
  if (cg->have_noise) HIPC(ctx, hipMemcpyAsync(&ldd, pc.scal.as<double>() + 1, 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(&iu, pc.info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(&ib, pc.info_b.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(&ld, pc.scal.p, 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  float t = 0;
  if (elapsed_ms(ctx, &t, ctx->ev[2], ctx->ev[3]) == hipSuccess) pc.ms_setup = t;
  if (iu != 0 || ib != 0 || !(ld == ld)) {
    char buf[200];
    snprintf(buf, sizeof buf, "the preconditioner's %s is not positive definite: leading minor of order %d", iu ? "Kuu + jitter" : "B",
             iu ? iu : ib);
    return fail(ctx, SVGP_NOT_POSDEF, buf);
  }
  pc.logdet_p = (cg->have_noise ? ldd : double(N) * std::log(pc.s2)) + ld;
  return SVGP_OK;
}

// the parameter set on the device: invl in the data dtype, the scaled padded rows and their bias (once per call); precond: the
// preconditioner's setup as well, when one is set
int set_params(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, bool precond = true) {
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
  if (cg->have_noise) {
    const size_t nb = size_t(cg->N) * cg->es;
    if ((rc = cg->sig2.reserve(ctx, nb, "the noise variances")) != SVGP_OK) return rc;
    if ((rc = cg->isig2.reserve(ctx, nb, "the noise variances")) != SVGP_OK) return rc;
    if ((rc = cg->ssig2.reserve(ctx, nb, "the noise variances")) != SVGP_OK) return rc;
    if ((rc = cg->isig64.reserve(ctx, size_t(cg->N) * 8, "the noise variances")) != SVGP_OK) return rc;
    launch_cg_noise_prep(cg->dtype, s, cg->noise_s.p, cg->N, p.diag, cg->sig2.p, cg->isig2.p, cg->ssig2.p, cg->isig64.as<double>());
    KCHECK(ctx, "cg (noise variances)");
  }
  if (precond && cg->pc.k > 0) return pc_setup(ctx, cg, p);
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
  a.dvec = (addv && cg->have_noise) ? cg->sig2.p : nullptr;   // Khat = K + diag(sig2); addv is only ever passed with the data as the points
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
  if ((rc = cg->ws.reserve(ctx, size_t(cg->pc.k > 0 ? 6 : 5) * size_t(cg->N) * 64 * cg->es, "the CG workspace")) != SVGP_OK) return rc;   // (z = P^-1 r)
  if ((rc = cg->st.reserve(ctx, size_t(CgState::WORDS) * 8, "the CG state")) != SVGP_OK) return rc;
  const int64_t cols = dot_cols < 64 ? 64 : dot_cols;
  if ((rc = cg->partial.reserve(ctx, size_t(cols) * size_t(cg_dot_blocks(cg->N)) * 8, "the CG dot partials")) != SVGP_OK) return rc;
  if (want_hist && (rc = cg->hist.reserve(ctx, size_t(2) * size_t(maxiter) * 64 * 8, "the CG coefficient history")) != SVGP_OK) return rc;
  return SVGP_OK;
}

// X = Khat^-1 B for S columns on the device (data dtype), in blocks of 64.  iters_out / relres_out: per column, host, nullable.
// SVGP_NOT_POSDEF: every column of X is NaN.  The caller has run ensure_solver and set_params.  With a preconditioner set (pc.k > 0)
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

// a host matrix (data dtype, column-major, ld) into a dense N x S device buffer and back
int upload_cols(svgp_ctx* ctx, const svgp_cg* cg, DevBuf& b, const void* host, int64_t ld, int64_t S, const char* what) {
  const size_t col = size_t(cg->N) * cg->es;
  const int rc = b.reserve(ctx, col * size_t(S), what);
  if (rc) return rc;
  if (host) HIPC(ctx, hipMemcpy2DAsync(b.p, col, host, size_t(ld) * cg->es, col, size_t(S), hipMemcpyHostToDevice, ctx->stream));
  return SVGP_OK;
}

int check_precond_desc(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds) {
  if (cg->have_noise) return SVGP_OK;   // the variances are diag + s_i: noise_check answers for them (SVGP_NOT_POSDEF)
  if (!(ds->diag > 0)) return fail(ctx, SVGP_INVALID_ARG, "a preconditioner is set: diag must be > 0 (P = Z Kuu^-1 Z' + diag I)");
  return SVGP_OK;
}

int common_checks(svgp_ctx* ctx, const svgp_cg* cg, const svgp_cg_desc* ds) {
  if (cg->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the CG handle lives on another device than the context");
  return check_desc(ctx, cg, ds);
}

// svgp_cg_fit and svgp_cg_lml_grad: g non-null asks for the gradient {d_variance, d_inv_lengthscale[d], d_diag, d_mean_const}
struct FitGrad { double *dv, *dil, *dd, *dm; };

// NaN into every entry of the input gradient's output (T = 0, SVGP_NOT_POSDEF); the context's message is the caller's to keep
int xgrad_fill_nan(svgp_ctx* ctx, const svgp_cg* cg, const svgp_input_grad* gx) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (gx->on_device) {
    launch_cg_affine(cg->dtype, ctx->stream, gx->x, 0, gx->ld, cg->N, cg->d, 0.0, nan, gx->x, gx->ld);
    KCHECK(ctx, "cg (NaN outputs)");
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return SVGP_OK;
  }
  for (int f = 0; f < cg->d; ++f)
    for (int64_t i = 0; i < cg->N; ++i) {
      if (cg->dtype == SVGP_F64) static_cast<double*>(gx->x)[int64_t(f) * gx->ld + i] = nan;
      else static_cast<float*>(gx->x)[int64_t(f) * gx->ld + i] = std::numeric_limits<float>::quiet_NaN();
    }
  return SVGP_OK;
}

// NaN into the noise gradient's output (SVGP_NOT_POSDEF)
int sbar_fill_nan(svgp_ctx* ctx, const svgp_cg* cg, const svgp_point_noise_grad* gpn) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (gpn->on_device) {
    launch_cg_affine(cg->dtype, ctx->stream, gpn->s_bar, 0, cg->N, cg->N, 1, 0.0, nan, gpn->s_bar, cg->N);
    KCHECK(ctx, "cg (NaN outputs)");
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return SVGP_OK;
  }
  for (int64_t i = 0; i < cg->N; ++i) {
    if (cg->dtype == SVGP_F64) static_cast<double*>(gpn->s_bar)[i] = nan;
    else static_cast<float*>(gpn->s_bar)[i] = std::numeric_limits<float>::quiet_NaN();
  }
  return SVGP_OK;
}

// d lml / d x after the gradient block of fit_impl: U = fitX = [alpha, w_t], P = fitB = [alpha, p_t] on the device.
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
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_strip = t;   // the data-sized kernels of the input gradient alone
  ctx->timing.ms_total = t;
  return SVGP_OK;
}
// with a preconditioner: probes_k (k x T) joins the probes, z_t = sigma eps_t + Z Lu^-T xi_t (E z z' = P), log det Khat = log det P +
// (1 / T) sum_t (z_t' P^-1 z_t) e_1' log(T_t) e_1, and the gradient's trace terms are w_t' dKhat (P^-1 z_t)
int fit_impl(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* ds, const double* delta, int32_t T, const double* probes, double* lml_out,
             svgp_cg_info* info, const FitGrad* g, const double* probes_k = nullptr, bool precond_call = false,
             const svgp_input_grad* gx = nullptr, const svgp_point_noise_grad* gpn = nullptr) {
  int rc = common_checks(ctx, cg, ds);
  if (rc) return rc;
  const bool pc = cg->pc.k > 0;
  if (precond_call && !pc) return fail(ctx, SVGP_INVALID_ARG, "no preconditioner is set on this handle (svgp_cg_set_preconditioner)");
  if (pc && (rc = check_precond_desc(ctx, cg, ds)) != SVGP_OK) return rc;
  if (pc && T > 0 && !precond_call)
    return fail(ctx, SVGP_INVALID_ARG, "a preconditioner is set: the probes need their k x T part (svgp_cg_fit_precond / svgp_cg_lml_grad_precond)");
  if (pc && T > 0 && !probes_k) return fail(ctx, SVGP_INVALID_ARG, "null probes_k with T > 0");
  if (!delta && !cg->data->y.p) return fail(ctx, SVGP_INVALID_ARG, "the data handle has no y and no delta was given");
  if (T < 0) return fail(ctx, SVGP_INVALID_ARG, "the number of probes must be >= 0");
  if (T > 0 && !probes) return fail(ctx, SVGP_INVALID_ARG, "null probes with T > 0");
  if (g && (!g->dv || !g->dil)) return fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  if (gx && (rc = check_input_grad(ctx, cg->data, cg->N, gx)) != SVGP_OK) return rc;
  if (gpn && !gpn->s_bar) return fail(ctx, SVGP_INVALID_ARG, "null noise-gradient output");
  if (gpn && gpn->on_device != 0 && gpn->on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  if (gpn && gpn->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved must be 0");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype, d = cg->d;
  const bool want_sbar = g && (gpn || cg->have_noise);   // with a vector set d_variance needs sum_i sigma_i^2 s_bar_i
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
  if (want_sbar && (rc = cg->sbar.reserve(ctx, col, "the noise gradient")) != SVGP_OK) return rc;
  if (gx && T > 0) {
    const size_t S2 = 2 * size_t(T) + 1;
    if ((rc = cg->xL.reserve(ctx, col * S2, "the input gradient's panels")) != SVGP_OK) return rc;
    if ((rc = cg->xR.reserve(ctx, col * S2, "the input gradient's panels")) != SVGP_OK) return rc;
    if ((rc = cg->xpart.reserve(ctx, ((S2 + 15) / 16) * size_t(d) * size_t(N) * 8, "the input gradient's partial sums")) != SVGP_OK) return rc;
    if (!gx->on_device && (rc = cg->xout.reserve(ctx, col * size_t(d), "the input gradient")) != SVGP_OK) return rc;
  }
  // SVGP_NOT_POSDEF: NaN in the input gradient as well, the status and its message kept
  auto nan_inputs = [&](int status) {
    if ((gx || gpn) && status == SVGP_NOT_POSDEF) {
      const std::string keep = ctx->err;
      if (gx) (void)xgrad_fill_nan(ctx, cg, gx);
      if (gpn) (void)sbar_fill_nan(ctx, cg, gpn);
      ctx->err = keep;
    }
    return status;
  };
  if ((rc = noise_check(ctx, cg, ds, pc)) == SVGP_OK) rc = set_params(ctx, cg, par);
  if (rc != SVGP_OK) {
    if (rc == SVGP_NOT_POSDEF) {
      svgp_cg_info bad{};
      bad.max_rel_residual = bad.quad = bad.logdet = bad.lml = std::numeric_limits<double>::quiet_NaN();
      if (info) *info = bad;
      if (lml_out) *lml_out = bad.lml;
    }
    return nan_inputs(rc);
  }
  // [delta, z_1 .. z_T], each entry rounded once to the data dtype
  if (delta) {
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, delta, size_t(N) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, 1, 1.0, 0.0, cg->fitB.p, N);
  } else {
    launch_cg_affine(dt, s, cg->data->y.p, 0, N, N, 1, 1.0, -par.mean_const, cg->fitB.p, N);
  }
  if (T > 0 && !pc) {
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, probes, size_t(N) * size_t(T) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, T, 1.0, 0.0, cg->fitB.as<char>() + col, N);
  }
  if (T > 0 && pc) {   // z_t = sigma eps_t + Z (Lu^-T xi_t): eps rounded into fitX (the solve overwrites it), Lu^-T xi into pc.v
    CgPrecond& P = cg->pc;
    if ((rc = P.xi.reserve(ctx, size_t(P.k) * size_t(T) * 8, "the probes")) != SVGP_OK) return rc;
    if ((rc = P.v.reserve(ctx, size_t(P.kp) * size_t(T) * cg->es, "the preconditioner's products")) != SVGP_OK) return rc;
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, probes, size_t(N) * size_t(T) * 8, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(P.xi.p, probes_k, size_t(P.k) * size_t(T) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, T, 1.0, 0.0, cg->fitX.as<char>() + col, N);
    launch_cg_pc_mm(dt, s, P.LinvRM.as<double>(), P.Mp, P.k, P.xi.p, 1, P.k, T, 1.0, P.v.p, P.kp, P.kp);
    pc_expand(ctx, cg, par, P.v.p, T, cg->fitX.as<char>() + col, N, std::sqrt(P.s2), cg->fitB.as<char>() + col, N,
              cg->have_noise ? cg->ssig2.p : nullptr);   // per-point noise: z_t = D^1/2 eps_t + Z Lu^-T xi_t
  }
  KCHECK(ctx, "cg (right-hand sides)");
  CgHist hist;
  svgp_cg_info out{};
  rc = solve_core(ctx, cg, par, S, cg->fitB.p, N, cg->fitX.p, N, nullptr, nullptr, &out, &hist);
  if (rc) {
    if (info) *info = out;
    if (lml_out) *lml_out = out.lml;
    return nan_inputs(rc);
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
    if (pc) logdet += cg->pc.logdet_p;
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
    if (pc && T > 0) {   // the panel's probe columns become P^-1 z_t
      if ((rc = pc_apply(ctx, cg, par, cg->fitB.as<char>() + col, N, T, static_cast<char*>(O) + col, N)) != SVGP_OK) return rc;
      HIPC(ctx, hipMemcpyAsync(cg->fitB.as<char>() + col, static_cast<char*>(O) + col, col * size_t(T), hipMemcpyDeviceToDevice, s));
    }
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
    if (want_sbar) {   // s_bar from the panels, and sum_i sigma_i^2 s_bar_i behind the other results
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
      return 0.5 * first - (T > 0 ? tr / (2.0 * double(T)) : nan);
    };
    const double dd = combine(h.data(), nullptr, 0.0);
    if (g->dd) *g->dd = dd;
    if (!cg->have_noise) *g->dv = combine(h.data() + S, h.data(), par.diag) / par.variance;   // K v = Khat v - diag v
    else *g->dv = (combine(h.data() + S, nullptr, 0.0) - h[size_t(d + 2) * size_t(S) + 1]) / par.variance;   // K v = Khat v - D v
    for (int f = 0; f < d; ++f) g->dil[f] = combine(h.data() + size_t(2 + f) * size_t(S), nullptr, 0.0) / par.invl[f];
    if (g->dm) *g->dm = h[size_t(d + 2) * size_t(S)];
    if (gpn) {
      HIPC(ctx, hipMemcpyAsync(gpn->s_bar, cg->sbar.p, col, gpn->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
      HIPC(ctx, hipStreamSynchronize(s));
    }
    if (gx && (rc = T > 0 ? xgrad_enqueue(ctx, cg, par, T, gx) : xgrad_fill_nan(ctx, cg, gx)) != SVGP_OK) return rc;
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
  const void* vp = on_device ? V : Vd.p;
  void* op = on_device ? out : Od.p;
  const int64_t lv = on_device ? ldv : N, lo = on_device ? ldo : N;
  if ((rc = noise_check(ctx, cg, desc, false)) != SVGP_OK) {   // a bad variance: NaN outputs, the status and its message kept
    const std::string keep = ctx->err;
    launch_cg_affine(cg->dtype, s, op, 0, lo, N, S, 0.0, std::numeric_limits<double>::quiet_NaN(), op, lo);
    KCHECK(ctx, "cg (NaN outputs)");
    if (!on_device) HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * cg->es, Od.p, col, col, size_t(S), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    ctx->err = keep;
    return rc;
  }
  if ((rc = set_params(ctx, cg, par, false)) != SVGP_OK) return rc;
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
  if (cg->pc.k > 0 && (rc = check_precond_desc(ctx, cg, desc)) != SVGP_OK) return rc;
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
  if ((rc = noise_check(ctx, cg, desc, cg->pc.k > 0)) == SVGP_OK) rc = set_params(ctx, cg, par);
  if (rc == SVGP_NOT_POSDEF) {   // the preconditioner did not factor, or a bad noise variance: NaN outputs, as for a bad curvature
    const std::string keep = ctx->err;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    void* Xp = on_device ? X : Xd.p;
    launch_cg_affine(cg->dtype, s, Xp, 0, on_device ? ldx : N, N, S, 0.0, nan, Xp, on_device ? ldx : N);
    KCHECK(ctx, "cg (NaN outputs)");
    if (!on_device) HIPC(ctx, hipMemcpy2DAsync(X, size_t(ldx) * cg->es, Xd.p, col, col, size_t(S), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    for (int64_t j = 0; j < S; ++j) {
      if (iters_out) iters_out[j] = 0;
      if (relres_out) relres_out[j] = nan;
    }
    if (info) {
      *info = svgp_cg_info{};
      info->max_rel_residual = info->quad = info->logdet = info->lml = nan;
    }
    ctx->err = keep;
    return rc;
  }
  if (rc) return rc;
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
  if ((rc = mv.reserve(ctx, size_t(n) * es, "the predictions")) != SVGP_OK) return rc;
  if (var_out) {
    if ((rc = Bk.reserve(ctx, col * size_t(n), "k(X, x*)")) != SVGP_OK) return rc;
    if ((rc = Xk.reserve(ctx, col * size_t(n), "Khat^-1 k(X, x*)")) != SVGP_OK) return rc;
    if ((rc = vres.reserve(ctx, size_t(n) * 8, "the predictive variances")) != SVGP_OK) return rc;
    if ((rc = ensure_solver(ctx, cg, n, false, par.maxiter)) != SVGP_OK) return rc;
  }
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

int32_t svgp_cg_set_preconditioner(svgp_ctx* ctx, svgp_cg* cg, int32_t layout, int64_t k, const void* z_host, double jitter) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (cg->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the CG handle lives on another device than the context");
  if (k < 0 || k > 2048) return fail(ctx, SVGP_INVALID_ARG, "the number of preconditioner points must be in [0, 2048]");
  if (k > 0 && !z_host) return fail(ctx, SVGP_INVALID_ARG, "null preconditioner points");
  if (k > 0 && layout != SVGP_COLVECS && layout != SVGP_ROWVECS && layout != SVGP_VEC) return fail(ctx, SVGP_INVALID_ARG, "bad layout");
  if (k > 0 && layout == SVGP_VEC && cg->d != 1) return fail(ctx, SVGP_INVALID_ARG, "bad layout: a plain vector needs d = 1");
  if (!(jitter >= 0)) return fail(ctx, SVGP_INVALID_ARG, "jitter must be >= 0");
  HIPC(ctx, hipSetDevice(ctx->device));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  svgp_data* z = nullptr;
  if (k > 0) {
    const int rc = svgp_data_upload(ctx, cg->dtype, layout, cg->d, k, z_host, nullptr, &z);
    if (rc) return rc;
  }
  delete cg->pc.z;
  cg->pc.z = z;
  cg->pc.k = k;
  cg->pc.kp = (k + 31) / 32 * 32;
  cg->pc.Mp = (k + 127) / 128 * 128;
  cg->pc.jitter = jitter;
  cg->pc.ms_setup = 0;
  cg->pc.z64_ready = false;
  return SVGP_OK;
}

int32_t svgp_cg_precond_cross(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* V, int64_t ldv, void* out, int64_t ldo,
                              int32_t on_device) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg || !V || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  int rc = common_checks(ctx, cg, desc);
  if (rc) return rc;
  if (cg->pc.k < 1) return fail(ctx, SVGP_INVALID_ARG, "no preconditioner is set on this handle (svgp_cg_set_preconditioner)");
  if (S < 1) return fail(ctx, SVGP_INVALID_ARG, "S must be >= 1");
  if (ldv < cg->N || ldo < cg->pc.k) return fail(ctx, SVGP_INVALID_ARG, "ldv must be >= N and ldo >= k");
  if (on_device != 0 && on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t k = cg->pc.k;
  const size_t kcol = size_t(k) * cg->es;
  const CgPar par = par_of(desc);
  DevBuf Vd, Od;
  if (!on_device) {
    if ((rc = upload_cols(ctx, cg, Vd, V, ldv, S, "the panel")) != SVGP_OK) return rc;
    if ((rc = Od.reserve(ctx, kcol * size_t(S), "the product")) != SVGP_OK) return rc;
  }
  if ((rc = set_params(ctx, cg, par, false)) != SVGP_OK) return rc;
  if ((rc = pc_cross(ctx, cg, par, on_device ? V : Vd.p, on_device ? ldv : cg->N, S, on_device ? out : Od.p, on_device ? ldo : k)) != SVGP_OK) return rc;
  KCHECK(ctx, "kmv (row-split)");
  if (!on_device) HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * cg->es, Od.p, kcol, kcol, size_t(S), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

int32_t svgp_cg_precond_apply(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* R, int64_t ldr, void* out, int64_t ldo,
                              int32_t on_device, double* logdet_p_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg || !R || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  int rc = common_checks(ctx, cg, desc);
  if (rc) return rc;
  if (cg->pc.k < 1) return fail(ctx, SVGP_INVALID_ARG, "no preconditioner is set on this handle (svgp_cg_set_preconditioner)");
  if ((rc = check_precond_desc(ctx, cg, desc)) != SVGP_OK) return rc;
  if (S < 1) return fail(ctx, SVGP_INVALID_ARG, "S must be >= 1");
  if (ldr < cg->N || ldo < cg->N) return fail(ctx, SVGP_INVALID_ARG, "ldr and ldo must be >= N");
  if (on_device != 0 && on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  if (on_device && R == out) return fail(ctx, SVGP_INVALID_ARG, "out must not be R");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = cg->N;
  const size_t col = size_t(N) * cg->es;
  const CgPar par = par_of(desc);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (logdet_p_out) *logdet_p_out = nan;
  DevBuf Rd, Od;
  if (!on_device) {
    if ((rc = upload_cols(ctx, cg, Rd, R, ldr, S, "the panel")) != SVGP_OK) return rc;
    if ((rc = upload_cols(ctx, cg, Od, nullptr, N, S, "the product")) != SVGP_OK) return rc;
  }
  void* op = on_device ? out : Od.p;
  const int64_t lo = on_device ? ldo : N;
  if ((rc = noise_check(ctx, cg, desc, true)) == SVGP_OK) rc = set_params(ctx, cg, par);
  if (rc != SVGP_OK && rc != SVGP_NOT_POSDEF) return rc;
  const int status = rc;
  const std::string keep = ctx->err;
  if (status == SVGP_OK) {
    TREC(ctx, ctx->ev[0], s);
    if ((rc = pc_apply(ctx, cg, par, on_device ? R : Rd.p, on_device ? ldr : N, S, op, lo)) != SVGP_OK) return rc;
    TREC(ctx, ctx->ev[1], s);
    KCHECK(ctx, "cg preconditioner (apply)");
  } else {
    launch_cg_affine(cg->dtype, s, op, 0, lo, N, S, 0.0, nan, op, lo);
    KCHECK(ctx, "cg (NaN outputs)");
  }
  if (!on_device) HIPC(ctx, hipMemcpy2DAsync(out, size_t(ldo) * cg->es, Od.p, col, col, size_t(S), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  if (status == SVGP_OK) {
    float t = 0;
    (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
    ctx->timing = svgp_timing{};
    ctx->timing.ms_prep = cg->pc.ms_setup;
    ctx->timing.ms_strip = t;
    ctx->timing.ms_total = t + cg->pc.ms_setup;
    cg->pc.ms_setup = 0;
    if (logdet_p_out) *logdet_p_out = cg->pc.logdet_p;
  }
  ctx->err = keep;
  return status;
}

int32_t svgp_cg_fit_precond(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                            const double* probes_k, double* lml_out, svgp_cg_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  return fit_impl(ctx, cg, desc, delta, T, probes, lml_out, info, nullptr, probes_k, true);
}

int32_t svgp_cg_lml_grad_precond(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                                 const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                                 double* d_diag, double* d_mean_const) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  const FitGrad g{d_variance, d_inv_lengthscale, d_diag, d_mean_const};
  return fit_impl(ctx, cg, desc, delta, T, probes, lml_out, info, &g, probes_k, true);
}

int32_t svgp_cg_lml_grad_inputs(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                                const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                                double* d_diag, double* d_mean_const, const svgp_input_grad* gx) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!gx || !gx->x) return fail(ctx, SVGP_INVALID_ARG, "null input-gradient output");
  const bool pc = cg->pc.k > 0;
  if (!pc && probes_k) return fail(ctx, SVGP_INVALID_ARG, "probes_k without a preconditioner on this handle (svgp_cg_set_preconditioner)");
  const FitGrad g{d_variance, d_inv_lengthscale, d_diag, d_mean_const};
  return fit_impl(ctx, cg, desc, delta, T, probes, lml_out, info, &g, probes_k, pc, gx);
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

int32_t svgp_cg_lml_grad_noise(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                               const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                               double* d_diag, double* d_mean_const, const svgp_input_grad* gx, svgp_point_noise_grad* gpn) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!cg) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (gx && !gx->x) return fail(ctx, SVGP_INVALID_ARG, "null input-gradient output");
  if (!gpn || !gpn->s_bar) return fail(ctx, SVGP_INVALID_ARG, "null noise-gradient output");
  const bool pc = cg->pc.k > 0;
  if (!pc && probes_k) return fail(ctx, SVGP_INVALID_ARG, "probes_k without a preconditioner on this handle (svgp_cg_set_preconditioner)");
  const FitGrad g{d_variance, d_inv_lengthscale, d_diag, d_mean_const};
  return fit_impl(ctx, cg, desc, delta, T, probes, lml_out, info, &g, probes_k, pc, gx, gpn);
}

}  // extern "C"

// ---- pathwise function samples ---------------------------------------------------------------------------------------------------

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

void cgs_timing(svgp_ctx* ctx) {
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_strip = t;
  ctx->timing.ms_total = t;
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
  struct { DevBuf* b; size_t bytes; } req[] = {
      {&sp->invl, size_t(SVGP_MAX_D) * 8}, {&sp->rows, size_t(d) * size_t(cg->Np) * es}, {&sp->bias, size_t(cg->Np) * es},
      {&sp->frows, size_t(d) * size_t(Lp) * es}, {&sp->fbias, size_t(Lp) * es}, {&sp->W, size_t(Lp) * size_t(S) * es}, {&sp->V, col * size_t(S)},
      {&d_omega, size_t(L) * size_t(d) * es}, {&d_tau, size_t(L) * es}, {&d_w, size_t(S) * size_t(L) * es}, {&d_eps, col * size_t(S)},
      {&dvec, col}, {&phi, L > 0 ? col * size_t(S) : 0}, {&B, col * size_t(S)}, {&cg->f64tmp, size_t(N) * 8}, {&cg->res, size_t(S) * 8}};
  for (auto& r : req)
    if (r.bytes > 0 && (rc = r.b->reserve(ctx, r.bytes, "the sampler")) != SVGP_OK) return rc;
  if ((rc = ensure_solver(ctx, cg, S, false, par.maxiter)) != SVGP_OK) return rc;
  if ((rc = noise_check(ctx, cg, desc, cg->pc.k > 0)) == SVGP_OK) rc = set_params(ctx, cg, par);
  if (rc != SVGP_OK) {   // SVGP_NOT_POSDEF: the preconditioner did not factor, or a bad noise variance - no sampler
    if (rc == SVGP_NOT_POSDEF && info) {
      *info = svgp_cg_info{};
      info->max_rel_residual = info->quad = info->logdet = info->lml = nan;
    }
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
  // delta, rounded once as svgp_cg_fit rounds it
  if (delta) {
    HIPC(ctx, hipMemcpyAsync(cg->f64tmp.p, delta, size_t(N) * 8, hipMemcpyHostToDevice, s));
    launch_cg_affine(dt, s, cg->f64tmp.p, 1, N, N, 1, 1.0, 0.0, dvec.p, N);
  } else {
    launch_cg_affine(dt, s, cg->data->y.p, 0, N, N, 1, 1.0, -par.mean_const, dvec.p, N);
  }
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
    oi.n_unconverged = int32_t(S < 2147483647 ? S : 2147483647);
    oi.max_rel_residual = oi.quad = oi.logdet = oi.lml = nan;
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
  cgs_timing(ctx);
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
  cgs_timing(ctx);
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
