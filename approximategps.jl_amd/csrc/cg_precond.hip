// cg_precond.hip — the Nystrom preconditioner of the exact GP's conjugate gradients (CgPrecond, cg_host.hpp): svgp_cg_set_preconditioner /
// _precond_cross / _precond_apply.  Set up on the device once per call (pc_setup, from set_params) and applied with two kernel
// products of N k generated entries (pc_apply, from the solver).  Host orchestration only; cg.hip holds the kernels.
#include <cstdio>

#include "cg_host.hpp"

using namespace svgp;

namespace {

// K(z_p, X) V (k x S, ldo) by the row-split kernel, in the data dtype
int pc_cross(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* V, int64_t ldv, int64_t S, void* out, int64_t ldo) {
  CgPrecond& pc = cg->pc;
  int64_t seg_rows = 0;
  const int nseg = kmv_split_segments(cg->N, pc.k, &seg_rows);
  const int rc = pc.part.reserve(ctx, size_t(nseg) * 64 * size_t(pc.k) * cg->es, "the preconditioner's partial products");
  if (rc) return rc;
  KmvArgs a = kmv_args(cg, p);
  a.px = pc.z->x.p;
  a.ldp = pc.z->ldx;
  a.n = pc.k;
  a.V = V;
  a.ldv = ldv;
  a.S = S;
  a.out = out;
  a.ldo = ldo;
  launch_kmv_split(cg->dtype, ctx->stream, a, pc.part.p);
  return SVGP_OK;
}

}  // namespace

namespace svgp {

void pc_expand(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* V, int64_t S, const void* addv, int64_t lda, double diag, void* out, int64_t ldo,
               const void* dvec) {
  KmvArgs a = kmv_args(cg, p, true);
  a.px = cg->data->x.p;
  a.ldp = cg->data->ldx;
  a.n = cg->N;
  a.V = V;
  a.ldv = cg->pc.kp;
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

int pc_apply(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p, const void* R, int64_t ldr, int64_t S, void* out, int64_t ldo) {
  CgPrecond& pc = cg->pc;
  const size_t kS = size_t(pc.kp) * size_t(S) * cg->es;
  int rc = reserve_all(ctx, {{&pc.t, kS, "the preconditioner's products"}, {&pc.v, kS, "the preconditioner's products"}});
  if (rc) return rc;
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

int pc_setup(svgp_ctx* ctx, svgp_cg* cg, const CgPar& p) {
  CgPrecond& pc = cg->pc;
  hipStream_t s = ctx->stream;
  const int dt = cg->dtype, d = cg->d;
  const int64_t N = cg->N, k = pc.k, kp = pc.kp, Mp = pc.Mp;
  const size_t mm = size_t(Mp) * size_t(Mp) * 8;
  const char* what = "the preconditioner";
  pc.s2 = dt == SVGP_F64 ? p.diag : double(float(p.diag));
  pc.logdet_p = std::numeric_limits<double>::quiet_NaN();
  pc.ms_setup = 0;
  int rc = reserve_all(ctx, {
      {&pc.rows, size_t(d) * size_t(kp) * cg->es, what}, {&pc.bias, size_t(kp) * cg->es, what}, {&pc.zblk, size_t(N) * 64 * 8, what},
      {&pc.zs64, size_t(d) * size_t(Mp) * 8, what}, {&pc.Lu, mm, what}, {&pc.Tu, mm, what}, {&pc.LinvRM, mm, what}, {&pc.LinvCM, mm, what},
      {&pc.Ytmp, mm, what}, {&pc.G, mm, what}, {&pc.H, mm, what}, {&pc.H2, mm, what}, {&pc.Bm, mm, what}, {&pc.TB, mm, what},
      {&pc.LBinvRM, mm, what}, {&pc.LBinvCM, mm, what}, {&pc.W, mm, what}, {&pc.info, info_bytes(Mp), what}, {&pc.info_b, info_bytes(Mp), what},
      {&pc.scal, 64, what}, {&pc.rho, 128 * 8, what},
      {&cg->partial, cg->have_noise ? size_t(64) * size_t(cg_dot_blocks(N)) * 8 : 0, what}});   // (sum_i log sigma_i^2: ensure_solver's own minimum)
  if (rc) return rc;
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
    rc = reserve_all(ctx, {{&pc.x64, size_t(d) * size_t(N) * 8, what}, {&pc.z64, size_t(d) * size_t(k) * 8, what},
                           {&pc.invl64, size_t(SVGP_MAX_D) * 8, what}, {&pc.rows64, size_t(d) * size_t(cg->Np) * 8, what},
                           {&pc.bias64, size_t(cg->Np) * 8, what}});
    if (rc) return rc;
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
    KmvArgs a = kmv_args(cg, p);
    a.rows = rows64;   // the fp64 operands, whatever the data dtype
    a.bias = bias64;
    a.invl = invl64;
    a.px = z64;
    a.ldp = ldz64;
    a.n = k;
    a.V = pc.zblk.p;
    a.ldv = N;
    a.ldo = Mp;
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

}  // namespace svgp

extern "C" {

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
  const CgPar par = par_of(desc);
  Panel Vp, Op;   // N x S in, k x S out
  if ((rc = stage_panel(ctx, Vp, V, ldv, cg->N, S, cg->es, on_device, true, "the panel")) != SVGP_OK) return rc;
  if ((rc = stage_panel(ctx, Op, out, ldo, cg->pc.k, S, cg->es, on_device, false, "the product")) != SVGP_OK) return rc;
  if ((rc = set_params(ctx, cg, par, false)) != SVGP_OK) return rc;
  if ((rc = pc_cross(ctx, cg, par, Vp.p, Vp.ld, S, Op.p, Op.ld)) != SVGP_OK) return rc;
  KCHECK(ctx, "kmv (row-split)");
  if ((rc = download_panel(ctx, Op)) != SVGP_OK) return rc;
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
  const CgPar par = par_of(desc);
  if (logdet_p_out) *logdet_p_out = std::numeric_limits<double>::quiet_NaN();
  Panel Rp, Op;
  if ((rc = stage_panel(ctx, Rp, R, ldr, N, S, cg->es, on_device, true, "the panel")) != SVGP_OK) return rc;
  if ((rc = stage_panel(ctx, Op, out, ldo, N, S, cg->es, on_device, false, "the product")) != SVGP_OK) return rc;
  int status = noise_check(ctx, cg, desc, true);
  if (status == SVGP_OK) status = set_params(ctx, cg, par);
  if (status != SVGP_OK && status != SVGP_NOT_POSDEF) return status;
  if (status == SVGP_OK) {
    TREC(ctx, ctx->ev[0], s);
    if ((rc = pc_apply(ctx, cg, par, Rp.p, Rp.ld, S, Op.p, Op.ld)) != SVGP_OK) return rc;
    TREC(ctx, ctx->ev[1], s);
    KCHECK(ctx, "cg preconditioner (apply)");
  } else if ((rc = nan_fill(ctx, cg->dtype, Op.p, Op.ld, N, S, true)) != SVGP_OK) {   // NaN outputs, the status and its message kept
    return rc;
  }
  if ((rc = download_panel(ctx, Op)) != SVGP_OK) return rc;
  HIPC(ctx, hipStreamSynchronize(s));
  if (status == SVGP_OK) {
    cg_timing(ctx, cg->pc.ms_setup);
    cg->pc.ms_setup = 0;
    if (logdet_p_out) *logdet_p_out = cg->pc.logdet_p;
  }
  return status;
}

}  // extern "C"
