// api_grad.hip — value and gradient of the ELBO: the workspace, the schedule of one evaluation (grad_enqueue), the data-parallel
// protocol around it, the read-back, and svgp_elbo_grad / _shard / _ext / _inputs / _ext_inputs / _with_mean,
// svgp_model_set_mean_z.  Host orchestration only (strip.hip / grad.hip hold the kernels).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"

using namespace svgp;

namespace svgp {

// split-K slice count of the SYRK for a chunk of nc points (the rule: grad_workspace)
int syrk_slices(const svgp_ctx* ctx, const svgp_model* m, int64_t nc) {
  static const int ns_forced = exp_int("SVGP_GEMM_PM_SLICES", 0);   // tuning knob (experiments build)
  if (ns_forced > 0) return ns_forced;
  const int64_t Mp = m->Mp;
  const int nP = int(Mp / 128), ntiles = nP * (nP + 1) / 2;
  const int items = ntiles * (m->dtype == SVGP_F64 ? 2 : 1), slots = 2 * ctx->num_cus;
  int ns = 1;
  double best = 0.0;
  for (int c = 1; c <= 64; ++c) {
    if (c > 1 && (size_t(c) * size_t(Mp) * size_t(Mp) * m->es > (size_t(2) << 30) || nc / c < 512)) break;
    const double wg = double(items) * c, eff = wg / (std::ceil(wg / slots) * slots);
    if (eff > best + 1e-9) { best = eff; ns = c; }
    if (eff >= 0.97) break;
  }
  return ns;
}

// points per chunk of a value-and-gradient evaluation over `len` points (a multiple of 128): the At / Pt buffers hold one chunk
int64_t grad_chunk_points(int64_t Mp, size_t es, int64_t len) {
  static const int64_t cap_cols = exp_ll("SVGP_GRAD_CHUNK", 65536ll);   // tuning knobs (experiments build)
  static const double cap_bytes = exp_double("SVGP_GRAD_CHUNK_BYTES", 1.0e9);
  int64_t cap = int64_t(cap_bytes / double(Mp * int64_t(es))) / 128 * 128;
  cap = cap < 128 ? 128 : (cap > cap_cols ? cap_cols : cap);
  int64_t nc = (len + 127) / 128 * 128;
  // a batch of at most two chunks' worth goes as ONE chunk (C2, 1e5 points: 3.7 -> 3.5 ms - one SYRK / kgrad launch, no drain between
  // the strips of the two chunks); longer batches keep the 65 536-point chunks (H, H32 flat from 32 768 to 262 144; C5 best at 65 536)
  if (nc > cap && nc <= 2 * cap && double(nc) * double(Mp * int64_t(es)) <= 2.0 * cap_bytes) cap = nc;
  return nc < cap ? nc : cap;
}

int grad_workspace(svgp_ctx* ctx, svgp_model* m, int64_t len, GradWs** out) {
  const size_t es = m->es;
  const int64_t Mp = m->Mp;
  const int64_t nc = grad_chunk_points(Mp, es, len);
  GradWs* w = ctx->gws;
  if (w && w->dtype == m->dtype && w->Mp == Mp && w->d == m->d && w->nc >= nc) { *out = w; return SVGP_OK; }
  delete w;
  ctx->gws = nullptr;
  w = new (std::nothrow) GradWs();
  if (!w) return SVGP_OOM;
  w->dtype = m->dtype; w->Mp = Mp; w->d = m->d; w->nc = nc;
  // Split-K slices of the SYRK: work items = tiles (f64: two 128 x 64 halves each) x slices over 2 workgroup slots per CU.  The
  // smallest count whose last round of slots is >= 97 % full, else the fullest (H: 72 items, 7 slices = 504 of 512; C3: 136 items,
  // 11 slices = 1496 of 1536 - the round-2 rule floor(512 / tiles) left C3 with 408 of 512: 175 -> 164 ms), within 2 GiB of slice
  // buffer and >= 512 points per slice.  Placing the items of a slice on one XCD (they read the same rows of A) was measured
  // and rejected: H 81.9 -> 85-87 ms - the operand re-reads come out of the Infinity Cache at no cost to the MFMA pipe.
  w->nslices = syrk_slices(ctx, m, int64_t(1) << 40);   // the buffer holds the count an unbounded chunk would take: a call's count never exceeds it
  w->rb = grad_rowblocks(m->dtype, m->d, Mp);
  // workgroups per CU of the kernel-gradient reductions (grad.hip: kgrad_mfma_kernel): as many as its registers and LDS admit - the kernel
  // is a chain global load -> MFMA -> kernel function -> MFMA per 16-point tile and lives off the waves it can interleave (rocprofv3, us
  // per 65 536-point chunk at M = 1024, 2 / 3 / 4 / 6 per CU: d = 8 f64 185 / 171 / 162 / 177, fp32 115 / 99 / 88 / 104; d = 64 f64, whose
  // 72 KiB of LDS admit two, 512 / 671 / 549 / 598; profiles/round6/kgrad_wg_per_cu.log)
  const int kg_dflt = grad_dreg(m->d) <= 16 ? 4 : (grad_dreg(m->d) <= 32 ? 3 : 2);
  static const int kg_knob = exp_int("SVGP_KGRAD_WG_PER_CU", 0);   // tuning knob (experiments build)
  const int kg_wg = kg_knob > 0 ? kg_knob : kg_dflt;
  int nu = (kg_wg * ctx->num_cus + w->rb - 1) / w->rb;
  w->ns_uf = nu < 1 ? 1 : (nu > 256 ? 256 : nu);
  w->ns_uu = 8;
  const int dreg = grad_dreg(m->d);
  const size_t mn = size_t(Mp) * size_t(nc) * es, mm = size_t(Mp) * size_t(Mp) * es;
  w->g_b = size_t(w->nslices) * mm;
  w->rp_uf_b = size_t(w->ns_uf) * (2 + dreg) * Mp * 8; w->sp_uf_b = size_t(w->ns_uf) * w->rb * (1 + dreg) * 8;
  w->rp_uu_b = size_t(w->ns_uu) * (2 + dreg) * Mp * 8; w->sp_uu_b = size_t(w->ns_uu) * w->rb * (1 + dreg) * 8;
  w->part5_strips = nc / 32 + 2;   // narrowest strips: 32 points
  // [rp_uf | sp_uf | rp_uu | sp_uu | sums (8) | scal_out (1 + dreg) | prep scalars (4) + info (1)]: one memset, and the tail
  // [sums .. info] is the ONE fp64 read-back of an evaluation
  w->zero_b = w->rp_uf_b + w->sp_uf_b + w->rp_uu_b + w->sp_uu_b + size_t(8 + 1 + dreg + 5) * 8;
  struct { DevBuf* p; size_t b; } req[] = {
      {&w->At, mn}, {&w->Pt, mn}, {&w->gmu, 2 * size_t(nc) * es + 256},   // g_mu | g_v contiguous: one memset per chunk (+ the SYRK's weight DMA reads 256 B at a time)
      {&w->Lqp, mm}, {&w->G1, w->g_b}, {&w->G2, mm}, {&w->LkRM, mm},
      {&w->LbarRM, mm}, {&w->Phi, mm}, {&w->tmp, mm}, {&w->H, mm}, {&w->LinvRM, mm}, {&w->LinvCM, mm},
      // the user-layout blocks hold M d + M + M^2 elements; sized by Mp because the workspace is reused for every model of the
      // same (dtype, Mp, d), whatever its M (M = 45 then M = 96 on one context overran the smaller buffers)
      {&w->gblk, (size_t(Mp) * m->d + size_t(Mp)) * es + mm}, {&w->cblk, (size_t(Mp) * m->d + size_t(Mp)) * es + mm / 2 + size_t(Mp) * es},
      {&w->BbarRM, mm}, {&w->rbar, size_t(Mp) * es},
      {&w->W2, mm}, {&w->Rcm, mm}, {&w->G1p, mm}, {&w->alpha, size_t(Mp) * es}, {&w->avec, size_t(Mp) * 8},
      {&w->gemv_part, size_t(Mp / 128) * size_t(Mp) * 8},
      {&w->zero_blk, w->zero_b},
      {&w->partial5, size_t(w->part5_strips) * 5 * 8}, {&w->invl_d, size_t(m->d) * 8},
      {&w->kred, (size_t(2 + dreg) * size_t(Mp) + size_t(1 + dreg)) * 8}};
  for (auto& r : req) {
    if (r.p->alloc(r.b) != hipSuccess) {
      delete w;
      return alloc_failed(ctx, "for the gradient workspace");
    }
  }
  w->gv = static_cast<char*>(w->gmu.p) + size_t(nc) * es;
  {
    char* z = static_cast<char*>(w->zero_blk.p);
    w->rp_uf = reinterpret_cast<double*>(z); z += w->rp_uf_b;
    w->sp_uf = reinterpret_cast<double*>(z); z += w->sp_uf_b;
    w->rp_uu = reinterpret_cast<double*>(z); z += w->rp_uu_b;
    w->sp_uu = reinterpret_cast<double*>(z); z += w->sp_uu_b;
    w->sums = reinterpret_cast<double*>(z);
  }
  w->scal_out = w->sums + 8;   // contiguous with sums: the data-parallel path all-reduces [sums | scal_out] in one piece
  // Linv is written block-lower only and the products skip the tiles above the diagonal, but the stale upper part of a reused
  // buffer must at least be finite (0 x NaN): start from zeros once
  for (void* p : {w->LinvRM.p, w->LinvCM.p})
    if (hipMemsetAsync(p, 0, mm, ctx->stream) != hipSuccess) {
      delete w;
      return fail(ctx, SVGP_HIP_ERROR, "memset failed");
    }
  // the point-major chunk buffers are read beyond the written points of a short last chunk (against g_v = 0): start from zeros
  for (void* p : {w->At.p, w->Pt.p})
    if (hipMemsetAsync(p, 0, mn, ctx->stream) != hipSuccess) {
      delete w;
      return fail(ctx, SVGP_HIP_ERROR, "memset failed");
    }
  ctx->gws = w;
  *out = w;
  return SVGP_OK;
}

}  // namespace svgp

namespace {

// out = Xt' Yt for M x M operands ("k-major": Xt[k][r] at Xt[k Mp + r]; a row-major matrix Z is the operand Z, a column-major
// one is Z').  Lower 128-tiles of the row-major result, or all tiles with kMmFull; kMm?Low / kMm?Up name triangular operands
// (half the k-steps).  One workgroup pair per tile is 72 (128) workgroups at M = 1024 for 256 CUs, so the product is split
// along K into slices whose partials land in `scratch` ([ns][Mp][Mp], the SYRK's slice buffer when it is idle) and are summed
// in a fixed order.  The result OVERWRITES `out` (no pre-zeroing: round 2 spent a memset per product on it).
void gemm_mm(svgp_ctx* ctx, GradWs* w, int dt, hipStream_t s, const void* Xt, const void* Yt, int64_t Mp, void* out, int flags = 0,
             void* scratch = nullptr) {   // scratch: [min(nP, nslices)][Mp][Mp] instead of the SYRK's slice buffer
  const int nP = int(Mp / 128), ntiles = (flags & kMmFull) ? nP * nP : nP * (nP + 1) / 2;
  int ns = (2 * ctx->num_cus) / (ntiles * (dt == SVGP_F64 ? 2 : 1));   // fill the workgroup slots once (f64: two 128 x 64 halves per tile)
  if (ns > nP) ns = nP;                         // at least 8 k-steps of 16 per slice
  if (ns > w->nslices) ns = w->nslices;         // the scratch is the SYRK's [nslices][Mp][Mp]
  static const int knob = exp_int("SVGP_GEMM_MM_SPLITK", 1);   // A/B knob (experiments build)
  if (ns < 2 || !knob) {
    launch_gemm_pm(dt, s, Xt, Yt, nullptr, 1.0, Mp, Mp, Mp, 1, out, 1, flags);
    return;
  }
  const int64_t sl = ((Mp + ns - 1) / ns + 15) / 16 * 16;
  void* sc = scratch ? scratch : w->G1.p;
  launch_gemm_pm(dt, s, Xt, Yt, nullptr, 1.0, Mp, Mp, sl, ns, sc, 1, flags);
  launch_sum_slices_lower(dt, s, sc, ns, Mp, out, (flags & kMmFull) ? 1 : 0, 1);
}

// ---- the schedule of one value-and-gradient evaluation -------------------------------------------------------------------------
// What the stages of grad_enqueue_impl share: the call, its sizes, and the plan made by grad_plan.
struct GradRun {
  svgp_ctx* ctx = nullptr;
  svgp_model* m = nullptr;
  const svgp_data* data = nullptr;
  int64_t off = 0, len = 0;
  GradCall* gc = nullptr;
  GradWs* w = nullptr;
  hipStream_t s = nullptr;
  int dt = 0, dreg = 0;
  int64_t Mp = 0, M = 0;
  size_t es = 8;
  bool centered = false;
  int64_t nc = 0;        // this call's chunk
  int ns_syrk = 1;       // the SYRK's slices
  LikParams lp{};
  KernelParams kp{};
  double *ext_gmu = nullptr, *ext_gv = nullptr;   // the host's point gradients: their place on the device
  bool uniform_w = false, syrk_early = false;
  OverlapPlan gop;
  // the adjoint runs on the whitened problem: (m~, B) are (m, Lq) for NonCentered and (Lk^-1 (m - c), Lk^-1 Lq) for Centered
  const void* Bq = nullptr;
  // segmented strips (gop.on): enqueued panel by panel from inside the factorisation's launch loop (SegRun), so built before the prep
  SegRun gseg;
  LikParams lpc_seg{};
};

// Stage 1: workspace / overlap plan - every size and every allocation of the call, the host's point gradients onto the device
int grad_plan(GradRun& g) {
  svgp_ctx* ctx = g.ctx;
  svgp_model* m = g.m;
  GradCall& gc = *g.gc;
  const int64_t len = g.len;
  hipStream_t s = g.s;
  GradWs* w = gc.w;
  if (!w) {
    int rcw = grad_workspace(ctx, m, len, &w);
    if (rcw) return rcw;
    gc.w = w;
  }
  g.w = w;
  int rc = SVGP_OK;
  gc.len = len;
  const int dt = g.dt = m->dtype;
  const int64_t Mp = g.Mp = m->Mp, M = g.M = m->M;
  // this call's chunk (a reused workspace may hold more: the chunking - and with it the summation order - depends on the call only)
  const int64_t nc = g.nc = std::min<int64_t>(w->nc, grad_chunk_points(Mp, m->es, len));
  g.ns_syrk = std::min(w->nslices, syrk_slices(ctx, m, nc));   // the SYRK's slices: a function of the call, like the chunk
  const size_t es = g.es = m->es;
  g.dreg = grad_dreg(m->d);
  // the user-layout gradient blocks of THIS model, contiguous: {z_bar | m_bar | Lq_bar}
  w->zbar = w->gblk.p;
  w->mbar = static_cast<char*>(w->gblk.p) + size_t(M) * m->d * es;
  w->Lqbar = static_cast<char*>(w->mbar) + size_t(M) * es;
  // Strips beside the factorisation (round 4): a one-chunk, one-round batch runs its phase 1 as segmented strips on the second
  // stream - panel I behind the event of block row I of T - and its phase 3 behind the M-sized gradient prep (Linv, alpha, R) that
  // the main stream computes meanwhile.  Same conditions as the forward path (overlap_plan), plus: the whole batch is one chunk.
  OverlapPlan& gop = g.gop;
  if (len <= nc && g.centered == false) {
    gop = overlap_plan(ctx, m, len);   // (one round of the single-launch plan's strips: no concurrent tail there)
    if (gop.on) {
      rc = ensure_overlap(ctx, size_t(gop.nstrips) * strip_seg_state_doubles(dt, gop.nt));
      // the size the chunk loop below asks for (per workgroup >= per strip here): nothing may reallocate once segments are enqueued
      if (rc == SVGP_OK) rc = ensure_scratch(ctx, 2 * strip_work_bytes(dt, Mp, gop.nt, gop.grid > int(gop.nstrips) ? gop.grid : int(gop.nstrips)), size_t(nc));
      if (rc) return rc;
    }
  }
  g.lp = lik_params(m);
  g.kp = kparams(m);
  if (gc.ext_gmu) {   // the host's point gradients: one H2D copy of 2 x len doubles
    rc = ctx->ext_g.reserve(ctx, 2 * size_t(len) * 8, "the point gradients");
    if (rc) return rc;
    g.ext_gmu = ctx->ext_g.as<double>();
    g.ext_gv = g.ext_gmu + ctx->ext_g.cap / 16;   // [2][capacity in points]
    HIPC(ctx, hipMemcpyAsync(g.ext_gmu, gc.ext_gmu, size_t(len) * 8, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(g.ext_gv, gc.ext_gv, size_t(len) * 8, hipMemcpyHostToDevice, s));
  }
  // The likelihood gradients come from point_grad_kernel behind the strips (both likelihood routes); A g_mu (the data part of m_bar): the
  // kernel-gradient reductions, which evaluate the kernel anyway, sum Kuf g_mu and the tail applies Lk^-1 (one gemv with the explicit
  // inverse), so A is read by the SYRK only (round 3, f64: 0.32 -> 0.2 ms per 65 536-point chunk at M = 1024).
  // the SYRK's weights 2 g_v are uniform over the points for the built-in Gaussian likelihood (grad.hip: UW) unless a variance was
  // negative and clamped (then that point's g_v differs... it does not: dE/dv = -1 / (2 sigma^2) whatever v) - so: Gaussian, built in
  g.uniform_w = m->desc.likelihood == SVGP_LIK_GAUSSIAN && !gc.ext_gmu && m->gh_n == 0 && ctx->kn.syrk_uniform && !gc.noise;   // (knob: experiments build; per-point noise: g_v_j = -scale / (2 sigma_j^2))
  // Round 6: strips beside the factorisation + uniform weights = the SYRK needs nothing but A, which phase 1 has
  // written by the time the chain ends - so it goes on the second stream right behind the last phase-1 segment, BESIDE the M-sized prep
  // of phase 3 on the main stream (Lk^-1 by recursive doubling, R, alpha: ~230 us of small launches at M = 1024), instead of behind
  // phase 3 and the kernel-gradient reductions.  Same kernel, same slices, same single overwrite of the slice buffer: bitwise the
  // serial result.  The one M x M product that runs meanwhile (R) takes a split-K scratch of its own.  Measured (same box, update +
  // value and gradient, ms): 16 384 points M = 1024 f64 2.72 -> 2.67, fp32 1.94 -> 1.88; 4 096 points 1.87 -> 1.81 - the SYRK's 504
  // workgroups and the prep's small launches slow each other, so only a quarter of the 230 us comes back (profiles/round6/minibatch_trace.md).
  static const int early_knob = exp_int("SVGP_SYRK_EARLY", 1);   // (experiments build: 0 = the SYRK behind phase 3, as rounds 3-5)
  g.syrk_early = gop.on && g.uniform_w && early_knob != 0;
  if (g.syrk_early) {   // (the size is a function of the workspace's shape: allocated once)
    rc = w->Gmm.reserve(ctx, size_t(std::min<int64_t>(Mp / 128, w->nslices)) * size_t(Mp) * size_t(Mp) * m->es, "the gradient workspace");
    if (rc) return rc;
  }
  g.Bq = g.centered ? m->B.p : w->Lqp.p;
  return SVGP_OK;
}

// the strips' arguments for the chunk [c0, c0 + clen) (scratch / moment pointers: read after the ensure_scratch of the caller)
StripArgs grad_strip_args(const GradRun& g, int64_t c0, int64_t clen, LikParams& lpc) {
  const GradCall& gc = *g.gc;
  StripArgs a = strip_args(g.ctx, g.m, g.data->x.p, g.data->ldx, g.off + c0, clen);   // (its moments: read by launch_point_grads)
  a.At_out = g.w->At.p;
  if (gc.mux) a.mux = static_cast<const char*>(gc.mux) + size_t(c0) * g.es;   // (c0: the chunk's first point inside the batch)
  a.R = g.w->Rcm.p; a.alpha = g.w->alpha.p; a.Pt_out = g.w->Pt.p;
  lpc = g.lp;
  if (gc.ext_gmu) { lpc.lik = kLikExternal; lpc.gh_x = g.ext_gmu + c0; lpc.gh_w = g.ext_gv + c0; }   // (launch_point_grads' arguments)
  return a;
}

// Stage 2: the M-sized work of the adjoint that does NOT depend on the factorisation: the cleared accumulators, the inverse
// lengthscales for the kernel-gradient kernels, S = B B' - I (B = the padded Lq: NonCentered) - ~60 us of small launches.  Serial path:
// behind the prep on the main stream.  Strips beside the factorisation: on the second stream AHEAD of the pre-generation (that stream
// has nothing to do until block row 0 of T exists, ~130 us into the chain), the main stream waits for ev_S before it forms R.
int grad_pre_chain(GradRun& g, hipStream_t st) {
  svgp_ctx* ctx = g.ctx;
  svgp_model* m = g.m;
  GradWs* w = g.w;
  HIPC(ctx, hipMemsetAsync(w->zero_blk.p, 0, w->zero_b, st));   // every accumulator of the evaluation, one fill
  // (as kernel arguments: a hipMemcpyAsync from pageable memory blocks the host until the stream gets there - on the second stream
  // that was ~45 us during which the main stream's Kuu launch was not even enqueued)
  launch_setvec_f64(st, w->invl_d.as<double>(), m->invl_host.data(), m->d);
  if (!g.centered) launch_pad_lower(g.dt, st, m->Lq_raw.p, g.M, g.Mp, w->Lqp.p);
  gemm_mm(ctx, w, g.dt, st, g.Bq, g.Bq, g.Mp, w->G2.p, kMmXUp | kMmYUp);   // lower tiles of B B' (row-major); B[r][k] = 0 for k > r
  launch_sym_from_lower(g.dt, st, w->G2.p, 1, g.Mp, 1.0, w->tmp.p);         // S = B B' - I, full
  KCHECK(ctx, "grad prep (S)");
  return SVGP_OK;
}
// ... as the segmented strips' SegRun::pre: on the second stream, ev_S behind it
int grad_pre_chain_seg(void* user) {
  GradRun& g = *static_cast<GradRun*>(user);
  const int rcp = grad_pre_chain(g, g.ctx->stream2);
  if (rcp) return rcp;
  HIPC(g.ctx, hipEventRecord(g.ctx->ev_S, g.ctx->stream2));
  return SVGP_OK;
}

// Stage 3: the M-sized operands of the strips' phase 3 (main stream, behind the prep)
int grad_phase3_operands(GradRun& g) {
  svgp_ctx* ctx = g.ctx;
  svgp_model* m = g.m;
  GradWs* w = g.w;
  hipStream_t s = g.s;
  const int dt = g.dt;
  const int64_t Mp = g.Mp;
  // Linv = Lk^-1 (both storage orders): every Lk^-T . below is a GEMM with it (round 2: four blocked substitutions, 0.18 ms each
  // at M = 1024 whatever the batch size)
  launch_linv(dt, s, m->L.p, m->T.p, Mp, w->LinvRM.p, w->LinvCM.p, w->H.p);
  // M-sized operands of the strips' phase 3:  R = Lk^-T (B B' - I)  (column-major: the P operand of the GEMM); then, for the
  // kernel-gradient reductions behind the strips, alpha = Lk^-T m~ (no strip reads it: it follows ev_R)
  gemm_mm(ctx, w, dt, s, w->tmp.p, w->LinvRM.p, Mp, w->Rcm.p, kMmFull | kMmYLow, g.syrk_early ? w->Gmm.p : nullptr); // out[c][r] = sum_k S[k][c] Linv[k][r] = R[r][c]: R column-major
  KCHECK(ctx, "grad prep");
  if (g.gop.on) HIPC(ctx, hipEventRecord(ctx->ev_R, s));   // R is final: the segmented strips' closing launch (phase 3) may run
  launch_linv_t_gemv(dt, s, w->LinvRM.p, m->mp.p, Mp, w->alpha.p, w->gemv_part.as<double>());
  return SVGP_OK;
}

// Stage 4: the chunk body - the strips of the chunk [c0, c0 + clen), its point gradients, kernel-gradient reductions and SYRK
int grad_chunk(GradRun& g, int64_t c0) {
  svgp_ctx* ctx = g.ctx;
  svgp_model* m = g.m;
  const svgp_data* data = g.data;
  const GradCall& gc = *g.gc;
  GradWs* w = g.w;
  hipStream_t s = g.s;
  const OverlapPlan& gop = g.gop;
  const int dt = g.dt, ns_syrk = g.ns_syrk;
  const int64_t Mp = g.Mp, M = g.M, off = g.off, len = g.len, nc = g.nc;
  const size_t es = g.es;
  const double scale = gc.scale;
  const double* n_global_dev = gc.n_global_dev;   // data-parallel: the all-reduced batch size, on the device (grad_handshake)
  const int64_t clen = (len - c0 < nc) ? len - c0 : nc;
  const int64_t ncp = (clen + 127) / 128 * 128;
  // forward strips + likelihood gradients + phase 3 in ONE launch: leaves A, P point-major and g_mu, g_v of the chunk
  const SinglePlan plan = single_plan(dt, Mp, clen, ctx->num_cus);
  const int nt = plan.nt, grid = plan.grid;
  const int64_t nstrips = plan.nstrips;
  // (g_mu | g_v, w->nc apart: the weighted SYRK reads g_v over the chunk padded to 128 points - launch_point_grads writes that padding)
  LikParams lpc{};
  StripArgs a = gop.on ? g.gseg.a : grad_strip_args(g, c0, clen, lpc);
  if (gop.on) lpc = g.lpc_seg;
  if (gop.on) {   // (single chunk) the segments are on the second stream already; the closing launch (phase 2 + 3) waits for R and alpha,
                  // and the main stream joins before the point gradients
    hipStream_t s2 = ctx->stream2;
    const int nPn = int(Mp / 128);
    if (a.work != ctx->work.p || a.mom_mu != ctx->mom_mu()) return fail(ctx, SVGP_HIP_ERROR, "internal: scratch moved under the segmented strips");
    // A small batch has fewer strips than the chip has workgroup slots and phase 3 - 2 M^2 flops per point, one panel after the other
    // inside a strip's workgroup - is latency-bound on the few CUs it reaches (1024 points, M = 1024: 32 workgroups, 340 us for 27 us
    // of MFMA work).  Its output panels are independent: the closing launch runs S workgroups per strip (strip.hip: seg_split).
    // SVGP_SEG_SPLIT=0 (per call): the unsplit launch, whose result is bitwise the serial kernel's (the split one differs in the
    // variance's summation order).
    const int S = seg_split_factor(ctx, nPn, nstrips);
    int cgrid = grid;
    if (S > 1) {
      const int rc = seg_split_setup(ctx, a, S, nstrips);
      if (rc) return rc;
      cgrid = int(nstrips) * S;
    }
    if (g.syrk_early) {   // W = w A A' behind the last phase-1 segment, beside the main stream's Lk^-1 / R / alpha
      const int64_t n16 = (clen + 15) / 16 * 16, sl_e = ((ncp + ns_syrk - 1) / ns_syrk + 15) / 16 * 16;
      if (n16 > clen) HIPC(ctx, hipMemsetAsync(static_cast<char*>(w->At.p) + size_t(clen) * size_t(Mp) * es, 0, size_t(n16 - clen) * size_t(Mp) * es, s2));
      launch_syrk_uniform(dt, s2, w->At.p, -0.5 / g.lp.sigma2, scale, n_global_dev, gc.num_data, 2.0, Mp, n16, sl_e, ns_syrk, w->G1.p, 1);
      KCHECK(ctx, "syrk (beside the prep of phase 3)");
    }
    HIPC(ctx, hipStreamWaitEvent(s2, ctx->ev_R, 0));
    a.seg_lo = a.seg_hi = nPn;
    a.seg_flags = kSegLoad | kSegPhase2;
    launch_strip_seg(dt, s2, a, nt, cgrid, nstrips, true);
    KCHECK(ctx, "strip (value and gradient, segmented)");
    HIPC(ctx, hipEventRecord(ctx->ev_join, s2));
    HIPC(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
  } else {
    // the head of the strips' queue: zeroed here for the first chunk, by the previous chunk's launch_point_grads for the others
    if (c0 == 0) HIPC(ctx, hipMemsetAsync(a.counter, 0, sizeof(unsigned), s));
    launch_strip_grad(dt, s, a, nt, grid, nstrips);
    KCHECK(ctx, "strip (value and gradient)");
  }
  if (gc.noise || gc.noise_bar) {   // svgp_collapsed_grad_with_noise (Gaussian, closed form, never collective): point j with sigma_j^2
    launch_point_grads_noise(dt, s, lpc.sigma2, lpc.clamp_neg_var, a.mom_mu, a.mom_var, data->y.p, off + c0, clen, scale,
                             gc.noise ? static_cast<const char*>(gc.noise) + size_t(c0) * es : nullptr, w->gmu.p, w->gv,
                             w->partial5.as<double>(), gop.on ? nullptr : a.counter, ncp,
                             gc.mux_bar ? static_cast<char*>(gc.mux_bar) + size_t(c0) * es : nullptr,
                             gc.noise_bar ? static_cast<char*>(gc.noise_bar) + size_t(c0) * es : nullptr);
  } else {
    launch_point_grads(dt, s, lpc, a.mom_mu, a.mom_var, gc.ext_gmu ? nullptr : data->y.p, off + c0, clen, scale, n_global_dev, gc.num_data, w->gmu.p, w->gv,
                       w->partial5.as<double>(), gop.on ? nullptr : a.counter, ncp,
                       gc.mux_bar ? static_cast<char*>(gc.mux_bar) + size_t(c0) * es : nullptr);
  }
  KCHECK(ctx, "point gradients");
  const int n5 = point_grad_blocks(clen);   // rows of partial5: one per 256-point block
  int64_t ksl = ((clen + w->ns_uf - 1) / w->ns_uf + 127) / 128 * 128;
  launch_kgrad(dt, s, g.kp, m->zs.p, Mp, M, data->x.p, data->ldx, off + c0, 0, clen, clen, w->Pt.p, w->gmu.p, w->gv, w->alpha.p, ksl, w->ns_uf,
               w->rp_uf, w->sp_uf, 1);
  KCHECK(ctx, "kgrad uf");
  if (gc.gx) {   // d elbo / d x of the chunk's points, from the same P while Pt holds the chunk (host output: into w->xg, [d][len])
    const bool dev = gc.gx->on_device != 0;
    launch_xgrad(dt, s, g.kp, m->zs.p, Mp, M, data->x.p, data->ldx, off + c0, clen, w->Pt.p, w->gmu.p, w->gv, w->alpha.p, dev ? gc.gx->x : w->xg.p,
                 dev ? gc.gx->ld : len, c0);
    KCHECK(ctx, "xgrad");
  }
  launch_sum5(s, w->partial5.as<double>(), n5, w->sums);
  int64_t sl = ((ncp + ns_syrk - 1) / ns_syrk + 15) / 16 * 16;   // as even as the 16-point k-step allows
  // W (+)= A diag(2 g_v) A' (lower tiles, split-K slices): the first chunk overwrites, so the slice buffer needs no zeroing
  if (g.syrk_early) {
    // (already on the second stream, joined above)
  } else if (g.uniform_w) {
    // g_v is the same for every point (Gaussian: -scale / (2 sigma^2)): the unweighted loop, the weight applied to the accumulators.
    // Columns of the chunk's last strip beyond its last point hold the replicated last point: zero them up to the k-step boundary
    const int64_t n16 = (clen + 15) / 16 * 16;
    if (n16 > clen) HIPC(ctx, hipMemsetAsync(static_cast<char*>(w->At.p) + size_t(clen) * size_t(Mp) * es, 0, size_t(n16 - clen) * size_t(Mp) * es, s));
    launch_syrk_uniform(dt, s, w->At.p, -0.5 / g.lp.sigma2, scale, n_global_dev, gc.num_data, 2.0, Mp, n16, sl, ns_syrk, w->G1.p, c0 == 0 ? 1 : 0);
  } else {
    launch_gemm_pm(dt, s, w->At.p, w->At.p, w->gv, 2.0, Mp, ncp, sl, ns_syrk, w->G1.p, c0 == 0 ? 1 : 0);
  }
  KCHECK(ctx, "syrk");
  return SVGP_OK;
}

// Stage 5: the M-sized tail.  With W = A diag(2 g_v) A' and a = A g_mu:
//   Lq_bar = tril(W B) - klw dKL/dB,   Lk_bar = -tril(alpha a' + R W)     (B = Lq whitened; W, R carry the factors 2)
int grad_tail(GradRun& g) {
  svgp_ctx* ctx = g.ctx;
  svgp_model* m = g.m;
  GradWs* w = g.w;
  hipStream_t s = g.s;
  const int dt = g.dt;
  const int64_t Mp = g.Mp, M = g.M;
  const bool centered = g.centered;
  launch_sym_from_lower(dt, s, w->G1.p, g.ns_syrk, Mp, 0.0, w->W2.p);
  gemm_mm(ctx, w, dt, s, w->W2.p, m->U.p, Mp, w->G1p.p, kMmYLow);   // (W B)[r][c] = sum_i W[i][r] B[i][c]; B[i][c] = 0 for i < c
  gemm_mm(ctx, w, dt, s, w->Rcm.p, w->W2.p, Mp, w->G2.p);           // (R W)[r][c] = sum_i R[r][i] W[i][c]
  launch_avec(s, w->rp_uf, w->ns_uf, int64_t(2 + g.dreg) * Mp, Mp, w->avec.as<double>());
  // avec holds Kuf g_mu: A g_mu = Lk^-1 (Kuf g_mu)
  launch_linv_t_gemv(dt, s, w->LinvCM.p, w->avec.as<double>(), Mp, w->avec.as<double>(), w->gemv_part.as<double>(), 1, 1);   // avec is fp64 in both builds
  launch_finish_mm2(dt, s, w->G1p.p, w->G2.p, w->alpha.p, w->avec.as<double>(), Mp, M, centered ? m->B.p : m->Lq_raw.p, centered ? Mp : M, g.gc->klw, w->Lqbar,
                    centered ? w->BbarRM.p : nullptr, w->LbarRM.p);
  KCHECK(ctx, "Lq_bar / Lk_bar");
  return SVGP_OK;
}

// Stage 6 (Centered): the chain through m~ = Lk \ (m - c) and B = Lk \ Lq:  m_bar = Lk^-T m~_bar,  Rb = Lk^-T B_bar,  Lq_bar = tril(Rb),
// Lk_bar -= tril(m_bar m~') + tril(Rb B')
int grad_centered_chain(GradRun& g) {
  svgp_ctx* ctx = g.ctx;
  svgp_model* m = g.m;
  GradWs* w = g.w;
  hipStream_t s = g.s;
  const int dt = g.dt;
  const int64_t Mp = g.Mp, M = g.M;
  launch_mbar(dt, s, w->avec.as<double>(), m->mp.p, g.gc->klw, M, Mp, w->rbar.p);
  launch_linv_t_gemv(dt, s, w->LinvRM.p, w->rbar.p, Mp, w->alpha.p, w->gemv_part.as<double>());   // alpha is free after finish_mm2: holds m_bar (padded)
  HIPC(ctx, hipMemcpyAsync(w->mbar, w->alpha.p, size_t(M) * g.es, hipMemcpyDeviceToDevice, s));
  // out[c][r] = sum_i B_bar[i][c] Linv[i][r] = Rb[r][c]: Rb column-major = the k-major operand of Rb B' below
  gemm_mm(ctx, w, dt, s, w->BbarRM.p, w->LinvRM.p, Mp, w->tmp.p, kMmFull | kMmXLow | kMmYLow);
  launch_cm_tril_to_user(dt, s, w->tmp.p, Mp, M, w->Lqbar);
  gemm_mm(ctx, w, dt, s, w->tmp.p, m->B.p, Mp, w->Phi.p, kMmYUp);   // (Rb B')[r][c] = sum_i Rb[r][i] B[c][i]; B[c][i] = 0 for i > c
  launch_lbar_adjust(dt, s, w->LbarRM.p, w->Phi.p, w->alpha.p, m->mp.p, Mp);
  KCHECK(ctx, "centered chain");
  return SVGP_OK;
}

// Stage 7: the Cholesky backward, Kuu_bar = sym(Lk^-T Phi(Lk' Lk_bar) Lk^-1), and the Kuu part of the kernel gradients
int grad_chol_backward(GradRun& g) {
  svgp_ctx* ctx = g.ctx;
  svgp_model* m = g.m;
  GradWs* w = g.w;
  hipStream_t s = g.s;
  const int dt = g.dt;
  const int64_t Mp = g.Mp, M = g.M;
  launch_lower_to_rowmajor(dt, s, m->L.p, Mp, w->LkRM.p);
  gemm_mm(ctx, w, dt, s, w->LkRM.p, w->LbarRM.p, Mp, w->Phi.p, kMmXLow | kMmYLow);   // (Lk' Lk_bar)[r][c], lower tiles
  launch_phi(dt, s, w->Phi.p, Mp);                                               // tril, diagonal halved; zero above
  gemm_mm(ctx, w, dt, s, w->Phi.p, w->LinvRM.p, Mp, w->tmp.p, kMmFull | kMmXLow | kMmYLow);   // out[c][r] = sum_i Phi[i][c] Linv[i][r] = (Linv' Phi)[r][c]
  gemm_mm(ctx, w, dt, s, w->tmp.p, w->LinvRM.p, Mp, w->G1p.p, kMmFull | kMmYLow);             // out[r][c] = sum_j (Linv' Phi)[r][j] Linv[j][c]
  launch_symmetrize(dt, s, w->G1p.p, Mp, w->H.p);
  KCHECK(ctx, "chol backward");
  // the Kuu part: the ns_uu slices must cover all M columns (a fixed slice of 128 covered only 1024 of them: the kernel-
  // parameter and z gradients were wrong for M > 1024 until tests/test_gpu_grad.py::test_gradient_large_m_float32_strips)
  const int64_t uu_sl = ((M + w->ns_uu - 1) / w->ns_uu + 127) / 128 * 128;
  launch_kgrad(dt, s, g.kp, m->zs.p, Mp, M, m->zs.p, Mp, 0, 1, M, M, w->H.p, nullptr, nullptr, nullptr, uu_sl, w->ns_uu, w->rp_uu, w->sp_uu);
  launch_finish_kgrad(dt, s, m->d, M, Mp, m->zs.p, w->invl_d.as<double>(), w->rp_uf, w->ns_uf, w->rp_uu, w->ns_uu, w->sp_uf, w->ns_uf * w->rb,
                      w->sp_uu, w->ns_uu * w->rb, m->mp.p, g.gc->klw, m->desc.layout_z, m->desc.variance, w->zbar, g.centered ? nullptr : w->mbar,
                      w->scal_out, w->kred.as<double>(), w->avec.as<double>());
  // status slots of the all-reduced scalars + this rank's prep scalars / info behind them: ONE fp64 read-back per evaluation
  launch_grad_status(s, w->sums, m->info.as<int>(), double(g.len), m->scal.as<double>(), w->scal_out + 1 + g.dreg);
  KCHECK(ctx, "kgrad uu / finish");
  return SVGP_OK;
}

int grad_enqueue_impl(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, GradCall& gc) {
  GradRun g;
  g.ctx = ctx; g.m = m; g.data = data; g.off = off; g.len = len; g.gc = &gc;
  g.centered = gc.centered = (m->desc.parametrization == SVGP_CENTERED);
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = g.s = ctx->stream;
  int rc = grad_plan(g);
  if (rc) return rc;
  GradWs* w = g.w;
  const OverlapPlan& gop = g.gop;
  RowHook ghook{seg_row_hook, &g.gseg};
  if (gop.on) {
    SegRun& gseg = g.gseg;
    gseg.ctx = ctx; gseg.m = m; gseg.op = gop; gseg.grad = true; gseg.nP = int(g.Mp / 128);
    gseg.a = grad_strip_args(g, 0, len, g.lpc_seg);
    gseg.a.seg_state = ctx->seg_state.as<double>();
    gseg.a.counter = ctx->counter2.as<unsigned>();
    gseg.pre = grad_pre_chain_seg;
    gseg.pre_user = &g;
  }
  ctx->overlapped = gop.on;
  TREC(ctx, ctx->ev[0], s);
  rc = enqueue_prep(ctx, m, gop.on, gop.on ? &ghook : nullptr);
  if (rc == SVGP_OK && gop.on) rc = g.gseg.rc;
  if (rc) {
    if (gop.on) drain_second_stream(ctx);   // segments already enqueued: drain before the scratch is reused
    return rc;
  }
  TREC(ctx, ctx->ev[1], s);
  if (!gop.on) {
    rc = grad_pre_chain(g, s);
    if (rc) return rc;
  } else {
    HIPC(ctx, hipStreamWaitEvent(s, ctx->ev_S, 0));   // S = B B' - I and the cleared accumulators: done on the second stream beside the chain
  }
  rc = grad_phase3_operands(g);
  if (rc) return rc;
  // the strips' scratch (the A strip and, beside it, the Kuf strip) and the chunk's moments, sized for every chunk of the call BEFORE
  // anything of the loop is enqueued (ensure_scratch may reallocate)
  int64_t max_strips = 0;
  const size_t wb_max = 2 * chunk_work_bytes(ctx, g.dt, g.Mp, len, g.nc, &max_strips);
  if (max_strips > w->part5_strips) return fail(ctx, SVGP_HIP_ERROR, "internal: strip partial buffer too small");
  rc = ensure_scratch(ctx, wb_max, size_t(g.nc));
  if (rc) return rc;
  // The chunks run one after the other on the main stream.  Measured and not adopted (no longer in the tree): a chunk pipeline with
  // the strips of chunk k + 1 on other streams beside the consumers of chunk k (round 5), and the kernel-gradient reductions on the
  // second stream beside the SYRK (H 97.8-98.3 vs 98.2-98.4 ms: the SYRK's 504 workgroups leave them no room to run).
  for (int64_t c0 = 0; c0 < len; c0 += g.nc) {
    rc = grad_chunk(g, c0);
    if (rc) return rc;
  }
  if (gc.ext_gmu) launch_add_f64(s, w->sums, gc.ext_sum_e);   // sums[0] = sum E: the host's, before any collective
  TREC(ctx, ctx->ev[2], s);
  if (gc.ng_W) {
    launch_natgrad_gather_w(g.dt, s, w->G1.p, g.ns_syrk, g.Mp, gc.ng_W);
    KCHECK(ctx, "natgrad (W in fp64)");
  }
  rc = grad_tail(g);
  if (rc == SVGP_OK && g.centered) rc = grad_centered_chain(g);
  if (rc == SVGP_OK) rc = grad_chol_backward(g);
  if (rc) return rc;
  TREC(ctx, ctx->ev[3], s);
  return SVGP_OK;
}

}  // namespace

namespace svgp {
int grad_enqueue(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, GradCall& gc) {
  const int rc = grad_enqueue_impl(ctx, m, data, off, len, gc);
  if (rc != SVGP_OK && ctx->overlapped) drain_second_stream(ctx);   // a failure anywhere between the fork and the join of the segmented strips
  return rc;
}
}  // namespace svgp

namespace {

// Opening all-reduce of a collective value-and-gradient call: {global batch size, failure flag}, summed over the ranks ON THE DEVICE
// (the strips' phase 3 reads num_data / n_global there).  Asynchronous since round 3: the two values travel as kernel arguments, the
// 16-byte ncclAllReduce is enqueued behind them.  Round 6: it is the ONE collective of the call whose size does not
// depend on the model, so EVERY rank enters it - also one that cannot evaluate at all (NULL model, bad arguments, no memory for the
// gradient workspace): that rank sends {0, 1}, returns its own error and joins nothing else.  The reduced flag comes back through a
// pinned host word behind an event (grad_peers_failed); a healthy rank reads it after it has enqueued its backward pass - by then the
// 16 bytes have long arrived, so the wait costs nothing - and, if any peer failed, SKIPS the closing gradient all-reduce and returns
// SVGP_RCCL_ERROR.  No rank is left inside a collective a peer will never enter, and nothing is aborted.  (Rounds 2-5: the failing rank
// had to match the closing all-reduce with M^2-sized zeros, and without a model - the element counts unknown - it aborted its
// communicator, which does not wake the peers: a documented hang.)
int grad_handshake(svgp_ctx* ctx, GradCall& gc, int64_t len, bool failed) {
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SVGP_HIP_ERROR, "hipSetDevice failed");
  const int rch = ctx->h_open.reserve(ctx, 64, "the opening all-reduce's flag");
  if (rch) return rch;
  HIPC(ctx, ctx->ev_open.create(hipEventDisableTiming));
  launch_set2_f64(ctx->stream, ctx->d_coll.as<double>(), failed ? 0.0 : double(len), failed ? 1.0 : 0.0);
  if (hipGetLastError() != hipSuccess) return fail(ctx, SVGP_HIP_ERROR, "launch failed in the opening all-reduce");
  const int rc = comm_allreduce(ctx, ctx->d_coll.as<double>(), 2, SVGP_F64);
  if (rc != SVGP_OK) return rc;
  *ctx->h_open.as<double>() = -1.0;
  if (hipMemcpyAsync(ctx->h_open.p, ctx->d_coll.as<double>() + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipEventRecord(ctx->ev_open, ctx->stream) != hipSuccess)
    return fail(ctx, SVGP_HIP_ERROR, "read-back of the opening all-reduce's flag failed");
  gc.n_global_dev = ctx->d_coll.as<double>();
  return SVGP_OK;
}
// number of ranks that entered the opening all-reduce with the failure flag (blocks until that all-reduce has completed); < 0: unknown
double grad_peers_failed(svgp_ctx* ctx) {
  if (!ctx->ev_open || hipEventSynchronize(ctx->ev_open) != hipSuccess) return -1.0;
  return *ctx->h_open.as<double>();
}

// A rank of a collective svgp_elbo_grad / svgp_elbo_grad_ext that failed BEFORE anything could be enqueued (argument checks, NULL model,
// workspace allocation): it enters the opening all-reduce with the failure flag - its peers then skip the closing one and return
// SVGP_RCCL_ERROR - and returns its own error.  Only if even that 16-byte collective cannot be issued is the communicator aborted.
int grad_fail_collective(svgp_ctx* ctx, int pre_rc) {
  const std::string keep = ctx->err;
  GradCall gc;
  if (grad_handshake(ctx, gc, 0, true) != SVGP_OK) comm_abort(ctx);
  else (void)hipStreamSynchronize(ctx->stream);
  ctx->err = keep;
  return pre_rc;
}

}  // namespace

namespace svgp {

// the gradient's ONE (grouped) all-reduce; a rank whose enqueue failed still takes part with its failure flag set
int grad_collective(svgp_ctx* ctx, svgp_model* m, GradCall& gc, int local_rc) {
  if (!ctx->comm || !gc.collective) return local_rc;
  GradWs* w = gc.w;
  if (!w) {   // failed before the workspace existed: nothing to reduce with; make the peers fail instead of hang
    comm_abort(ctx);
    return local_rc;
  }
  const std::string keep = ctx->err;
  const int dreg = grad_dreg(m->d);
  if (local_rc != SVGP_OK) {
    std::vector<double> poison(size_t(8 + 1 + dreg), 0.0);
    poison[7] = 1.0;
    if (hipSetDevice(ctx->device) != hipSuccess ||
        hipMemcpyAsync(w->sums, poison.data(), poison.size() * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
      comm_abort(ctx);
      ctx->err = keep;
      return local_rc;
    }
  }
  // {z_bar | m_bar | tril(Lq_bar)}: the lower triangle packed (M (M + 1) / 2 entries instead of M^2: SURVEY 8 f1), one all-reduce in
  // the compute dtype, one in fp64 for the scalars, then unpacked in place
  const int64_t M = m->M, head = M * m->d + M;
  const size_t ncoll = size_t(head) + size_t(M) * size_t(M + 1) / 2;
  if (hipSetDevice(ctx->device) == hipSuccess) launch_pack_tril(m->dtype, ctx->stream, w->gblk.p, w->cblk.p, head, M, 0);
  int rc = comm_group_start(ctx);
  if (rc == SVGP_OK) rc = comm_allreduce(ctx, w->cblk.p, ncoll, m->dtype);
  if (rc == SVGP_OK) rc = comm_allreduce(ctx, w->sums, size_t(8 + 1 + dreg), SVGP_F64);
  const int rce = comm_group_end(ctx);
  if (rc == SVGP_OK) rc = rce;
  // (the reduced block stays packed: grad_finish reads {z_bar | m_bar | packed tril(Lq_bar)} back as it is)
  if (rc == SVGP_OK) gc.packed = true;
  if (rc != SVGP_OK) {
    comm_abort(ctx);
    if (local_rc != SVGP_OK) ctx->err = keep;
    return local_rc != SVGP_OK ? local_rc : rc;
  }
  if (local_rc != SVGP_OK) ctx->err = keep;
  return local_rc;
}

int grad_finish(svgp_ctx* ctx, svgp_model* m, GradCall& gc, double* elbo_out, svgp_terms* terms_out, svgp_grads* g) {
  hipStream_t s = ctx->stream;
  HIPC(ctx, hipSetDevice(ctx->device));
  GradWs* w = gc.w;
  const int dt = m->dtype;
  const int64_t M = m->M;
  const size_t es = m->es;
  const int dreg = grad_dreg(m->d);
  const bool centered = gc.centered;
  // Read back: the fp64 block [sums (8) | scal_out (1 + dreg) | prep scalars (4) | chol_info] and the gradient blocks
  // {z_bar | m_bar | Lq_bar}, contiguous on the device (round 2: seven copies, ~20 us of host latency each).  Lq_bar is M^2 elements -
  // 8.4 MB at M = 1024 f64, 33.5 MB at M = 2048 - and a minibatch step is 1-3 ms of device time: until late in round 4 this went through a
  // fresh std::vector per call (page faults + zero fill), a pageable device-to-host copy and a second host copy into the caller's
  // buffers (M = 2048: 6.6 ms of an 11.7 ms call).  Round 4: a pinned staging buffer kept by the context, the copy issued in up to 8
  // pieces with an event behind each, and the host copy of piece i into the caller's buffers running while piece i + 1 is on the bus.
  // Round 5: Lq_bar is lower triangular, so only its M (M + 1) / 2 entries cross the bus - packed by columns on the
  // device (pack_tril_kernel, the all-reduce's layout) and scattered into the caller's dense column-major M x M array by the host
  // copy, which also writes the zeros above the diagonal.  The C-ABI keeps its dense Lq_bar.
  const size_t nz = size_t(M) * m->d, head = nz + size_t(M), tri = size_t(M) * size_t(M + 1) / 2, nblk = head + tri;
  const size_t f64n = size_t(8 + 1 + dreg + 5), f64b = (f64n * 8 + 255) / 256 * 256, gbytes = nblk * es;
  if (!gc.packed) launch_pack_tril(dt, s, w->gblk.p, w->cblk.p, int64_t(head), M, 0);
  KCHECK(ctx, "pack Lq_bar");
  const int rcs = ctx->hstage.reserve(ctx, f64b + gbytes, "the gradient read-back's staging");
  if (rcs) return rcs;
  for (auto& e : ctx->ev_piece) HIPC(ctx, e.create(hipEventDisableTiming));
  double* f64blk = ctx->hstage.as<double>();
  char* gh = ctx->hstage.as<char>() + f64b;
  HIPC(ctx, hipMemcpyAsync(f64blk, w->sums, f64n * 8, hipMemcpyDeviceToHost, s));
  const int npiece = int(std::min<size_t>(8, std::max<size_t>(1, gbytes >> 20)));   // >= 1 MiB per piece
  const size_t piece = ((gbytes + npiece - 1) / npiece + 255) / 256 * 256;
  for (int q = 0; q < npiece; ++q) {
    const size_t lo = std::min(gbytes, size_t(q) * piece), hi = std::min(gbytes, lo + piece);
    if (hi > lo) HIPC(ctx, hipMemcpyAsync(gh + lo, static_cast<const char*>(w->cblk.p) + lo, hi - lo, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipEventRecord(ctx->ev_piece[q], s));
  }
  struct Dst { size_t lo, hi; void* p; };
  const Dst dst[2] = {{0, nz * es, g->z}, {nz * es, head * es, g->m}};
  int64_t col = 0;   // column of Lq_bar the packed stream has reached (pieces arrive in order)
  for (int q = 0; q < npiece; ++q) {
    HIPC(ctx, hipEventSynchronize(ctx->ev_piece[q]));
    const size_t lo = std::min(gbytes, size_t(q) * piece), hi = std::min(gbytes, lo + piece);
    for (const Dst& d : dst) {
      const size_t a = std::max(lo, d.lo), b = std::min(hi, d.hi);
      if (d.p && b > a) memcpy(static_cast<char*>(d.p) + (a - d.lo), gh + a, b - a);
    }
    // packed entries [e_lo, e_hi) of the triangle (piece boundaries are multiples of 256 bytes, hence of the element size):
    // column c holds the rows c .. M - 1 at st(c) = c M - c (c - 1) / 2; its part above the diagonal is zeroed as the column begins
    if (g->Lq && hi > head * es && hi > lo) {
      const int64_t e_lo = int64_t((std::max(lo, head * es) - head * es) / es), e_hi = int64_t((hi - head * es) / es);
      auto st = [M](int64_t c) { return c * M - c * (c - 1) / 2; };
      char* Lq = static_cast<char*>(g->Lq);
      const char* pk = gh + head * es;
      while (col + 1 < M && st(col + 1) <= e_lo) ++col;
      for (int64_t c = col; c < M && st(c) < e_hi; ++c) {
        const int64_t a = std::max(e_lo, st(c)), b = std::min(e_hi, st(c + 1));
        if (a == st(c) && c > 0) memset(Lq + size_t(c) * size_t(M) * es, 0, size_t(c) * es);
        if (b > a) memcpy(Lq + (size_t(c) * size_t(M) + size_t(c + (a - st(c)))) * es, pk + size_t(a) * es, size_t(b - a) * es);
        col = c;
      }
    }
  }
  HIPC(ctx, hipStreamSynchronize(s));
  const double* sums = f64blk;
  const double* sc = sums + 8;
  PrepScalars ps;
  for (int q = 0; q < 4; ++q) ps.scal[q] = sums[8 + 1 + dreg + q];
  ps.info = int(sums[8 + 1 + dreg + 4]);
  const char* mhost = gh + nz * es;
  finish_prep(m, ps);
  float t01 = 0, t13 = 0;
  (void)elapsed_ms(ctx, &t01, ctx->ev[0], ctx->ev[1]);
  (void)elapsed_ms(ctx, &t13, ctx->ev[1], ctx->ev[3]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_prep = t01;
  ctx->timing.ms_strip = t13;
  ctx->timing.ms_total = t01 + t13;
  float tch = 0;
  (void)elapsed_ms(ctx, &tch, ctx->ev_chol[0], ctx->ev_chol[1]);
  ctx->timing.ms_chol = tch;
  ElboRead r;
  r.E = sums[0]; r.n_neg = sums[4]; r.n_points = sums[5]; r.bad_chol = gc.collective ? sums[6] : 0.0; r.failed = gc.collective ? sums[7] : 0.0;
  // collective: the sums are global; scale = num_data / n_global (as on the device), and the KL counts once
  const double scale = gc.collective ? (gc.num_data > 0 ? gc.num_data / r.n_points : 1.0) : gc.scale;
  const double klw = gc.collective ? 1.0 : gc.klw;
  const double elbo = r.E * scale - klw * m->kl;
  g->variance = sc[0] + sums[2];
  g->lik_sigma2 = sums[3];
  double msum = 0.0;   // Centered: mean_const also enters through m~ = Lk \\ (m - c)
  if (centered)
    for (int64_t i = 0; i < M; ++i) msum += (dt == SVGP_F64) ? reinterpret_cast<const double*>(mhost)[i] : double(reinterpret_cast<const float*>(mhost)[i]);
  g->mean_const = sums[1] - msum;
  if (g->inv_lengthscale)
    for (int f = 0; f < m->d; ++f) g->inv_lengthscale[f] = sc[1 + f];
  fill_terms(terms_out, m, elbo, r, scale);
  const int rc = status_of(ctx, m, r.n_neg, r.bad_chol, r.failed);
  if (elbo_out) *elbo_out = (rc == SVGP_OK) ? elbo : NAN;
  return rc;
}

int elbo_grad_impl(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, const GradRequest& rq,
                   double* elbo_out, svgp_terms* terms_out, svgp_grads* g) {
  const svgp_input_grad* gx = rq.gx;
  const svgp_point_mean_grad* gpm = rq.gpm;
  NatgradCall* ng = rq.ng;
  GradCall gc;
  if (ng) gc.ng_W = ng->c->Wm.as<double>();
  gc.ext_gmu = rq.ext_gmu; gc.ext_gv = rq.ext_gv; gc.ext_sum_e = rq.ext_sum_e;
  gc.gx = gx;
  gc.noise = rq.noise; gc.noise_bar = rq.noise_bar;
  gc.collective = rq.collective && ctx && ctx->comm;
  gc.scale = rq.scale;
  gc.klw = gc.collective ? 1.0 / double(ctx->world) : rq.klw;
  gc.num_data = rq.num_data;
  int rc = check_batch(ctx, m, data, off, len, rq.ext_gmu == nullptr);   // a host-evaluated likelihood needs no y on the device
  if (rc == SVGP_OK && !g) rc = fail(ctx, SVGP_INVALID_ARG, "null gradient output");
  if (rc == SVGP_OK && (!(rq.scale > 0.0) || !(rq.klw >= 0.0))) rc = fail(ctx, SVGP_INVALID_ARG, "scale must be positive and kl_weight non-negative");
  if (rc == SVGP_OK && hipSetDevice(ctx->device) != hipSuccess) rc = fail(ctx, SVGP_HIP_ERROR, "hipSetDevice failed");
  if (rc == SVGP_OK) rc = grad_workspace(ctx, m, len, &gc.w);
  if (rc == SVGP_OK && gx && !gx->on_device) {   // host output: the kernel writes [d][len] on the device, one copy brings it over
    rc = gc.w->xg.reserve(ctx, size_t(m->d) * size_t(len) * m->es, "d elbo / d x");
  }
  if (rc == SVGP_OK && rq.pm) rc = stage_point_mean(ctx, rq.pm, size_t(len) * m->es, &gc.mux);
  if (rc == SVGP_OK && gpm) {   // host destination: point_grad_kernel writes ctx->pm_g, one copy brings it over
    if (gpm->on_device) gc.mux_bar = gpm->mu_bar;
    else if ((rc = ctx->pm_g.reserve(ctx, size_t(len) * m->es, "the prior mean offsets' gradient")) == SVGP_OK) gc.mux_bar = ctx->pm_g.p;
  }
  if (rc != SVGP_OK) return (ctx && gc.collective) ? grad_fail_collective(ctx, rc) : rc;
  if (gc.collective) {
    rc = grad_handshake(ctx, gc, len, false);
    if (rc != SVGP_OK) {   // the opening all-reduce itself could not be issued: nothing sane can follow on this communicator
      comm_abort(ctx);
      return rc;
    }
  }
  rc = grad_enqueue(ctx, m, data, off, len, gc);
  if (rc == SVGP_OK && ng) rc = natgrad_enqueue(ctx, m, gc, *ng);
  if (gc.collective) {
    const double nfail = grad_peers_failed(ctx);
    if (nfail != 0.0) {   // a peer failed before its backward pass (or the flag could not be read): it will not enter the closing all-reduce
      (void)hipStreamSynchronize(ctx->stream);
      if (ctx->overlapped) drain_second_stream(ctx);
      if (nfail < 0.0) { comm_abort(ctx); return rc != SVGP_OK ? rc : fail(ctx, SVGP_RCCL_ERROR, "the opening all-reduce of svgp_elbo_grad did not complete"); }
      return rc != SVGP_OK ? rc : fail(ctx, SVGP_RCCL_ERROR, "a peer rank failed before its backward pass (opening all-reduce of svgp_elbo_grad): the gradient all-reduce was skipped on every rank");
    }
  }
  rc = grad_collective(ctx, m, gc, rc);
  if (rc) return rc;
  if (gx && !gx->on_device)   // (never all-reduced: this rank's points; the stream synchronisation of grad_finish covers the copy)
    HIPC(ctx, hipMemcpy2DAsync(gx->x, size_t(gx->ld) * m->es, gc.w->xg.p, size_t(len) * m->es, size_t(len) * m->es, size_t(m->d),
                               hipMemcpyDeviceToHost, ctx->stream));
  if (gpm && !gpm->on_device)   // (never all-reduced either)
    HIPC(ctx, hipMemcpyAsync(gpm->mu_bar, ctx->pm_g.p, size_t(len) * m->es, hipMemcpyDeviceToHost, ctx->stream));
  rc = grad_finish(ctx, m, gc, elbo_out, terms_out, g);
  if (rc == SVGP_OK && ng) rc = natgrad_finish(ctx, m, *ng);
  return rc;
}

// argument checks of the `_inputs` calls (before anything is enqueued; a NULL or inconsistent data handle is check_batch's to report)
int check_input_grad(svgp_ctx* ctx, const svgp_data* data, int64_t len, const svgp_input_grad* gx) {
  if (!gx || !gx->x) return fail(ctx, SVGP_INVALID_ARG, "null input-gradient output");
  if (gx->ld < len) return fail(ctx, SVGP_INVALID_ARG, "input-gradient leading dimension smaller than the batch");
  if ((gx->on_device != 0 && gx->on_device != 1) || gx->reserved != 0)
    return fail(ctx, SVGP_INVALID_ARG, "input-gradient on_device must be 0 or 1 and reserved 0");
  if (gx->on_device && data && data->x.p && len >= 1 && data->d >= 1) {
    const size_t es = data->dtype == SVGP_F64 ? 8 : 4;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(gx->x), a1 = a0 + (size_t(data->d - 1) * size_t(gx->ld) + size_t(len)) * es;
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(data->x.p), b1 = b0 + (size_t(data->d - 1) * size_t(data->ldx) + size_t(data->n)) * es;
    if (a0 < b1 && b0 < a1) return fail(ctx, SVGP_INVALID_ARG, "input-gradient output overlaps the data's x");
  }
  return SVGP_OK;
}

}  // namespace svgp

namespace {
// the request of the collective entry points: scale = num_data / len (num_data <= 0: 1), the whole KL
GradRequest batch_request(int64_t len, double num_data) {
  GradRequest rq;
  rq.scale = len >= 1 ? (num_data > 0 ? num_data : double(len)) / double(len) : 1.0;   // len < 1 fails check_batch
  rq.num_data = num_data;
  rq.collective = true;
  return rq;
}
// ... with the point gradients of a host-evaluated likelihood
GradRequest ext_request(int64_t len, double num_data, double sum_e, const double* g_mu, const double* g_v) {
  GradRequest rq = batch_request(len, num_data);
  rq.ext_gmu = g_mu; rq.ext_gv = g_v; rq.ext_sum_e = sum_e;
  return rq;
}
}  // namespace

// With a communicator attached this call is COLLECTIVE like svgp_elbo: value and gradient of the GLOBAL minibatch ELBO on
// every rank (one 8-byte all-reduce of the batch size up front, one grouped all-reduce of the gradient at the end).
extern "C" int32_t svgp_elbo_grad(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                  double num_data, double* elbo_out, svgp_terms* terms_out, svgp_grads* g) {
  if (!ctx) return SVGP_INVALID_ARG;
  return elbo_grad_impl(ctx, m, data, off, len, batch_request(len, num_data), elbo_out, terms_out, g);
}

// always local (no collective): the building block for hosts that run their own all-reduce
extern "C" int32_t svgp_elbo_grad_shard(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                        double scale, double kl_weight, double* value_out, svgp_terms* terms_out,
                                        svgp_grads* g) {
  GradRequest rq;
  rq.scale = scale;
  rq.klw = kl_weight;
  return elbo_grad_impl(ctx, m, data, off, len, rq, value_out, terms_out, g);
}

// Value and gradient of  scale sum_e - kl_weight KL  with (dE_i/dmu_i, dE_i/dv_i) = (g_mu[i], g_v[i]) supplied by the host
// (fp64, unscaled, one per point of the batch), scale = num_data / len.  Everything else - outputs, statuses, the collective
// form on a context with a communicator (sum_e and the gradients are then this rank's shard's) - is svgp_elbo_grad's;
// grads->lik_sigma2 is 0 (the likelihood's own parameters are the host's).
extern "C" int32_t svgp_elbo_grad_ext(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                      double num_data, double sum_e, const double* g_mu, const double* g_v,
                                      double* elbo_out, svgp_terms* terms_out, svgp_grads* g) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!g_mu || !g_v) {
    const int rc = fail(ctx, SVGP_INVALID_ARG, "null point gradients");
    return ctx->comm ? grad_fail_collective(ctx, rc) : rc;   // the peers learn it from the opening all-reduce: they return SVGP_RCCL_ERROR
  }
  return elbo_grad_impl(ctx, m, data, off, len, ext_request(len, num_data, sum_e, g_mu, g_v), elbo_out, terms_out, g);
}

// svgp_elbo_grad / svgp_elbo_grad_ext + d elbo / d x (include/svgp_mi355x.h): the same launches, plus one xgrad_mfma_kernel per gradient chunk
extern "C" int32_t svgp_elbo_grad_inputs(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                         double num_data, double* elbo_out, svgp_terms* terms_out, svgp_grads* g,
                                         const svgp_input_grad* gx) {
  if (!ctx) return SVGP_INVALID_ARG;
  const int rc = check_input_grad(ctx, data, len, gx);
  if (rc) return ctx->comm ? grad_fail_collective(ctx, rc) : rc;
  GradRequest rq = batch_request(len, num_data);
  rq.gx = gx;
  return elbo_grad_impl(ctx, m, data, off, len, rq, elbo_out, terms_out, g);
}

extern "C" int32_t svgp_elbo_grad_ext_inputs(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                             double num_data, double sum_e, const double* g_mu, const double* g_v,
                                             double* elbo_out, svgp_terms* terms_out, svgp_grads* g, const svgp_input_grad* gx) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = (!g_mu || !g_v) ? fail(ctx, SVGP_INVALID_ARG, "null point gradients") : SVGP_OK;
  if (rc == SVGP_OK) rc = check_input_grad(ctx, data, len, gx);
  if (rc) return ctx->comm ? grad_fail_collective(ctx, rc) : rc;
  GradRequest rq = ext_request(len, num_data, sum_e, g_mu, g_v);
  rq.gx = gx;
  return elbo_grad_impl(ctx, m, data, off, len, rq, elbo_out, terms_out, g);
}

namespace svgp {
// argument checks of the prior mean offsets' gradient output (before anything is enqueued)
int check_point_mean_grad(svgp_ctx* ctx, const svgp_data* data, int64_t len, const svgp_input_grad* gx, const svgp_point_mean_grad* gpm) {
  if (!gpm) return SVGP_OK;
  if (!gpm->mu_bar) return fail(ctx, SVGP_INVALID_ARG, "null prior-mean gradient output");
  if ((gpm->on_device != 0 && gpm->on_device != 1) || gpm->reserved != 0)
    return fail(ctx, SVGP_INVALID_ARG, "prior-mean gradient: on_device must be 0 or 1 and reserved 0");
  if (gpm->on_device && data && len >= 1) {
    const size_t es = data->dtype == SVGP_F64 ? 8 : 4;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(gpm->mu_bar), a1 = a0 + size_t(len) * es;
    auto hits = [&](const void* p, size_t bytes) {
      const uintptr_t b0 = reinterpret_cast<uintptr_t>(p), b1 = b0 + bytes;
      return p && a0 < b1 && b0 < a1;
    };
    if (data->d >= 1 && hits(data->x.p, (size_t(data->d - 1) * size_t(data->ldx) + size_t(data->n)) * es))
      return fail(ctx, SVGP_INVALID_ARG, "prior-mean gradient output overlaps the data's x");
    if (hits(data->y.p, size_t(data->n) * es)) return fail(ctx, SVGP_INVALID_ARG, "prior-mean gradient output overlaps the data's y");
    if (gx && gx->on_device && data->d >= 1 && hits(gx->x, (size_t(data->d - 1) * size_t(gx->ld) + size_t(len)) * es))
      return fail(ctx, SVGP_INVALID_ARG, "prior-mean gradient output overlaps the input-gradient output");
  }
  return SVGP_OK;
}
}  // namespace svgp

// svgp_elbo_grad / _ext / _inputs / _ext_inputs with the batch's prior mean offsets (include/svgp_mi355x.h): the same launches; the
// offsets enter the strips' moment epilogue, and their gradient is a second store of point_grad_kernel's g_mu
extern "C" int32_t svgp_elbo_grad_with_mean(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                            double num_data, const svgp_point_mean* pm, double sum_e, const double* g_mu,
                                            const double* g_v, double* elbo_out, svgp_terms* terms_out, svgp_grads* g,
                                            const svgp_input_grad* gx, svgp_point_mean_grad* gpm) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = ((g_mu == nullptr) != (g_v == nullptr)) ? fail(ctx, SVGP_INVALID_ARG, "exactly one of g_mu / g_v is NULL") : SVGP_OK;
  if (rc == SVGP_OK && gx) rc = check_input_grad(ctx, data, len, gx);
  if (rc == SVGP_OK) rc = check_point_mean(ctx, pm);
  if (rc == SVGP_OK) rc = check_point_mean_grad(ctx, data, len, gx, gpm);
  if (rc) return ctx->comm ? grad_fail_collective(ctx, rc) : rc;
  GradRequest rq = ext_request(len, num_data, g_mu ? sum_e : 0.0, g_mu, g_v);
  rq.gx = gx;
  rq.pm = pm;
  rq.gpm = gpm;
  return elbo_grad_impl(ctx, m, data, off, len, rq, elbo_out, terms_out, g);
}

// mean(fz) = mean_const + muz: a model-owned copy (include/svgp_mi355x.h); the next evaluation prepares the model again
extern "C" int32_t svgp_model_set_mean_z(svgp_ctx* ctx, svgp_model* m, const void* mu_z) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!m) return fail(ctx, SVGP_INVALID_ARG, "null model");
  HIPC(ctx, hipSetDevice(ctx->device));
  if (!mu_z) {
    if (m->mu_z.p) {
      HIPC(ctx, hipStreamSynchronize(ctx->stream));
      m->mu_z.release();
    }
  } else {
    const int rc = m->mu_z.reserve(ctx, size_t(m->M) * m->es, "the inducing points' prior mean offsets");
    if (rc) return rc;
    HIPC(ctx, hipMemcpyAsync(m->mu_z.p, mu_z, size_t(m->M) * m->es, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));   // the host buffer may be released by the caller
  }
  m->prepared = false;
  return SVGP_OK;
}
