// api_forward.hip — the forward schedule of the C-ABI: the M-sized prep, the strips (one launch, two launches, or segmented beside
// the factorisation), the expectation, and the calls built on them: svgp_elbo*, svgp_marginals*, svgp_predict*, svgp_posterior,
// svgp_prior_kl, svgp_kuf.  Host orchestration only (prep.hip / strip.hip hold the kernels).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <memory>
#include <string>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"
#include "lik.hpp"

using namespace svgp;

namespace {

// Gaussian sigma^2 / Gamma shape alpha; 1 for the parameter-free likelihoods
double lik_param(const svgp_model_desc& d) {
  return (d.likelihood == SVGP_LIK_GAUSSIAN || d.likelihood == SVGP_LIK_GAMMA_EXP) ? d.lik_sigma2 : 1.0;
}

}  // namespace

namespace svgp {

KernelParams kparams(const svgp_model* m) {
  KernelParams kp;
  kp.family = m->desc.kernel;
  kp.d = m->d;
  kp.variance = m->desc.variance;
  kp.invl = m->invl.p;
  return kp;
}

LikParams lik_params(const svgp_model* m) {
  LikParams lp{};
  lp.lik = m->desc.likelihood;
  lp.gh_n = m->gh_n;
  lp.sigma2 = lik_param(m->desc);
  lp.digamma_alpha = m->desc.likelihood == SVGP_LIK_GAMMA_EXP ? digamma_d(m->desc.lik_sigma2) : 0.0;
  lp.gh_x = m->gh_x.as<double>();
  lp.gh_w = m->gh_w.as<double>();
  lp.clamp_neg_var = (m->desc.neg_var_policy == SVGP_NEGVAR_CLAMP);
  lp.mean_const = m->desc.mean_const;
  return lp;
}

// The M-sized work of posterior(sva): enqueue only, no sync.
// overlap (NonCentered only): everything the strips need besides T - the scaled inducing inputs, U = Lq', the padded mean - is
// enqueued FIRST and ctx->ev_fork recorded behind it; the factorisation then records ctx->ev_row[p] as block row p of T becomes
// final, so that strips on a second stream can run beside it (SegRun: seg_enqueue_row).
int enqueue_prep(svgp_ctx* ctx, svgp_model* m, bool overlap, const RowHook* hook) {
  hipStream_t s = ctx->stream;
  const KernelParams kp = kparams(m);
  HIPC(ctx, hipMemsetAsync(m->info.as<int>(), 0, info_bytes(m->Mp), s));   // info + the factorisation's hand-over counters and flags
  launch_scale_inputs(m->dtype, s, m->z_raw.p, m->desc.layout_z, m->d, m->M, m->Mp, m->invl.p, m->zs.p);
  KCHECK(ctx, "scale_inputs");
  if (overlap) {
    launch_pack_q(m->dtype, s, m->Lq_raw.p, m->m_raw.p, m->M, m->Mp, m->U.p, m->mp.p);          // B = Lq      SVA:183-184
    KCHECK(ctx, "pack_q");
    HIPC(ctx, hipEventRecord(ctx->ev_fork, s));
    TREC(ctx, ctx->ev_ov[0], s);
    if (hook && hook->fn) hook->fn(hook->user, -1);   // the strips' pre-generation: behind the fork, before the chain is enqueued
  }
  launch_kuu(m->dtype, s, kp, m->zs.p, m->M, m->Mp, m->desc.jitter, m->L.p);
  KCHECK(ctx, "kuu");
  TREC(ctx, ctx->ev_chol[0], s);
  hipEvent_t rows[16] = {};   // the row events as the plain handles launch_potrf takes
  if (overlap) std::copy(std::begin(ctx->ev_row), std::end(ctx->ev_row), rows);
  launch_potrf(m->dtype, s, m->L.p, m->T.p, m->Mp, m->info.as<int>(), reinterpret_cast<unsigned*>(m->info.as<int>() + 1), ctx->num_cus, overlap ? rows : nullptr,
               overlap ? hook : nullptr);   // T panels included
  KCHECK(ctx, "potrf");
  TREC(ctx, ctx->ev_chol[1], s);
  if (overlap) {
    launch_kl_terms(m->dtype, s, m->Lq_raw.p, m->m_raw.p, m->L.p, m->M, m->Mp, m->scal.as<double>());        // SVA:364-373
  } else if (m->desc.parametrization == SVGP_NONCENTERED) {
    launch_pack_q(m->dtype, s, m->Lq_raw.p, m->m_raw.p, m->M, m->Mp, m->U.p, m->mp.p);          // B = Lq      SVA:183-184
    launch_kl_terms(m->dtype, s, m->Lq_raw.p, m->m_raw.p, m->L.p, m->M, m->Mp, m->scal.as<double>());        // SVA:364-373
  } else {
    // Centered (SVA:115-136): B = Lk \ Lq, whitened mean m~ = Lk \ (m - mean(fz)); then α = Lk' \ m~ = Kuu \ (m - μ)
    // and KL(q || p(u)) = ½(ΣB² + m~'m~ − M − logdet(BB')) — the NonCentered expression evaluated at (m~, B).
    launch_pad_lower(m->dtype, s, m->Lq_raw.p, m->M, m->Mp, m->B.p);
    launch_trsm_mat(m->dtype, s, m->T.p, m->Mp, m->B.p);
    if (m->mu_z.p)   // mean(fz) = mean_const + muz (svgp_model_set_mean_z)
      launch_shift_sub_vec(m->dtype, s, m->m_raw.p, -m->desc.mean_const, m->mu_z.p, m->M, m->Mp, m->mp.p);
    else
      launch_shift_vec(m->dtype, s, m->m_raw.p, -m->desc.mean_const, m->M, m->Mp, m->mp.p);
    launch_trsv2(m->dtype, s, m->L.p, m->T.p, m->Mp, 0, m->mp.p);
    launch_pack_q_ld(m->dtype, s, m->B.p, m->Mp, nullptr, m->Mp, m->Mp, m->U.p, nullptr);
    launch_kl_terms_ld(m->dtype, s, m->B.p, m->Mp, m->mp.p, m->L.p, m->M, m->Mp, m->scal.as<double>());
  }
  KCHECK(ctx, "pack_q/kl");
  return SVGP_OK;
}

void finish_prep(svgp_model* m, const PrepScalars& ps) {
  m->chol_info = ps.info;
  m->kl = 0.5 * (ps.scal[0] + ps.scal[1] - double(m->M) - 2.0 * ps.scal[2]);
  m->logdet_kuu = 2.0 * ps.scal[3];
  m->prepared = (ps.info == 0);
}

int ensure_scratch(svgp_ctx* ctx, size_t work_bytes, size_t npoints) {
  const int rc = ctx->work.reserve(ctx, work_bytes, "the strips' scratch");
  return rc ? rc : ctx->mom.reserve(ctx, 2 * npoints * sizeof(double), "the moments");
}

}  // namespace svgp

namespace {

// second stream (+ fork / join events, its own strip queue head) for launches that run BESIDE the main stream's
int ensure_stream2(svgp_ctx* ctx) {
  if (ctx->counter2.p) return SVGP_OK;   // made last: a call that failed half-way is completed by the next one
  // the second stream carries work that runs BESIDE the main stream's (the ragged tail of a large batch, the segmented strips beside
  // the factorisation): lowest priority, so that where both have workgroups to dispatch the main stream's serial chain goes first
  static const int prio_knob = exp_int("SVGP_STREAM2_LOW_PRIO", 1);   // A/B knob (experiments build)
  int least = 0, greatest = 0;
  if (!ctx->stream2) {
    const bool low = prio_knob && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest;
    HIPC(ctx, low ? ctx->stream2.create(hipStreamNonBlocking, least) : ctx->stream2.create(hipStreamNonBlocking));
  }
  HIPC(ctx, ctx->ev_fork.create(kSyncEvent));
  HIPC(ctx, ctx->ev_join.create(kSyncEvent));
  HIPC(ctx, ctx->counter2.alloc(64));
  return SVGP_OK;
}

// split closing launch of small batches (kernels.hpp: seg_split): at most kSegSplitSlots workgroups, each leaving 3 x NT <= 384 doubles;
// then one counter per strip
constexpr size_t kSegSplitSlots = 512, kSegSplitPart = 384, kSegSplitDoubles = kSegSplitSlots * kSegSplitPart + kSegSplitSlots;

}  // namespace

namespace svgp {

// S = the largest power of two with S <= nP and nstrips S <= kSegSplitSlots - if that is at least 4: two workgroups per strip do not
// pay for the extra launch (measured, profiles/round4/minibatch_step.md: 8192 points / M = 1024 f64 forward 0.84 -> 0.87 ms, gradient
// 2.29 -> 2.28; 4096 points 0.81 -> 0.78 / 2.13 -> 2.00; 1024 points 0.80 -> 0.71 / 2.05 -> 1.78).  SVGP_SEG_SPLIT=0 (at context creation): never split
int seg_split_factor(const svgp_ctx* ctx, int nP, int64_t nstrips) {
  int S = 1;
  if (ctx->kn.seg_split)
    while (2 * S <= nP && int64_t(2 * S) * nstrips <= int64_t(kSegSplitSlots)) S *= 2;
  return S >= 4 ? S : 1;
}
// points the split closing launch at its partials and counters (behind the saved sums) and zeroes the counters on the second stream
int seg_split_setup(svgp_ctx* ctx, StripArgs& a, int S, int64_t nstrips) {
  double* extra = ctx->seg_state.as<double>() + (ctx->seg_state.cap / sizeof(double) - kSegSplitDoubles);
  a.seg_split = S;
  a.seg_part = extra;
  a.seg_cnt = reinterpret_cast<unsigned*>(extra + kSegSplitSlots * kSegSplitPart);
  HIPC(ctx, hipMemsetAsync(a.seg_cnt, 0, size_t(nstrips) * sizeof(unsigned), ctx->stream2));
  return SVGP_OK;
}
int ensure_overlap(svgp_ctx* ctx, size_t state_doubles) {
  int rc = ensure_stream2(ctx);
  if (rc) return rc;
  if (!ctx->ev_row_ready) {
    for (auto& e : ctx->ev_row) HIPC(ctx, e.create(kSyncEvent));
    for (auto& e : ctx->ev_ov) HIPC(ctx, e.create(kTimingEvent));
    HIPC(ctx, ctx->ev_R.create(kSyncEvent));
    HIPC(ctx, ctx->ev_S.create(kSyncEvent));
    ctx->ev_row_ready = true;
  }
  state_doubles += kSegSplitDoubles;   // behind the saved sums: the split closing launch's partials and its per-strip counters
  return ctx->seg_state.reserve(ctx, state_doubles * sizeof(double), "the segmented strips' saved sums");
}

void drain_second_stream(svgp_ctx* ctx) {
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
}

// (launch_trsm_point_major - the collapsed bound - reads T, zs, x, work, counter, mom_var, At_out and the shape only: strip.hip)
StripArgs strip_args(const svgp_ctx* ctx, const svgp_model* m, const void* x, int64_t ldx, int64_t off, int64_t len) {
  StripArgs a{};
  a.T = m->T.p; a.U = m->U.p; a.zs = m->zs.p; a.mp = m->mp.p; a.x = x;
  a.work = ctx->work.p; a.counter = ctx->counter.as<unsigned>();
  a.mom_mu = ctx->mom_mu(); a.mom_var = ctx->mom_var();
  a.ldx = ldx; a.off = off; a.len = len; a.Mp = m->Mp; a.M = m->M; a.kp = kparams(m);
  a.mean_const = m->desc.mean_const;
  return a;
}

SinglePlan single_plan(int dtype, int64_t Mp, int64_t len, int num_cus) {
  const StripPlan plan = strip_plan_single(dtype, Mp, len, num_cus);
  SinglePlan p;
  p.nt = plan.grid ? plan.nt : plan.nt_tail;
  p.grid = plan.grid ? plan.grid : plan.grid_tail;
  p.nstrips = plan.grid ? plan.nstrips : plan.nstrips_tail;
  return p;
}

size_t chunk_work_bytes(const svgp_ctx* ctx, int dtype, int64_t Mp, int64_t len, int64_t nc, int64_t* max_strips) {
  size_t wb_max = 0;
  int64_t ns_max = 0;
  const int64_t nchunks = (len + nc - 1) / nc;
  for (int64_t clen : {std::min(len, nc), len - (nchunks - 1) * nc}) {
    const SinglePlan p = single_plan(dtype, Mp, clen, ctx->num_cus);
    wb_max = std::max(wb_max, strip_work_bytes(dtype, Mp, p.nt, p.grid));
    ns_max = std::max(ns_max, p.nstrips);
  }
  if (max_strips) *max_strips = ns_max;
  return wb_max;
}

}  // namespace svgp

namespace {

struct StripOuts {
  void* mu = nullptr;
  void* var = nullptr;
  void* A = nullptr;
  void* C = nullptr;
  void* At = nullptr;
  void* Ct = nullptr;
  int64_t lda = 0;
  bool skip_expect = false;   // svgp_marginals: the caller wants the moments themselves
  const void* mux = nullptr;  // the batch's prior mean offsets (device, data dtype; svgp_*_with_mean)
};

// the expectation over the moments of points [off, off + len) + the final reduce, on the main stream (both forward routes)
int enqueue_expect(svgp_ctx* ctx, svgp_model* m, const void* y, int64_t off, int64_t len, void* mu_out, void* var_out) {
  hipStream_t s = ctx->stream;
  launch_expect(m->dtype, s, lik_params(m), ctx->mom_mu(), ctx->mom_var(), y, off, len, ctx->partial.as<double>(), ctx->negcnt.as<unsigned>(), mu_out, var_out);
  KCHECK(ctx, "expect");
  launch_final_reduce(s, ctx->partial.as<double>(), ctx->negcnt.as<unsigned>(), expect_blocks(len), m->info.as<int>(), double(len), ctx->d_res.as<double>(), m->scal.as<double>());
  KCHECK(ctx, "final_reduce");
  HIPC(ctx, hipGetLastError());
  return SVGP_OK;
}

// enqueue the fused strip kernel + final reduce over points [off, off+len) of (x, y)
int enqueue_strips(svgp_ctx* ctx, svgp_model* m, const void* x, int64_t ldx, const void* y, int64_t off, int64_t len,
                   const StripOuts& o) {
  StripPlan plan = strip_plan(m->dtype, m->Mp, len, ctx->num_cus);
  if (plan.concurrent_tail && (o.A || o.C || o.At || o.Ct)) plan = strip_plan_single(m->dtype, m->Mp, len, ctx->num_cus);
  const size_t wb_main = plan.grid ? strip_work_bytes(m->dtype, m->Mp, plan.nt, plan.grid) : 0;
  const size_t wb_tail = plan.nt_tail ? strip_work_bytes(m->dtype, m->Mp, plan.nt_tail, plan.grid_tail) : 0;
  int rc = ensure_scratch(ctx, plan.concurrent_tail ? wb_main : (wb_main > wb_tail ? wb_main : wb_tail), size_t(len));
  if (rc) return rc;
  if (plan.concurrent_tail) {
    rc = ensure_stream2(ctx);
    if (rc) return rc;
    rc = ctx->work2.reserve(ctx, wb_tail, "the concurrent tail's scratch");
    if (rc) return rc;
  }
  StripArgs a = strip_args(ctx, m, x, ldx, off, len);
  a.A_out = o.A;
  a.C_out = o.C;
  a.At_out = o.At;
  a.Ct_out = o.Ct;
  a.lda = o.lda;
  a.mux = o.mux;
  if (plan.concurrent_tail) HIPC(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
  if (plan.grid) {
    StripArgs am = a;
    am.len = plan.points;
    HIPC(ctx, hipMemsetAsync(ctx->counter.as<unsigned>(), 0, sizeof(unsigned), ctx->stream));
    launch_strip(m->dtype, ctx->stream, am, plan.nt, plan.grid, plan.nstrips);
    KCHECK(ctx, "strip");
  }
  if (plan.nt_tail) {   // remaining points as half-width strips: same arithmetic per point, outputs shifted by plan.points
    StripArgs at = a;
    const int64_t sh = plan.points;
    const size_t es = m->es;
    at.off = off + sh;
    at.len = len - sh;
    at.mom_mu = a.mom_mu + sh;
    at.mom_var = a.mom_var + sh;
    if (a.mux) at.mux = static_cast<const char*>(a.mux) + size_t(sh) * es;
    if (a.A_out) at.A_out = static_cast<char*>(a.A_out) + size_t(sh) * es;
    if (a.C_out) at.C_out = static_cast<char*>(a.C_out) + size_t(sh) * es;
    if (a.At_out) at.At_out = static_cast<char*>(a.At_out) + size_t(sh) * size_t(m->Mp) * es;
    if (a.Ct_out) at.Ct_out = static_cast<char*>(a.Ct_out) + size_t(sh) * size_t(m->Mp) * es;
    if (plan.concurrent_tail) {
      // fork: the tail may start as soon as everything before this point on the main stream is done (the prep kernels,
      // recorded BEFORE the main launch); join: the main stream continues after both launches
      at.work = ctx->work2.p;
      at.counter = ctx->counter2.as<unsigned>();
      HIPC(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
      HIPC(ctx, hipMemsetAsync(ctx->counter2.as<unsigned>(), 0, sizeof(unsigned), ctx->stream2));
      launch_strip(m->dtype, ctx->stream2, at, plan.nt_tail, plan.grid_tail, plan.nstrips_tail);
      KCHECK(ctx, "strip tail (concurrent)");
      HIPC(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
      HIPC(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    } else {
      HIPC(ctx, hipMemsetAsync(ctx->counter.as<unsigned>(), 0, sizeof(unsigned), ctx->stream));
      launch_strip(m->dtype, ctx->stream, at, plan.nt_tail, plan.grid_tail, plan.nstrips_tail);
      KCHECK(ctx, "strip tail");
    }
  }
  ctx->timing.strip_launches = (plan.grid ? 1 : 0) + (plan.nt_tail ? 1 : 0);
  TREC(ctx, ctx->ev[2], ctx->stream);
  if (o.skip_expect) return SVGP_OK;
  return enqueue_expect(ctx, m, y, off, len, o.mu, o.var);
}

}  // namespace

namespace svgp {

// ---- prep beside the strips (round 4) --------------------------------------------------------------------
// The M-sized prep is a serial chain of ~2 nP launches (0.43 ms at M = 1024 whatever the batch) and minibatches are where real
// callers live.  Phase 1 of panel I needs only block row I of T, final after panel step I of the factorisation.  For a batch of
// at most one round of strips the evaluation therefore runs as SEGMENTED strips (strip.hip: SEG) on the second stream: the Kuf
// pre-generation right away, phase-1 panel I behind ev_row[I], phase 2 with the last panel; the main stream joins before the
// expectation.  Nothing spins and no launch waits while resident, so the factorisation's launches always find free CUs.
OverlapPlan overlap_plan(const svgp_ctx* ctx, const svgp_model* m, int64_t len) {
  OverlapPlan p;
  if (!ctx->kn.overlap) return p;   // SVGP_OVERLAP=0 at context creation
  const int nP = int(m->Mp / 128);
  // measured (profiles/round4/overlap.md, f64, one round of strips): M = 256 +5 %, 512 0..-4 %, 1024 -9..-11 %, 2048 -19 %: the
  // 2 nP extra launches and the chain's slowdown beside the strips are paid back from about six panels on
  const int min_panels = ctx->kn.overlap_min_panels;   // 5 (SVGP_OVERLAP_MIN_PANELS in the experiments build)
  if (m->desc.parametrization != SVGP_NONCENTERED || m->d > 16 || nP < 2 || nP > potrf_max_row_events()) return p;
  // (every caller leaves the strips' A / C outputs unset; the single-launch plan is one launch: SinglePlan)
  const SinglePlan sp = single_plan(m->dtype, m->Mp, len, ctx->num_cus);
  p.nt = sp.nt;
  p.nstrips = sp.nstrips;
  p.grid = sp.grid;
  // More than one round of strips (C5: 4, C2: 3) does not overlap.  Measured and not adopted (round 4, profiles/round4/overlap.md;
  // no longer in the tree): a SEGMENTED HEAD - the first round beside the factorisation, the rest behind the prep - C5 5.02 -> 4.91 ms,
  // C2 / H32 / C3 unchanged: the head's long panel launches hold the CUs the factorisation waits for (C5 prep 0.48 -> 0.84 ms).
  if (p.nstrips > p.grid) return OverlapPlan{};
  if (nP < min_panels) return p;   // one round: pays from about five panels on
  p.on = true;
  return p;
}

}  // namespace svgp

namespace {

// row -1: the Kuf pre-generation (behind ev_fork); row I >= 0: phase-1 panel I (behind ev_row[I]); the forward's last panel carries
// phase 2, the gradient's closing launch (phase 2 + 3, behind ev_R) is enqueued by grad_enqueue_impl
int seg_enqueue_row(SegRun& r, int row) {
  svgp_ctx* ctx = r.ctx;
  hipStream_t s2 = ctx->stream2;
  StripArgs& a = r.a;
  const int dt = r.m->dtype;
  if (row < 0) {
    HIPC(ctx, hipStreamWaitEvent(s2, ctx->ev_fork, 0));
    a.seg_flags = kSegPregen; a.seg_lo = 0; a.seg_hi = 0;
    launch_strip_seg(dt, s2, a, r.op.nt, r.op.grid, r.op.nstrips, r.grad);
    KCHECK(ctx, "strip (segmented: pre-generation)");
    return SVGP_OK;
  }
  const int I = row, nP = r.nP;
  HIPC(ctx, hipStreamWaitEvent(s2, ctx->ev_row[I], 0));
  a.seg_lo = I; a.seg_hi = I + 1;
  a.seg_flags = (I > 0 ? kSegLoad : 0) | ((r.grad || r.split > 1 || I + 1 < nP) ? kSegStore : kSegPhase2);
  launch_strip_seg(dt, s2, a, r.op.nt, r.op.grid, r.op.nstrips, r.grad);
  KCHECK(ctx, "strip (segmented: panel)");
  if (I == 0) TREC(ctx, ctx->ev_ov[1], s2);
  // The gradient's chain-independent prep goes behind the strips of panel 1: its ~10 launches are ~55 us of HOST time, and enqueued
  // any earlier (it sat in front of the pre-generation at first) they kept the host from enqueueing the factorisation's first launches -
  // the main stream idled for 45 us waiting for its Kuu kernel (kernel trace, profiles/round4/minibatch_step.md section 7)
  if (I == 1 && r.pre) {
    const int rcp = r.pre(r.pre_user);
    if (rcp) return rcp;
  }
  return SVGP_OK;
}

}  // namespace

namespace svgp {

void seg_row_hook(void* user, int row) {
  SegRun& r = *static_cast<SegRun*>(user);
  if (r.rc == SVGP_OK) r.rc = seg_enqueue_row(r, row);
}

}  // namespace svgp

namespace {

// forward evaluation, stage 1 (BEFORE the prep is enqueued): every allocation and the strips' arguments
int seg_prepare_forward(svgp_ctx* ctx, svgp_model* m, const void* x, int64_t ldx, int64_t off, int64_t len, const OverlapPlan& op, SegRun& r) {
  const int nP = int(m->Mp / 128);
  // the segmented strips' scratch is per STRIP (the one-launch kernel's is per workgroup): a buffer of its own
  const size_t wb1 = strip_work_bytes(m->dtype, m->Mp, op.nt, int(op.nstrips)), wb = wb1;
  // (A checkpointed phase 2 beside the factorisation - bitwise-tested, measured in round 4, profiles/round4/overlap.md: the factorisation
  // slows by what the strips' extra work beside it occupies, 16 384 / 1024 f64 1.046 -> 1.06-1.07 ms, M = 2048 1.94 -> 2.11 - left the
  // tree in round 6.)
  int rc = ctx->work_seg.reserve(ctx, wb, "the segmented strips' scratch");
  if (rc == SVGP_OK) rc = ensure_scratch(ctx, 0, size_t(len));
  if (rc) return rc;
  r.ctx = ctx; r.m = m; r.op = op; r.grad = false; r.nP = nP; r.wb1 = wb1;
  // A small batch (fewer strips than workgroup slots): phase 2 - one panel C_J after the other inside a strip's
  // workgroup - is latency-bound on the few CUs it reaches, and its panels are independent: a closing launch with S workgroups per strip
  r.split = seg_split_factor(ctx, nP, op.nstrips);
  r.a = strip_args(ctx, m, x, ldx, off, len);
  r.a.work = ctx->work_seg.p;
  r.a.counter = ctx->counter2.as<unsigned>();
  r.a.seg_state = ctx->seg_state.as<double>();
  return SVGP_OK;
}

// forward evaluation, stage 2 (AFTER the prep, whose launch loop enqueued the segments): the join, the expectation
int seg_finish_forward(svgp_ctx* ctx, svgp_model* m, const void* y, int64_t off, int64_t len, const StripOuts& o, SegRun& r) {
  hipStream_t s = ctx->stream, s2 = ctx->stream2;
  if (r.rc) return r.rc;
  int launches = r.nP + 1;
  if (r.split > 1) {   // phase 2 + moments, r.split workgroups per strip
    StripArgs& a = r.a;
    const int rcs = seg_split_setup(ctx, a, r.split, r.op.nstrips);
    if (rcs) return rcs;
    a.seg_lo = a.seg_hi = r.nP;
    a.seg_flags = kSegLoad | kSegPhase2;
    launch_strip_seg(m->dtype, s2, a, r.op.nt, int(r.op.nstrips) * r.split, r.op.nstrips, false);
    KCHECK(ctx, "strip (segmented: split phase 2)");
    ++launches;
  }
  HIPC(ctx, hipEventRecord(ctx->ev_join, s2));
  HIPC(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
  TREC(ctx, ctx->ev[2], s);
  ctx->timing.strip_launches = launches;
  if (o.skip_expect) return SVGP_OK;
  return enqueue_expect(ctx, m, y, off, len, o.mu, o.var);
}

}  // namespace

namespace svgp {

int check_batch(svgp_ctx* ctx, const svgp_model* m, const svgp_data* data, int64_t off, int64_t len, bool need_y) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!m || !data) return fail(ctx, SVGP_INVALID_ARG, "null model or data");
  if (data->dtype != m->dtype) return fail(ctx, SVGP_INVALID_ARG, "data and model dtypes differ");
  if (data->d != m->d) return fail(ctx, SVGP_INVALID_ARG, "data and model input dimensions differ");
  if (off < 0 || len < 1 || off + len > data->n) return fail(ctx, SVGP_INVALID_ARG, "batch range outside the data");
  if (need_y && !data->y.p) return fail(ctx, SVGP_INVALID_ARG, "data has no observations y");
  return SVGP_OK;
}

// argument checks of the prior mean offsets (svgp_*_with_mean), before anything is enqueued
int check_point_mean(svgp_ctx* ctx, const svgp_point_mean* pm) {
  if (!pm) return SVGP_OK;
  if (!pm->mu) return fail(ctx, SVGP_INVALID_ARG, "null prior mean offsets");
  if ((pm->on_device != 0 && pm->on_device != 1) || pm->reserved != 0)
    return fail(ctx, SVGP_INVALID_ARG, "prior mean offsets: on_device must be 0 or 1 and reserved 0");
  return SVGP_OK;
}

// the batch's offsets on the device: a device pointer as it is, host memory by one copy into ctx->pm_x (bytes = batch_len x dtype size)
int stage_point_mean(svgp_ctx* ctx, const svgp_point_mean* pm, size_t bytes, const void** dev) {
  if (pm->on_device) { *dev = pm->mu; return SVGP_OK; }
  const int rc = ctx->pm_x.reserve(ctx, bytes, "the prior mean offsets");
  if (rc) return rc;
  HIPC(ctx, hipMemcpyAsync(ctx->pm_x.p, pm->mu, bytes, hipMemcpyHostToDevice, ctx->stream));
  *dev = ctx->pm_x.p;
  return SVGP_OK;
}

// One evaluation = three stages, so that a process driving several GPUs (svgp_group_*) can enqueue every device before
// it waits for any:  elbo_enqueue (prep + strips + reduce, asynchronous)  ->  elbo_collective (ONE ncclAllReduce of the
// device-resident 8-vector d_res on the context's stream; nothing without a communicator)  ->  elbo_finish (read back).
// skip_expect (svgp_predictive): the same prep and strips, but neither expect_kernel nor final_reduce_kernel behind them - the caller
// launches its own point stage on the moments and reads the prep scalars itself
int elbo_enqueue(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, const void* mux, bool skip_expect) {
  hipStream_t s = ctx->stream;
  HIPC(ctx, hipSetDevice(ctx->device));
  const OverlapPlan op = overlap_plan(ctx, m, len);
  int rc = SVGP_OK;
  if (op.on) {
    rc = ensure_overlap(ctx, size_t(op.nstrips) * strip_seg_state_doubles(m->dtype, op.nt));
    if (rc) return rc;
  }
  ctx->overlapped = op.on;
  SegRun seg;
  RowHook hook{seg_row_hook, &seg};
  if (op.on) {
    rc = seg_prepare_forward(ctx, m, data->x.p, data->ldx, off, len, op, seg);
    if (rc) return rc;
    seg.a.mux = mux;
  }
  TREC(ctx, ctx->ev[0], s);
  rc = enqueue_prep(ctx, m, op.on, op.on ? &hook : nullptr);
  if (rc == SVGP_OK && op.on) rc = seg.rc;
  if (rc) {   // between the fork and the join
    if (op.on) drain_second_stream(ctx);
    return rc;
  }
  TREC(ctx, ctx->ev[1], s);
  StripOuts so;
  so.mux = mux;
  so.skip_expect = skip_expect;
  rc = op.on ? seg_finish_forward(ctx, m, data->y.p, off, len, so, seg)
             : enqueue_strips(ctx, m, data->x.p, data->ldx, data->y.p, off, len, so);
  if (rc) {
    if (op.on) drain_second_stream(ctx);
    return rc;
  }
  TREC(ctx, ctx->ev[3], s);
  return SVGP_OK;
}

// `local_rc` is the status of this rank's enqueue: a rank that failed still takes part in the collective, with its
// failure flag set, so that its peers return an error instead of waiting for it forever (they all see failed > 0).
int elbo_collective(svgp_ctx* ctx, int local_rc) {
  if (!ctx->comm) return local_rc;
  if (local_rc != SVGP_OK) {
    const std::string keep = ctx->err;
    static const double poison[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    if (hipSetDevice(ctx->device) != hipSuccess ||
        hipMemcpyAsync(ctx->d_res.as<double>(), poison, sizeof poison, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
      comm_abort(ctx);
      ctx->err = keep;
      return local_rc;
    }
    ctx->err = keep;
  }
  const int rc = comm_allreduce(ctx, ctx->d_res.as<double>(), 8, SVGP_F64);
  if (rc != SVGP_OK) {
    comm_abort(ctx);
    return local_rc != SVGP_OK ? local_rc : rc;
  }
  return local_rc;
}

int elbo_finish(svgp_ctx* ctx, svgp_model* m, ElboRead* out) {
  hipStream_t s = ctx->stream;
  HIPC(ctx, hipSetDevice(ctx->device));
  double res[13];   // {sum E, n, n_neg, chol flag, failure flag, 0, 0, 0 | prep scalars (4), chol_info}: one copy
  PrepScalars ps;
  HIPC(ctx, hipMemcpyAsync(res, ctx->d_res.as<double>(), sizeof(res), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  for (int q = 0; q < 4; ++q) ps.scal[q] = res[8 + q];
  ps.info = int(res[12]);
  finish_prep(m, ps);
  float t01 = 0, t12 = 0, t23 = 0;
  (void)elapsed_ms(ctx, &t01, ctx->ev[0], ctx->ev[1]);
  (void)elapsed_ms(ctx, &t12, ctx->ev[1], ctx->ev[2]);
  (void)elapsed_ms(ctx, &t23, ctx->ev[2], ctx->ev[3]);
  ctx->timing.ms_prep = t01;
  ctx->timing.ms_strip = t12;
  ctx->timing.ms_expect = t23;
  ctx->timing.ms_total = t01 + t12 + t23;
  ctx->timing.ms_kuf = 0;
  float tch = 0;
  (void)elapsed_ms(ctx, &tch, ctx->ev_chol[0], ctx->ev_chol[1]);
  ctx->timing.ms_chol = tch;
  ctx->timing.ms_overlap = 0;
  if (ctx->overlapped) {   // the part of the prep the strips ran beside: from their first launch's completion to the prep's end
    float tov = 0;
    if (elapsed_ms(ctx, &tov, ctx->ev_ov[1], ctx->ev[1]) == hipSuccess && tov > 0) ctx->timing.ms_overlap = tov;
  }
  out->E = res[0];
  out->n_points = res[1];
  out->n_neg = res[2];
  out->bad_chol = res[3];
  out->failed = res[4];
  return SVGP_OK;
}

}  // namespace svgp

namespace {

// prep + strips (+ collective) + readback; refreshes the model's prep scalars
int run_elbo(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, bool collective, ElboRead* out,
             const void* mux = nullptr) {
  int rc = elbo_enqueue(ctx, m, data, off, len, mux);
  if (collective) rc = elbo_collective(ctx, rc);
  if (rc) return rc;
  return elbo_finish(ctx, m, out);
}

}  // namespace

namespace svgp {

int status_of(svgp_ctx* ctx, const svgp_model* m, double nneg, double bad_chol, double failed) {
  if (failed > 0)
    return fail(ctx, SVGP_RCCL_ERROR, "a peer rank failed before the collective; the data-parallel evaluation was abandoned on every rank");
  if (m->chol_info != 0 || bad_chol > 0) {
    char buf[160];
    snprintf(buf, sizeof buf, "Kuu is not positive definite: leading minor of order %d (PosDefException)", m->chol_info);
    return fail(ctx, SVGP_NOT_POSDEF, buf);
  }
  if (nneg > 0 && m->desc.neg_var_policy == SVGP_NEGVAR_ERROR) {
    char buf[160];
    snprintf(buf, sizeof buf, "%lld predictive variances were negative (DomainError in sqrt)", (long long)nneg);
    return fail(ctx, SVGP_NEG_VARIANCE, buf);
  }
  return SVGP_OK;
}

int ensure_prepared(svgp_ctx* ctx, svgp_model* m) {
  if (m->prepared) return SVGP_OK;
  int rc = enqueue_prep(ctx, m);
  if (rc) return rc;
  PrepScalars ps;
  HIPC(ctx, hipMemcpyAsync(ps.scal, m->scal.as<double>(), sizeof(ps.scal), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(ctx, hipMemcpyAsync(&ps.info, m->info.as<int>(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  finish_prep(m, ps);
  return status_of(ctx, m, 0);
}

void fill_terms(svgp_terms* t, const svgp_model* m, double elbo, const ElboRead& r, double scale) {
  if (!t) return;
  t->elbo = elbo;
  t->expectation = r.E;
  t->kl = m->kl;
  t->scale = scale;
  t->logdet_kuu = m->logdet_kuu;
  t->n_points = int64_t(r.n_points);
  t->n_neg_var = int64_t(r.n_neg);
  t->chol_info = m->chol_info;
  t->reserved = 0;
}

}  // namespace svgp

namespace {

// svgp_elbo (pm = NULL) and svgp_elbo_with_mean
int elbo_impl(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double num_data, double* elbo_out,
              svgp_terms* terms_out, const svgp_point_mean* pm) {
  int rc = check_batch(ctx, m, data, off, len, true);
  const void* mux = nullptr;
  if (pm) {   // (ctx is not NULL here unless check_batch failed)
    if (rc == SVGP_OK) rc = check_point_mean(ctx, pm);
    if (rc == SVGP_OK && hipSetDevice(ctx->device) != hipSuccess) rc = fail(ctx, SVGP_HIP_ERROR, "hipSetDevice failed");
    if (rc == SVGP_OK) rc = stage_point_mean(ctx, pm, size_t(len) * m->es, &mux);
  }
  if (rc) return (ctx && ctx->comm) ? elbo_collective(ctx, rc) : rc;   // keep the peers' collective matched
  ElboRead r;
  rc = run_elbo(ctx, m, data, off, len, true, &r, mux);
  if (rc) return rc;
  const double scale = (num_data > 0 ? num_data : r.n_points) / r.n_points;   // SVA:357-358
  const double elbo = r.E * scale - m->kl;                                     // SVA:359
  fill_terms(terms_out, m, elbo, r, scale);
  rc = status_of(ctx, m, r.n_neg, r.bad_chol, r.failed);
  if (elbo_out) *elbo_out = (rc == SVGP_OK) ? elbo : NAN;
  return rc;
}

}  // namespace

extern "C" {

int32_t svgp_elbo_partial(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                          double partial_out[4]) {
  int rc = check_batch(ctx, m, data, off, len, true);
  if (rc) return rc;
  if (!partial_out) return fail(ctx, SVGP_INVALID_ARG, "null output");
  ElboRead r;
  rc = run_elbo(ctx, m, data, off, len, false, &r);   // always local: no collective
  if (rc) return rc;
  partial_out[0] = r.E;
  partial_out[1] = double(len);
  partial_out[2] = r.n_neg;
  partial_out[3] = double(m->chol_info);
  return status_of(ctx, m, r.n_neg);
}

// With a communicator attached (svgp_ctx_attach_comm / svgp_group_create) this call is COLLECTIVE: every rank passes
// its own shard's batch, the ranks' {sum E, n, n_neg, flags} are summed by one ncclAllReduce on the device, and every
// rank returns the same global ELBO = sum E * num_data / n_global - KL (SVA:355-359; the KL is replicated, not summed).
int32_t svgp_elbo(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double num_data,
                  double* elbo_out, svgp_terms* terms_out) {
  return elbo_impl(ctx, m, data, off, len, num_data, elbo_out, terms_out, nullptr);
}

int32_t svgp_elbo_with_mean(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double num_data,
                            const svgp_point_mean* pm, double* elbo_out, svgp_terms* terms_out) {
  return elbo_impl(ctx, m, data, off, len, num_data, elbo_out, terms_out, pm);
}

int32_t svgp_prior_kl(svgp_ctx* ctx, svgp_model* m, double* kl_out, double* logdet_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!m) return fail(ctx, SVGP_INVALID_ARG, "null model");
  HIPC(ctx, hipSetDevice(ctx->device));
  int rc = ensure_prepared(ctx, m);
  if (rc) return rc;
  if (kl_out) *kl_out = m->kl;
  if (logdet_out) *logdet_out = m->logdet_kuu;
  return SVGP_OK;
}

int32_t svgp_elbo_host(svgp_ctx* ctx, const svgp_model_desc* desc, int32_t layout_x, int64_t n, const void* x_host,
                       const void* y_host, double num_data, double* elbo_out, svgp_terms* terms_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!desc || !y_host) {
    const int rc0 = fail(ctx, SVGP_INVALID_ARG, "null descriptor or observations");
    return ctx->comm ? elbo_collective(ctx, rc0) : rc0;
  }
  svgp_model* m = nullptr;
  svgp_data* D = nullptr;
  int rc = svgp_model_create(ctx, desc, &m);
  if (rc == SVGP_OK) rc = svgp_data_upload(ctx, desc->dtype, layout_x, desc->d, n, x_host, y_host, &D);
  if (rc == SVGP_OK) rc = svgp_elbo(ctx, m, D, 0, n, num_data, elbo_out, terms_out);
  else if (ctx->comm) rc = elbo_collective(ctx, rc);   // this rank never reached svgp_elbo: join its peers' all-reduce with the failure flag
  svgp_data_free(ctx, D);
  svgp_model_free(ctx, m);
  return rc;
}

int32_t svgp_kuf(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, void* Kuf_out_host) {
  int rc = check_batch(ctx, m, data, off, len, false);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t bytes = size_t(m->M) * size_t(len) * m->es;
  rc = ctx->kuf_buf.reserve(ctx, bytes, "Kuf");
  if (rc) return rc;
  launch_scale_inputs(m->dtype, s, m->z_raw.p, m->desc.layout_z, m->d, m->M, m->Mp, m->invl.p, m->zs.p);
  TREC(ctx, ctx->ev[0], s);
  launch_kuf(m->dtype, s, kparams(m), m->zs.p, m->M, m->Mp, data->x.p, data->ldx, off, len, ctx->kuf_buf.p);
  TREC(ctx, ctx->ev[1], s);
  HIPC(ctx, hipGetLastError());
  if (Kuf_out_host) HIPC(ctx, hipMemcpyAsync(Kuf_out_host, ctx->kuf_buf.p, bytes, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  float t = 0;
  (void)elapsed_ms(ctx, &t, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_kuf = t;
  ctx->timing.ms_total = t;
  return SVGP_OK;
}

int32_t svgp_posterior(svgp_ctx* ctx, svgp_model* m, void* Lk_out, void* alpha_out, void* B_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!m) return fail(ctx, SVGP_INVALID_ARG, "null model");
  HIPC(ctx, hipSetDevice(ctx->device));
  int rc = ensure_prepared(ctx, m);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const size_t es = m->es, M = size_t(m->M), Mp = size_t(m->Mp);
  DevBuf tmpbuf;
  HIPC(ctx, tmpbuf.alloc((M * M + Mp) * es));
  void* tmp = tmpbuf.p;
  void* vec = static_cast<char*>(tmp) + M * M * es;
  if (Lk_out) {
    launch_extract_lower(m->dtype, s, m->L.p, m->Mp, m->M, tmp);
    HIPC(ctx, hipMemcpyAsync(Lk_out, tmp, M * M * es, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
  }
  if (alpha_out) {
    // α = Lk' \ m~ (SVA:182; for Centered m~ = Lk \ (m − μ) so α = Kuu \ (m − μ), SVA:134)
    HIPC(ctx, hipMemcpyAsync(vec, m->mp.p, Mp * es, hipMemcpyDeviceToDevice, s));
    launch_trsv2(m->dtype, s, m->L.p, m->T.p, m->Mp, 1, vec);
    HIPC(ctx, hipMemcpyAsync(alpha_out, vec, M * es, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
  }
  if (B_out) {
    if (m->desc.parametrization == SVGP_CENTERED) {
      launch_extract_lower(m->dtype, s, m->B.p, m->Mp, m->M, tmp);
    } else {
      launch_extract_lower(m->dtype, s, m->Lq_raw.p, m->M, m->M, tmp);
    }
    HIPC(ctx, hipMemcpyAsync(B_out, tmp, M * M * es, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
  }
  HIPC(ctx, hipGetLastError());
  return SVGP_OK;
}

static int32_t predict_impl(svgp_ctx* ctx, svgp_model* m, int32_t layout, int64_t nx, const void* x_host, int64_t ny,
                            const void* y_host, void* mean_out, void* var_out, void* cov_out, bool cross) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!m || !x_host || nx < 1) return fail(ctx, SVGP_INVALID_ARG, "bad predict arguments");
  HIPC(ctx, hipSetDevice(ctx->device));
  int rc = ensure_prepared(ctx, m);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const size_t es = m->es;
  svgp_data *Xd = nullptr, *Yd = nullptr;
  rc = make_data(ctx, m->dtype, layout, m->d, nx, x_host, nullptr, &Xd);
  std::unique_ptr<svgp_data> X(Xd), Y;
  if (rc == SVGP_OK && cross) {
    rc = make_data(ctx, m->dtype, layout, m->d, ny, y_host, nullptr, &Yd);
    Y.reset(Yd);
  }
  if (rc) return rc;
  auto pad = [](int64_t n) { return (n + 127) / 128 * 128; };
  const int64_t ldax = pad(nx), lday = cross ? pad(ny) : 0;
  DevBuf mu, var, Ax, Cx, Ay, Cy, cov;
  const bool want_cov = cov_out != nullptr;
  hipError_t e = mu.alloc(size_t(nx) * es);
  if (e == hipSuccess) e = var.alloc(size_t(nx) * es);
  if (want_cov) {
    if (e == hipSuccess) e = Ax.alloc(size_t(m->Mp) * ldax * es);
    if (e == hipSuccess) e = Cx.alloc(size_t(m->Mp) * ldax * es);
    if (cross) {
      if (e == hipSuccess) e = Ay.alloc(size_t(m->Mp) * lday * es);
      if (e == hipSuccess) e = Cy.alloc(size_t(m->Mp) * lday * es);
    }
    if (e == hipSuccess) e = cov.alloc(size_t(nx) * size_t(cross ? ny : nx) * es);
  }
  if (e != hipSuccess) return alloc_failed(ctx, "in predict");
  StripOuts o;
  o.mu = mu.p; o.var = var.p; o.A = Ax.p; o.C = Cx.p; o.lda = ldax;
  rc = enqueue_strips(ctx, m, X->x.p, X->ldx, nullptr, 0, nx, o);
  if (rc == SVGP_OK && cross && want_cov) {
    StripOuts oy;
    oy.A = Ay.p; oy.C = Cy.p; oy.lda = lday;
    rc = enqueue_strips(ctx, m, Y->x.p, Y->ldx, nullptr, 0, ny, oy);
  }
  if (rc == SVGP_OK && want_cov) {
    if (cross)
      launch_cov_assemble(m->dtype, s, kparams(m), X->x.p, X->ldx, nx, Y->x.p, Y->ldx, ny, Ax.p, Cx.p, ldax, Ay.p, Cy.p, lday, m->Mp, cov.p);
    else
      launch_cov_assemble(m->dtype, s, kparams(m), X->x.p, X->ldx, nx, X->x.p, X->ldx, nx, Ax.p, Cx.p, ldax, Ax.p, Cx.p, ldax, m->Mp, cov.p);
  }
  hipError_t le = hipGetLastError();
  if (rc == SVGP_OK && le != hipSuccess) rc = fail(ctx, SVGP_HIP_ERROR, hipGetErrorString(le));
  if (rc == SVGP_OK) {
    if (mean_out) (void)hipMemcpyAsync(mean_out, mu.p, size_t(nx) * es, hipMemcpyDeviceToHost, s);
    if (var_out) (void)hipMemcpyAsync(var_out, var.p, size_t(nx) * es, hipMemcpyDeviceToHost, s);
    if (want_cov) (void)hipMemcpyAsync(cov_out, cov.p, size_t(nx) * size_t(cross ? ny : nx) * es, hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) rc = fail(ctx, SVGP_HIP_ERROR, "stream sync failed in predict");
  } else {
    (void)hipStreamSynchronize(s);
  }
  return rc;
}

int32_t svgp_predict(svgp_ctx* ctx, svgp_model* m, int32_t layout_x, int64_t n, const void* x_host, void* mean_out,
                     void* var_out, void* cov_out) {
  return predict_impl(ctx, m, layout_x, n, x_host, 0, nullptr, mean_out, var_out, cov_out, false);
}

int32_t svgp_predict_cross_cov(svgp_ctx* ctx, svgp_model* m, int32_t layout, int64_t nx, const void* x_host, int64_t ny,
                               const void* y_host, void* cov_out) {
  if (ctx && (!y_host || ny < 1 || !cov_out)) return fail(ctx, SVGP_INVALID_ARG, "bad cross-cov arguments");
  return predict_impl(ctx, m, layout, nx, x_host, ny, y_host, nullptr, nullptr, cov_out, true);
}

}  // extern "C"

// ---- likelihoods the ABI does not enumerate ("generic GH for user link functions") -------------------
// The M^2 N work does not depend on the likelihood: only (mu_i, v_i) -> E_i does, and that is O(N) scalar work the host can do
// with ANY single-latent GPLikelihoods likelihood and quadrature.  svgp_marginals hands the host marginals(f_post(x)) of
// SVA:354; the host evaluates expected_loglikelihood (SVA:355) and, for training, its derivatives w.r.t. (mu_i, v_i);
// svgp_elbo_grad_ext runs the same backward pass as svgp_elbo_grad with those point gradients in place of lik.hpp's.
namespace {
// svgp_marginals (pm = NULL) and svgp_marginals_with_mean
int marginals_impl(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, double* mean_out, double* var_out,
                   const svgp_point_mean* pm) {
  int rc = check_batch(ctx, m, data, off, len, false);
  if (rc) return rc;
  if (!mean_out || !var_out) return fail(ctx, SVGP_INVALID_ARG, "null output");
  rc = check_point_mean(ctx, pm);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  HIPC(ctx, hipSetDevice(ctx->device));
  StripOuts so;
  so.skip_expect = true;
  if (pm) {
    rc = stage_point_mean(ctx, pm, size_t(len) * m->es, &so.mux);
    if (rc) return rc;
  }
  TREC(ctx, ctx->ev[0], s);
  rc = enqueue_prep(ctx, m);
  if (rc) return rc;
  TREC(ctx, ctx->ev[1], s);
  rc = enqueue_strips(ctx, m, data->x.p, data->ldx, nullptr, off, len, so);
  if (rc) return rc;
  PrepScalars ps;
  HIPC(ctx, hipMemcpyAsync(mean_out, ctx->mom_mu(), size_t(len) * 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(var_out, ctx->mom_var(), size_t(len) * 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(ps.scal, m->scal.as<double>(), sizeof(ps.scal), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(&ps.info, m->info.as<int>(), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  finish_prep(m, ps);
  float t01 = 0, t12 = 0;
  (void)elapsed_ms(ctx, &t01, ctx->ev[0], ctx->ev[1]);
  (void)elapsed_ms(ctx, &t12, ctx->ev[1], ctx->ev[2]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_prep = t01;
  ctx->timing.ms_strip = t12;
  ctx->timing.ms_total = t01 + t12;
  double nneg = 0;
  const bool clamp = m->desc.neg_var_policy == SVGP_NEGVAR_CLAMP;
  for (int64_t i = 0; i < len; ++i) {   // FiniteGP(f_post, x, 1e-18): the variance the reference's marginals() hold
    double v = var_out[i] + kDefaultSigma2;
    if (v < 0.0) { nneg += 1; if (clamp) v = 0.0; }
    var_out[i] = v;
  }
  return status_of(ctx, m, nneg);
}
}  // namespace

extern "C" int32_t svgp_marginals(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                  double* mean_out, double* var_out) {
  return marginals_impl(ctx, m, data, off, len, mean_out, var_out, nullptr);
}

extern "C" int32_t svgp_marginals_with_mean(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len,
                                            const svgp_point_mean* pm, double* mean_out, double* var_out) {
  return marginals_impl(ctx, m, data, off, len, mean_out, var_out, pm);
}
