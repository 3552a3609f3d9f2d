// host.hpp — the declarations that cross the host-only translation units of the C-ABI (api.hip, api_forward.hip, api_grad.hip,
// api_qopt.hip, api_predictive.hip, sample_api.hip), each under the unit that defines it.  A function used by one unit only lives in that unit's
// anonymous namespace; the owning types and the handles are ctx.hpp's.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/svgp_mi355x.h"
#include "ctx.hpp"
#include "kernels.hpp"
#include "knobs.hpp"

// Events between the context's own streams and for device-side timing need no system-scope fence (the cache write-back and invalidation
// that makes device memory visible to the HOST): a record then costs the stream ~1 instead of ~5 us (profiles/round4/minibatch_step.md
// section 7).  Everything the host reads comes through hipMemcpy + a stream / event synchronisation of DEFAULT events (ev_piece).
// SVGP_EVENT_FENCE=1 (experiments build, process-wide, A/B): default events everywhere.
inline unsigned event_flags(bool timing) {
  static const bool fence = svgp::exp_int("SVGP_EVENT_FENCE", 0) == 1;   // experiments build: A/B
  return (timing ? 0u : unsigned(hipEventDisableTiming)) | (fence ? 0u : unsigned(hipEventDisableSystemFence));
}
#define kSyncEvent event_flags(false)
#define kTimingEvent event_flags(true)
// (no query of events that were never recorded: it would leave a sticky "invalid resource handle" on the context's device)
inline hipError_t elapsed_ms(const svgp_ctx* ctx, float* ms, hipEvent_t a, hipEvent_t b) {
  if (!ctx->timing_on) { *ms = 0.0f; return hipErrorNotReady; }
  return hipEventElapsedTime(ms, a, b);
}
// timing events (ms_prep / ms_strip / ms_chol / ms_overlap of svgp_last_timing): recorded unless the context was created with SVGP_TIMING=0
#define TREC(ctx, ev, stream)                            \
  do {                                                   \
    if ((ctx)->timing_on) HIPC(ctx, hipEventRecord(ev, stream)); \
  } while (0)

namespace svgp {

// ---- api.hip ----------------------------------------------------------------------------------------------------------------
// Golub–Welsch: nodes/weights of the n-point Gauss–Hermite rule (weight exp(-x²)), as FastGaussQuadrature.gausshermite(n)
int gauss_hermite(int n, double* xs, double* ws);
int make_data(svgp_ctx* ctx, int dtype, int layout, int d, int64_t n, const void* x_host, const void* y_host, svgp_data** out);

// ---- api_forward.hip --------------------------------------------------------------------------------------------------------
KernelParams kparams(const svgp_model* m);
LikParams lik_params(const svgp_model* m);   // the ELBO's rule (the predictive rule is api_predictive.hip's own)
// info + the factorisation's hand-over counters and flags: 1 + 2 nP ints, rounded up to 256 bytes - a memset whose size is not a
// multiple of 16 bytes becomes TWO fill kernels (aligned body + tail), ~5 us of every call's prologue
inline size_t info_bytes(int64_t Mp) { return (sizeof(int) * size_t(1 + 2 * (Mp / 128)) + 255) / 256 * 256; }
int enqueue_prep(svgp_ctx* ctx, svgp_model* m, bool overlap = false, const RowHook* hook = nullptr);
// scalars of the last prep -> host (requires a stream sync by the caller before use)
struct PrepScalars { double scal[4]; int info; };
void finish_prep(svgp_model* m, const PrepScalars& ps);
int ensure_prepared(svgp_ctx* ctx, svgp_model* m);
int ensure_scratch(svgp_ctx* ctx, size_t work_bytes, size_t npoints);
int ensure_overlap(svgp_ctx* ctx, size_t state_doubles);   // second stream + the row events + the segmented strips' saved sums
// a failure between the fork and the join leaves work on the second stream that the main stream never waited for: drain it, so that
// the next call on this context cannot meet it in the shared scratch
void drain_second_stream(svgp_ctx* ctx);
int seg_split_factor(const svgp_ctx* ctx, int nP, int64_t nstrips);
int seg_split_setup(svgp_ctx* ctx, StripArgs& a, int S, int64_t nstrips);
// the strips' arguments every schedule shares, for points [off, off + len) of x: the model's operands, the context's scratch, queue
// head and moments (read them after the caller's ensure_scratch).  Outputs, seg_state, R / alpha and mux are the caller's.
StripArgs strip_args(const svgp_ctx* ctx, const svgp_model* m, const void* x, int64_t ldx, int64_t off, int64_t len);
// the one launch strip_plan_single gives `len` points: it never plans a main launch AND a tail, so one triple says it all
struct SinglePlan { int nt = 0, grid = 0; int64_t nstrips = 0; };
SinglePlan single_plan(int dtype, int64_t Mp, int64_t len, int num_cus);
// scratch of ONE strip per workgroup, sized for every chunk of a chunked data pass over `len` points BEFORE anything of its loop is
// enqueued (the full chunks and the shorter last one may plan differently); *max_strips: the larger strip count of the two
size_t chunk_work_bytes(const svgp_ctx* ctx, int dtype, int64_t Mp, int64_t len, int64_t nc, int64_t* max_strips = nullptr);

struct OverlapPlan { bool on = false; int nt = 0, grid = 0; int64_t nstrips = 0; };
OverlapPlan overlap_plan(const svgp_ctx* ctx, const svgp_model* m, int64_t len);
// The segmented strips of ONE evaluation.  Their launches wait for events the factorisation records panel by panel, and a wait can
// only be enqueued BEHIND its record - so they are enqueued from inside the factorisation's launch loop (RowHook), each right behind
// the record it waits for.  (Until late in round 4 they were enqueued after the whole prep: the host needs 5-10 us per launch, the ~25
// launches of the prep took it longer than the device needed to start the chain, and the strips' first panel reached the second stream
// when the chain was already a third - in the gradient, where the M-sized adjoint prep is enqueued first as well, completely - done.)
struct SegRun {
  svgp_ctx* ctx = nullptr;
  svgp_model* m = nullptr;
  StripArgs a{};
  OverlapPlan op;
  bool grad = false;
  int split = 1;   // forward: phase 2 in a closing launch of its own, `split` workgroups per strip (small batches; kernels.hpp: seg_split)
  int nP = 0, rc = SVGP_OK;
  size_t wb1 = 0;
  int (*pre)(void* user) = nullptr;   // work for the second stream ahead of the pre-generation (the gradient's chain-independent prep)
  void* pre_user = nullptr;
};
void seg_row_hook(void* user, int row);   // RowHook::fn with user = the evaluation's SegRun

int check_batch(svgp_ctx* ctx, const svgp_model* m, const svgp_data* data, int64_t off, int64_t len, bool need_y);
int check_point_mean(svgp_ctx* ctx, const svgp_point_mean* pm);
int stage_point_mean(svgp_ctx* ctx, const svgp_point_mean* pm, size_t bytes, const void** dev);

struct ElboRead {
  double E = 0, n_points = 0, n_neg = 0, bad_chol = 0, failed = 0;
};
int elbo_enqueue(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, const void* mux = nullptr,
                 bool skip_expect = false);
int elbo_collective(svgp_ctx* ctx, int local_rc);
int elbo_finish(svgp_ctx* ctx, svgp_model* m, ElboRead* out);
int status_of(svgp_ctx* ctx, const svgp_model* m, double nneg, double bad_chol = 0, double failed = 0);
void fill_terms(svgp_terms* t, const svgp_model* m, double elbo, const ElboRead& r, double scale);

// ---- api_grad.hip -----------------------------------------------------------------------------------------------------------
int syrk_slices(const svgp_ctx* ctx, const svgp_model* m, int64_t nc);
int64_t grad_chunk_points(int64_t Mp, size_t es, int64_t len);
int grad_workspace(svgp_ctx* ctx, svgp_model* m, int64_t len, GradWs** out);

// value = scale * sum_i E_i - klw * KL and its gradient over points [off, off + len): three stages like the forward
// evaluation.  Data-parallel (a communicator on the context, `collective`): every rank uses scale = num_data / n_global
// with n_global all-reduced on the device BEFORE the backward pass (the strips' phase 3 reads it there; no host hop) and
// klw = 1 / world, so the plain sum over ranks of (value, gradient) is the global ELBO and its gradient; that sum is ONE
// grouped ncclAllReduce of {z_bar, m_bar, Lq_bar, [sums | scal_out]} at the end.
struct GradCall {
  GradWs* w = nullptr;
  const double* n_global_dev = nullptr;
  double scale = 1.0, klw = 1.0, num_data = 0.0;
  bool collective = false, centered = false;
  bool packed = false;   // w->cblk already holds {z_bar | m_bar | packed tril(Lq_bar)} (the collective's all-reduced block)
  int64_t len = 0;
  // host-evaluated likelihood (svgp_elbo_grad_ext): per-point dE/dmu, dE/dv (host, fp64, [len] each) and the host's sum E
  const double *ext_gmu = nullptr, *ext_gv = nullptr;
  double ext_sum_e = 0.0;
  // svgp_elbo_grad_inputs / svgp_elbo_grad_ext_inputs: where d elbo / d x goes (NULL: not requested, nothing more is launched)
  const svgp_input_grad* gx = nullptr;
  // svgp_elbo_grad_with_mean: the batch's prior mean offsets (device, data dtype) and where their gradient goes (device; NULL: not
  // requested - point_grad_kernel writes its g_mu a second time there)
  const void* mux = nullptr;
  void* mux_bar = nullptr;
  // svgp_collapsed_grad_with_noise: the batch's per-point noise variances s (device, data dtype; the Gaussian likelihood's variance of
  // point j is lik_sigma2 + s[j]) and where d elbo / d sigma_j^2 goes (device; NULL: not requested).  With s the SYRK's weights 2 g_v
  // differ from point to point: the weighted route
  const void* noise = nullptr;
  void* noise_bar = nullptr;
  // svgp_natgrad_step: where W = A diag(-2 scale g_v) A' goes in fp64, gathered from the SYRK's slices before the tail reuses their
  // buffer as split-K scratch (NULL: not requested, nothing more is launched)
  double* ng_W = nullptr;
};
int grad_enqueue(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, GradCall& gc);
int grad_collective(svgp_ctx* ctx, svgp_model* m, GradCall& gc, int local_rc);
int grad_finish(svgp_ctx* ctx, svgp_model* m, GradCall& gc, double* elbo_out, svgp_terms* terms_out, svgp_grads* g);

// svgp_natgrad_step / _ext: the step length and the fp64 workspace of the M-sized tail that follows the value-and-gradient's launches
struct NatgradCall {
  double gamma = 1.0;
  CollapsedWs* c = nullptr;
};
// what one value-and-gradient call is asked for, beyond the batch and its outputs
struct GradRequest {
  double scale = 1.0, klw = 1.0, num_data = 0.0;
  bool collective = false;   // (only with a communicator on the context)
  const double *ext_gmu = nullptr, *ext_gv = nullptr;   // GradCall's
  double ext_sum_e = 0.0;
  const svgp_input_grad* gx = nullptr;
  const svgp_point_mean* pm = nullptr;
  const svgp_point_mean_grad* gpm = nullptr;
  const void* noise = nullptr;   // GradCall's: device pointers, staged by the caller (svgp_collapsed_grad_with_noise)
  void* noise_bar = nullptr;
  NatgradCall* ng = nullptr;   // (never collective): the natural-gradient tail behind the same launches
};
int elbo_grad_impl(svgp_ctx* ctx, svgp_model* m, const svgp_data* data, int64_t off, int64_t len, const GradRequest& rq,
                   double* elbo_out, svgp_terms* terms_out, svgp_grads* g);
int check_input_grad(svgp_ctx* ctx, const svgp_data* data, int64_t len, const svgp_input_grad* gx);
int check_point_mean_grad(svgp_ctx* ctx, const svgp_data* data, int64_t len, const svgp_input_grad* gx, const svgp_point_mean_grad* gpm);

// ---- api_qopt.hip -----------------------------------------------------------------------------------------------------------
int natgrad_enqueue(svgp_ctx* ctx, svgp_model* m, GradCall& gc, NatgradCall& ng);
int natgrad_finish(svgp_ctx* ctx, svgp_model* m, NatgradCall& ng);

}  // namespace svgp
