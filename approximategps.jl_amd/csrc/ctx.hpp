// ctx.hpp — internal definitions shared by the host-side translation units of libsvgp_mi355x (api.hip and its api_*.hip siblings, comm.hip, laplace.hip, nn.hip):
// the owning types of every device resource, the opaque handles of include/svgp_mi355x.h and the error macros.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/svgp_mi355x.h"
#include "knobs.hpp"

namespace svgp {
inline int fail(svgp_ctx* ctx, int code, const std::string& msg);
inline int alloc_failed(svgp_ctx* ctx, const std::string& where);   // SVGP_OOM, "hipMalloc failed <where>"

// ---- owning types -------------------------------------------------------------------------------
// Every device allocation, pinned host buffer, event and stream of the host layer is a member or a local of one of these four
// types, and this header is the only place that calls the HIP functions that make or release them
// (tests/test_resource_ownership_cpu.py).  A handle's destructor therefore releases what the handle holds, on every path.
// Releasing device memory synchronises the device: a buffer that persists on a handle is released on growth and with the handle only.

// device memory: pointer + capacity in bytes.  No conversion to a pointer: say .p, or as<T>() where arithmetic follows
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool own = true;   // false: a caller's device pointer (svgp_data_wrap_device), never freed here
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p && own) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  hipError_t alloc(size_t bytes) {
    release();
    own = true;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes; else p = nullptr;
    return e;
  }
  // grow-only, contents not kept; on failure empty, ctx's error set, SVGP_OOM
  int reserve(svgp_ctx* ctx, size_t bytes, const char* what) {
    if (bytes <= cap) return SVGP_OK;
    return alloc(bytes) == hipSuccess ? SVGP_OK : alloc_failed(ctx, std::string("for ") + what);
  }
  void borrow(const void* q) { release(); p = const_cast<void*>(q); own = false; }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// pinned host memory
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  int reserve(svgp_ctx* ctx, size_t bytes, const char* what) {
    if (bytes <= cap) return SVGP_OK;
    release();
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { p = nullptr; return fail(ctx, SVGP_OOM, std::string("hipHostMalloc failed for ") + what); }
    cap = bytes;
    return SVGP_OK;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned flags) {   // once: a second call keeps the event
    if (e) return hipSuccess;
    const hipError_t r = hipEventCreateWithFlags(&e, flags);
    if (r != hipSuccess) e = nullptr;
    return r;
  }
  operator hipEvent_t() const { return e; }
};

// a stream of the library's own, or the caller's (borrow): only the former is destroyed
struct Stream {
  hipStream_t s = nullptr;
  bool own = false;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s && own) (void)hipStreamDestroy(s); }
  void borrow(void* q) { s = static_cast<hipStream_t>(q); own = false; }
  hipError_t create(unsigned flags) { return made(hipStreamCreateWithFlags(&s, flags)); }
  hipError_t create(unsigned flags, int priority) { return made(hipStreamCreateWithPriority(&s, flags, priority)); }
  operator hipStream_t() const { return s; }
 private:
  hipError_t made(hipError_t r) { if (r == hipSuccess) own = true; else s = nullptr; return r; }
};
}  // namespace svgp

// ------------------------------------------------------------------------------------------------
struct svgp_ctx {
  int device = 0;
  svgp::Stream stream;
  // concurrent narrow-strip launch for the last partial round of a batch (enqueue_strips): its own stream, queue and scratch
  svgp::Stream stream2;
  int num_cus = 256;
  svgp::Knobs kn;   // environment settings, read once at context creation (knobs.hpp)
  std::string err;
  svgp_timing timing{};
  svgp::Event ev[4];        // start, prep done, strip done, all done
  svgp::Event ev_chol[2];   // around the blocked Cholesky inside the prep
  // growable scratch
  svgp::DevBuf work;
  svgp::DevBuf partial, negcnt;   // [1024] per-block sums of the expectation kernel (double / unsigned)
  svgp::DevBuf mom;               // [2][n] per-point mean / variance (double)
  double* mom_mu() const { return mom.as<double>(); }
  double* mom_var() const { return mom.as<double>() + mom.cap / (2 * sizeof(double)); }
  svgp::DevBuf d_res;     // [8] device results (double)
  svgp::DevBuf counter;   // strip queue head of the running strip launch (unsigned)
  svgp::Event ev_fork, ev_join;
  svgp::DevBuf counter2;
  svgp::DevBuf work2;
  // strips beside the factorisation (host.hpp: SegRun): one event per block row of T, the segmented strips' saved sums
  svgp::Event ev_row[16];
  bool ev_row_ready = false, overlapped = false;
  bool timing_on = true;   // SVGP_TIMING=0 at context creation: no timing events on the stream (each record costs the stream ~5 us); svgp_last_timing then reports zeros
  svgp::Event ev_S;       // the chain-independent part of the gradient's prep (S = B B' - I, cleared accumulators), second stream
  svgp::Event ev_R;       // the gradient's M-sized prep (Linv, alpha, R) is final: phase 3 of the segmented strips
  svgp::Event ev_ov[2];   // timed: fork point, first strip launch done (svgp_timing.ms_overlap)
  svgp::DevBuf seg_state;   // (double)
  svgp::DevBuf work_seg;    // per-strip scratch of the segmented strips
  svgp::HostBuf hstage;     // pinned host staging of the gradient read-back (api_grad.hip: grad_finish)
  svgp::Event ev_piece[8];  // one behind each piece of that read-back
  svgp::DevBuf kuf_buf;
  svgp::DevBuf ext_g;   // [2][n] point gradients of a host-evaluated likelihood (double)
  svgp::DevBuf pm_x;    // host-memory prior mean offsets of a call, copied in (svgp_*_with_mean)
  svgp::DevBuf pm_g;    // their gradient for a host destination, copied out (svgp_elbo_grad_with_mean)
  // svgp_collapsed_*_with_noise (allocated by their first call)
  svgp::DevBuf pn_x;    // host-memory per-point noise variances of a call, copied in (pm_x holds mux during the same call)
  svgp::DevBuf pn_g;    // their gradient for a host destination, copied out (pm_g holds mux_bar during the same call)
  svgp::DevBuf pn_w;    // w_j = 1 / sigma_j^2 of the window, model dtype, zero-padded to 128 points: the weighted SYRK's operand
  svgp::DevBuf pn_wd;   // ... in fp64: the reductions' (then one int: the count of sigma_j^2 <= 0)
  // svgp_predictive / svgp_lik_predictive (allocated by their first call)
  svgp::DevBuf pred_part;   // [1024][3] per-block sums of predictive_kernel, then [4] their sums (double)
  svgp::DevBuf pred_out;    // [3][n] per-point lpd | ymean | yvar (double)
  svgp::DevBuf pred_in;     // [3][n] a caller's mu | var | y (double; svgp_lik_predictive)
  svgp::DevBuf pred_gh;     // [2][pred_gh_n] Gauss-Hermite nodes | weights / sqrt(pi) of the predictive rule (double)
  int pred_gh_n = 0;
  svgp::DevBuf smp_out;     // [S][len] samples of a host-output svgp_sampler_eval call, copied out (model dtype)
  svgp::DevBuf smp_grad;    // [S][d][len] gradients of a host-output svgp_sampler_eval_grad call, copied out (model dtype)
  svgp::DevBuf cgs_part;    // the row segments' partial sums of one svgp_cg_sampler_eval / _eval_grad call (kernels.hpp: CgSampleArgs::part)
  struct GradWs* gws = nullptr;  // gradient workspace, cached by problem shape (deleted by svgp_ctx_destroy)
  struct CollapsedWs* cws = nullptr;   // fp64 M-sized tail of svgp_collapsed_*, cached by Mp (deleted by svgp_ctx_destroy)
  // data-parallel communicator (comm.hip): one RCCL rank per context; world == 1 without one
  void* comm = nullptr;        // ncclComm_t
  int world = 1, rank = 0;
  bool comm_owned_by_group = false;
  svgp::HostBuf h_open;   // pinned host word (double): the reduced failure flag of svgp_elbo_grad's opening all-reduce (api_grad.hip: grad_handshake)
  svgp::Event ev_open;    // ... recorded behind its copy
  svgp::DevBuf d_coll;    // [8] the all-reduced vector {sum E, n_points, n_neg_var, chol flag, failure flag, ...} (double)
};

// device buffers of svgp_elbo_grad, sized by (dtype, Mp, d, nc)
struct GradWs {
  int dtype = -1, d = 0, nslices = 1, ns_uf = 1, ns_uu = 1, rb = 1;
  int64_t Mp = 0, nc = 0;
  svgp::DevBuf At, Pt;   // per chunk: A and P = Kuf_bar point-major [nc][Mp]
  svgp::DevBuf gmu;      // per chunk: g_mu | g_v, one allocation
  void* gv = nullptr;    // ... its second half
  svgp::DevBuf Lqp, G1, G2, LkRM, LbarRM, Phi, tmp, H, BbarRM, rbar;
  svgp::DevBuf LinvRM, LinvCM;   // Lk^-1 in both storage orders (launch_linv): every Lk^-T . of the tail is a GEMM with it
  svgp::DevBuf Gmm;   // split-K scratch of the M x M products that run BESIDE an early SYRK (api_grad.hip: grad_plan), allocated on first use
  svgp::DevBuf W2, Rcm, G1p, alpha;   // W = A diag(2 g_v) A', R = Lk^-T (Lq Lq' - I), 2 W Lq, Lk^-T m
  // the user-layout gradient blocks {z_bar (M d) | m_bar (M) | Lq_bar (M^2)}: ONE allocation, contiguous for the model's M, so
  // that the data-parallel sum is one ncclAllReduce and the read-back one copy; zbar / mbar / Lqbar point into it (set per call)
  svgp::DevBuf gblk;
  void *zbar = nullptr, *mbar = nullptr, *Lqbar = nullptr;
  svgp::DevBuf cblk;   // the same block with Lq_bar packed to its lower triangle: what the collective all-reduces (M d + M + M (M + 1) / 2)
  // accumulators zeroed by ONE memset per evaluation: [rp_uf | sp_uf | rp_uu | sp_uu | sums (8) | scal_out (1 + dreg) | prep (5)]
  svgp::DevBuf zero_blk;
  size_t zero_b = 0;
  double *rp_uf = nullptr, *sp_uf = nullptr, *rp_uu = nullptr, *sp_uu = nullptr, *sums = nullptr, *scal_out = nullptr;   // into zero_blk
  svgp::DevBuf partial5, invl_d, avec, kred, gemv_part;   // (double)
  int64_t part5_strips = 0;
  size_t rp_uf_b = 0, sp_uf_b = 0, rp_uu_b = 0, sp_uu_b = 0, g_b = 0;
  svgp::DevBuf xg;   // d elbo / d x of a host-output svgp_elbo_grad_inputs call, [d][len], grown on demand
};

// device buffers of the M-sized tail of svgp_collapsed_* (fp64 whatever the model's dtype), sized by Mp
struct CollapsedWs {
  int64_t Mp = 0;
  svgp::DevBuf Bm, TB, LinvRM, LinvCM, Ytmp, Sinv;   // B -> LB, its T panels, LB^-1 in both storage orders, scratch, B^-1 -> Lq_w (Mp x Mp doubles each)
  svgp::DevBuf cvec, mw;       // c (Mp), m_w (Mp)
  svgp::DevBuf bpart, spart;   // the split partials of b = A r and of {r'r, sum A^2}
  svgp::DevBuf spart2;         // ... of {sum log sigma_j^2, sum w_j} (svgp_collapsed_*_with_noise)
  svgp::DevBuf scal;           // [8] {rr, t, sum log diag LB, c'c, info_b, info_s, 0, 0} (with per-point noise: [6] sum log sigma_j^2, [7] sum w_j)
  svgp::DevBuf info_b, info_s; // cholesky info + hand-over counters of the two factorisations (int)
  svgp::DevBuf gemv_part;
  // svgp_natgrad_step* only (allocated by its first call): W = A diag(-2 scale g_v) A' and the whitened factor B of q in fp64
  // (Mp x Mp doubles each), the index of B's first non-positive diagonal entry (int)
  svgp::DevBuf Wm, Bw, info_q;
};

struct svgp_data {
  int dtype = 0, d = 0;
  int64_t n = 0, ldx = 0;
  svgp::DevBuf x;  // feature-major [d][ldx]; the caller's memory after svgp_data_wrap_device
  svgp::DevBuf y;
};

struct svgp_model {
  svgp_model_desc desc{};
  std::vector<double> invl_host;
  int64_t M = 0, Mp = 0;
  int dtype = 0, d = 0;
  size_t es = 8;
  svgp::DevBuf z_raw, m_raw, Lq_raw;  // user layout
  svgp::DevBuf invl, zs, L, T, U, mp, B;
  svgp::DevBuf scal;  // [8 + Mp] (double)
  svgp::DevBuf info;  // (int)
  svgp::DevBuf gh_x, gh_w;   // (double)
  int gh_n = 0;
  bool prepared = false;
  svgp::DevBuf mu_z;    // [M] prior mean offsets at the inducing points (svgp_model_set_mean_z), model dtype; Centered prep only
  // host copies of the last prep's scalars
  double kl = 0, logdet_kuu = 0;
  int chol_info = 0;
};

// svgp_sampler_create's snapshot of S pathwise function samples (sample_api.hip): everything svgp_sampler_eval reads, so that the
// model it was made from may change or go
struct svgp_sampler {
  int dtype = 0, d = 0, family = 0, device = 0;
  size_t es = 8;
  int64_t M = 0, Mp = 0, L = 0, Lp = 0, S = 0, Sp = 0;
  double variance = 0, mean_const = 0;
  svgp::DevBuf invl, rows, bias, panel;   // model dtype (kernels.hpp: SampleEvalArgs)
  svgp::DevBuf u, V;                      // fp64: u [S][M], V [S][Mp] before its rounding into the panel (svgp_sampler_state)
};

// one process driving several GPUs: member contexts share one RCCL communicator (ncclCommInitAll), rank i = member i
struct svgp_group {
  std::vector<svgp_ctx*> ctxs;
  std::string err;
};

#define HIPC(ctx, call)                                                                            \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_) + svgp::noted();              \
      return (e_ == hipErrorOutOfMemory) ? SVGP_OOM : SVGP_HIP_ERROR;                              \
    }                                                                                              \
  } while (0)

namespace svgp {
std::string take_note_text();   // prep.hip: the pending host-side diagnosis (device_common.hpp: leave_note), emptied
inline std::string noted() {
  const std::string n = take_note_text();
  return n.empty() ? n : " [" + n + "]";
}
}  // namespace svgp

// SVGP_DEBUG_SYNC=1: synchronise and check after every kernel launch, naming the offender.
inline bool debug_sync() {
  static const bool on = [] { const char* e = getenv("SVGP_DEBUG_SYNC"); return e && e[0] == '1'; }();
  return on;
}
#define KCHECK(ctx, name)                                                                          \
  do {                                                                                             \
    hipError_t e_ = hipGetLastError();                                                             \
    if (e_ == hipSuccess && debug_sync()) e_ = hipStreamSynchronize((ctx)->stream);                \
    if (e_ != hipSuccess) {                                                                        \
      (ctx)->err = std::string("kernel ") + name + ": " + hipGetErrorString(e_) + svgp::noted();   \
      return SVGP_HIP_ERROR;                                                                       \
    }                                                                                              \
  } while (0)

namespace svgp {
// ---- comm.hip: RCCL, loaded lazily with dlopen (the library has no link-time dependency on it) ----
// in-place sum all-reduce of `count` elements (f64: dtype 0, f32: dtype 1) on the context's stream; no host sync
int comm_allreduce(svgp_ctx* ctx, void* buf, size_t count, int dtype);
int comm_group_start(svgp_ctx* ctx);
int comm_group_end(svgp_ctx* ctx);
void comm_abort(svgp_ctx* ctx);   // after a local failure that left peers inside a collective: abort instead of hanging

inline int fail(svgp_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}
inline int alloc_failed(svgp_ctx* ctx, const std::string& where) { return fail(ctx, SVGP_OOM, "hipMalloc failed " + where); }
}  // namespace svgp
