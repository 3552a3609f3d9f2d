// statespace_api.hip — the exact one-dimensional Matern GP in O(N): svgp_ss_create / _set_noise / _fit / _predict / _sample / _free (statespace.hip:
// the kernels).  Host orchestration only.  A Matern-3/2 or -5/2 GP over a scalar input is a linear Gaussian state-space model of state
// dimension 2 or 3: fit stages the points in fp64, runs the filter's scan and sums the one-step predictive log densities; predict merges
// the sorted test times into the sequence on the device as unobserved points and runs the filter's and the smoother's scans over the union;
// sample draws joint posterior paths over the same union by three scans of affine maps, a bounded group of samples at a time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <new>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"

using namespace svgp;

struct svgp_ss {
  const svgp_data* data = nullptr;
  int dtype = 0, device = 0;
  size_t es = 8;
  int64_t N = 0;
  DevBuf t, dl, r;               // the last fit's points in fp64
  DevBuf fm, work, part, res;    // filtered moments [D + D (D + 1) / 2][n], the scans' aggregates, the lml's partials and its sum
  DevBuf flag;                   // one int: what the device-side checks found
  DevBuf delta, noise_s;         // a caller's delta (fp64); the per-point noise snapshot (data dtype)
  DevBuf ts, tm, dm, rm, slot, out;   // predict: the test times, the union, the test points' slots, mean | var in the data dtype
  DevBuf ident, sz, seps, sft, smf, swork, sout;   // sample: the points' identities; one group's draws, prior paths, filtered means, aggregates, paths
  bool have_noise = false, have_fit = false;
  int family = 0;                // the parameter set of the last fit
  double variance = 0, inv_lengthscale = 0, mean_const = 0;
};

namespace {

constexpr int64_t kSsMaxPoints = (int64_t(1) << 31) - 1;   // (the slots are int)
constexpr size_t kSsSampleGroupBytes = size_t(4) << 30;     // svgp_ss_sample: the draws and intermediates of one group of samples

int check_desc(svgp_ctx* ctx, const svgp_ss* h, const svgp_ss_desc* ds) {
  if (!ds) return fail(ctx, SVGP_INVALID_ARG, "null descriptor");
  if (ds->dtype != h->dtype) return fail(ctx, SVGP_INVALID_ARG, "descriptor and data dtypes differ");
  if (ds->kernel == SVGP_KERNEL_SE) return fail(ctx, SVGP_UNSUPPORTED, "the squared-exponential kernel has no finite state-space form");
  if (ds->kernel != SVGP_KERNEL_MATERN32 && ds->kernel != SVGP_KERNEL_MATERN52) return fail(ctx, SVGP_INVALID_ARG, "unknown kernel family");
  if (!(ds->variance > 0) || !std::isfinite(ds->variance)) return fail(ctx, SVGP_INVALID_ARG, "variance must be > 0 and finite");
  if (!(ds->inv_lengthscale > 0) || !std::isfinite(ds->inv_lengthscale)) return fail(ctx, SVGP_INVALID_ARG, "inv_lengthscale must be > 0 and finite");
  if (!(ds->diag > 0) || !std::isfinite(ds->diag)) return fail(ctx, SVGP_INVALID_ARG, "diag must be > 0 and finite");
  if (!std::isfinite(ds->mean_const)) return fail(ctx, SVGP_INVALID_ARG, "mean_const must be finite");
  if (ds->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved must be 0");
  return SVGP_OK;
}

int handle_checks(svgp_ctx* ctx, const svgp_ss* h) {
  if (!h) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (h->device != ctx->device) return fail(ctx, SVGP_INVALID_ARG, "the state-space handle lives on another device than the context");
  if (ctx->comm) return fail(ctx, SVGP_UNSUPPORTED, "the state-space calls are local: the context has a communicator");
  return SVGP_OK;
}

// buffers of a filter over n points
int reserve_scan(svgp_ctx* ctx, svgp_ss* h, int64_t n) {
  int rc;
  if ((rc = h->fm.reserve(ctx, size_t(9) * size_t(n) * 8, "the filtered moments")) != SVGP_OK) return rc;
  if ((rc = h->work.reserve(ctx, ss_scan_work_doubles(n) * 8, "the scans' aggregates")) != SVGP_OK) return rc;
  if ((rc = h->part.reserve(ctx, 1024 * 8, "the lml's partial sums")) != SVGP_OK) return rc;
  return h->res.reserve(ctx, 8, "the lml");
}

int read_flag(svgp_ctx* ctx, svgp_ss* h, int* out) {
  HIPC(ctx, hipMemcpyAsync(out, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  return SVGP_OK;
}

template <typename T> bool sorted_and_finite(const T* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(double(v[i])) || (i > 0 && v[i] < v[i - 1])) return false;
  return true;
}

}  // namespace

extern "C" {

int32_t svgp_ss_create(svgp_ctx* ctx, const svgp_data* data, svgp_ss** out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!data || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  *out = nullptr;
  if (data->d != 1) return fail(ctx, SVGP_UNSUPPORTED, "the state-space form needs one-dimensional inputs (d = 1)");
  if (ctx->comm) return fail(ctx, SVGP_UNSUPPORTED, "the state-space calls are local: the context has a communicator");
  if (data->n < 1) return fail(ctx, SVGP_INVALID_ARG, "empty data");
  if (data->n > kSsMaxPoints) return fail(ctx, SVGP_UNSUPPORTED, "more than 2^31 - 1 points");
  std::unique_ptr<svgp_ss> h(new (std::nothrow) svgp_ss());
  if (!h) return SVGP_OOM;
  h->data = data;
  h->dtype = data->dtype;
  h->device = ctx->device;
  h->es = data->dtype == SVGP_F64 ? 8 : 4;
  h->N = data->n;
  HIPC(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = h->flag.reserve(ctx, sizeof(int), "the checks' flag")) != SVGP_OK) return rc;
  HIPC(ctx, hipMemsetAsync(h->flag.p, 0, sizeof(int), ctx->stream));
  launch_ss_check_sorted(h->dtype, ctx->stream, data->x.p, h->N, h->flag.as<int>());
  KCHECK(ctx, "ss (sorted times)");
  int flag = 0;
  if ((rc = read_flag(ctx, h.get(), &flag)) != SVGP_OK) return rc;
  if (flag & 1) return fail(ctx, SVGP_INVALID_ARG, "a time stamp is not finite");
  if (flag & 2) return fail(ctx, SVGP_INVALID_ARG, "the time stamps must be non-decreasing (sort the data)");
  *out = h.release();
  return SVGP_OK;
}

int32_t svgp_ss_free(svgp_ctx* ctx, svgp_ss* h) {
  if (!h) return SVGP_OK;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  delete h;
  return SVGP_OK;
}

int32_t svgp_ss_set_noise(svgp_ctx* ctx, svgp_ss* h, const svgp_point_noise* pn) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = handle_checks(ctx, h);
  if (rc) return rc;
  if (pn && !pn->s) return fail(ctx, SVGP_INVALID_ARG, "null noise vector");
  if (pn && pn->on_device != 0 && pn->on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  if (pn && pn->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved must be 0");
  HIPC(ctx, hipSetDevice(ctx->device));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  h->have_fit = false;   // the cached points belonged to the earlier variances
  h->have_noise = false;
  if (!pn) return SVGP_OK;
  const size_t nb = size_t(h->N) * h->es;
  if ((rc = h->noise_s.reserve(ctx, nb, "the noise vector")) != SVGP_OK) return rc;
  HIPC(ctx, hipMemcpyAsync(h->noise_s.p, pn->s, nb, pn->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  h->have_noise = true;
  return SVGP_OK;
}

int32_t svgp_ss_fit(svgp_ctx* ctx, svgp_ss* h, const svgp_ss_desc* desc, const double* delta, double* lml_out, svgp_ss_info* info) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = handle_checks(ctx, h);
  if (rc) return rc;
  if (!lml_out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if ((rc = check_desc(ctx, h, desc)) != SVGP_OK) return rc;
  if (!delta && !h->data->y.p) return fail(ctx, SVGP_INVALID_ARG, "the data have no y and no delta is given");
  *lml_out = std::numeric_limits<double>::quiet_NaN();
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = h->N;
  h->have_fit = false;
  for (DevBuf* b : {&h->t, &h->dl, &h->r})
    if ((rc = b->reserve(ctx, size_t(N) * 8, "the staged points")) != SVGP_OK) return rc;
  if ((rc = reserve_scan(ctx, h, N)) != SVGP_OK) return rc;
  if (delta) {
    if ((rc = h->delta.reserve(ctx, size_t(N) * 8, "delta")) != SVGP_OK) return rc;
    HIPC(ctx, hipMemcpyAsync(h->delta.p, delta, size_t(N) * 8, hipMemcpyHostToDevice, s));
  }
  TREC(ctx, ctx->ev[0], s);
  HIPC(ctx, hipMemsetAsync(h->flag.p, 0, sizeof(int), s));
  launch_ss_stage(h->dtype, s, h->data->x.p, h->data->y.p, delta ? h->delta.as<double>() : nullptr, h->have_noise ? h->noise_s.p : nullptr, N,
                  desc->diag, desc->mean_const, h->t.as<double>(), h->dl.as<double>(), h->r.as<double>(), h->flag.as<int>());
  launch_ss_filter(s, desc->kernel, desc->variance, desc->inv_lengthscale, h->t.as<double>(), h->dl.as<double>(), h->r.as<double>(), N,
                   h->work.as<double>(), h->fm.as<double>(), N);
  launch_ss_lml(s, desc->kernel, desc->variance, desc->inv_lengthscale, h->t.as<double>(), h->dl.as<double>(), h->r.as<double>(), N,
                h->fm.as<double>(), N, h->part.as<double>(), h->res.as<double>());
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "ss (fit)");
  double lml = 0;
  int flag = 0;
  HIPC(ctx, hipMemcpyAsync(&lml, h->res.p, 8, hipMemcpyDeviceToHost, s));
  if ((rc = read_flag(ctx, h, &flag)) != SVGP_OK) return rc;
  float ms = 0;
  (void)elapsed_ms(ctx, &ms, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_total = ms;
  if (flag & 4) return fail(ctx, SVGP_NOT_POSDEF, "per-point noise: a variance diag + s_i is not > 0");
  h->family = desc->kernel;
  h->variance = desc->variance;
  h->inv_lengthscale = desc->inv_lengthscale;
  h->mean_const = desc->mean_const;
  h->have_fit = true;
  *lml_out = lml;
  if (info) {
    *info = svgp_ss_info{};
    info->state_dim = desc->kernel == SVGP_KERNEL_MATERN32 ? 2 : 3;
    info->levels = ss_scan_levels(N);
    info->n_tiles = (N + ss_tile() - 1) / ss_tile();
    info->lml = lml;
    info->ms_total = ms;
  }
  return SVGP_OK;
}

int32_t svgp_ss_predict(svgp_ctx* ctx, svgp_ss* h, int64_t n, const void* t_host, void* mean_out, void* var_out) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = handle_checks(ctx, h);
  if (rc) return rc;
  if (!t_host) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!mean_out && !var_out) return fail(ctx, SVGP_INVALID_ARG, "null argument: neither mean nor var is asked for");
  if (!h->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_ss_fit on this handle yet");
  if (n < 1) return fail(ctx, SVGP_INVALID_ARG, "no test points");
  if (n > kSsMaxPoints - h->N) return fail(ctx, SVGP_UNSUPPORTED, "more than 2^31 - 1 points in the union of data and test points");
  const bool ok = h->dtype == SVGP_F64 ? sorted_and_finite(static_cast<const double*>(t_host), n) : sorted_and_finite(static_cast<const float*>(t_host), n);
  if (!ok) return fail(ctx, SVGP_INVALID_ARG, "the test times must be finite and non-decreasing (sort them)");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = h->N, U = N + n;
  const size_t nb = size_t(n) * h->es;
  if ((rc = h->ts.reserve(ctx, nb, "the test times")) != SVGP_OK) return rc;
  if ((rc = h->out.reserve(ctx, 2 * nb, "the predictions")) != SVGP_OK) return rc;
  for (DevBuf* b : {&h->tm, &h->dm, &h->rm})
    if ((rc = b->reserve(ctx, size_t(U) * 8, "the union of data and test points")) != SVGP_OK) return rc;
  if ((rc = h->slot.reserve(ctx, size_t(U) * sizeof(int), "the test points' slots")) != SVGP_OK) return rc;
  if ((rc = reserve_scan(ctx, h, U)) != SVGP_OK) return rc;
  HIPC(ctx, hipMemcpyAsync(h->ts.p, t_host, nb, hipMemcpyHostToDevice, s));
  TREC(ctx, ctx->ev[0], s);
  launch_ss_merge(h->dtype, s, h->t.as<double>(), h->dl.as<double>(), h->r.as<double>(), N, h->ts.p, n, h->tm.as<double>(), h->dm.as<double>(),
                  h->rm.as<double>(), h->slot.as<int>());
  launch_ss_filter(s, h->family, h->variance, h->inv_lengthscale, h->tm.as<double>(), h->dm.as<double>(), h->rm.as<double>(), U,
                   h->work.as<double>(), h->fm.as<double>(), U);
  void* mo = mean_out ? h->out.p : nullptr;
  void* vo = var_out ? static_cast<char*>(h->out.p) + nb : nullptr;
  launch_ss_smooth(s, h->family, h->variance, h->inv_lengthscale, h->tm.as<double>(), U, h->fm.as<double>(), U, h->work.as<double>(),
                   h->slot.as<int>(), h->mean_const, h->dtype, mo, vo);
  TREC(ctx, ctx->ev[1], s);
  KCHECK(ctx, "ss (predict)");
  if (mean_out) HIPC(ctx, hipMemcpyAsync(mean_out, mo, nb, hipMemcpyDeviceToHost, s));
  if (var_out) HIPC(ctx, hipMemcpyAsync(var_out, vo, nb, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  float ms = 0;
  (void)elapsed_ms(ctx, &ms, ctx->ev[0], ctx->ev[1]);
  ctx->timing = svgp_timing{};
  ctx->timing.ms_total = ms;
  return SVGP_OK;
}

int32_t svgp_ss_sample(svgp_ctx* ctx, svgp_ss* h, int64_t n, const void* t_host, int32_t n_samples, const double* z_host, const double* eps_host,
                       void* out) {
  if (!ctx) return SVGP_INVALID_ARG;
  int rc = handle_checks(ctx, h);
  if (rc) return rc;
  if (!t_host || !z_host || !eps_host || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!h->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_ss_fit on this handle yet");
  if (n < 1) return fail(ctx, SVGP_INVALID_ARG, "no test points");
  if (n_samples < 1) return fail(ctx, SVGP_INVALID_ARG, "n_samples must be >= 1");
  if (n > kSsMaxPoints - h->N) return fail(ctx, SVGP_UNSUPPORTED, "more than 2^31 - 1 points in the union of data and test points");
  const bool ok = h->dtype == SVGP_F64 ? sorted_and_finite(static_cast<const double*>(t_host), n) : sorted_and_finite(static_cast<const float*>(t_host), n);
  if (!ok) return fail(ctx, SVGP_INVALID_ARG, "the test times must be finite and non-decreasing (sort them)");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = h->N, U = N + n, S = n_samples;
  const int D = h->family == SVGP_KERNEL_MATERN32 ? 2 : 3, SC = ss_sample_chunk();
  // a group of whole chunks whose draws and intermediates fit kSsSampleGroupBytes (one chunk at least)
  const size_t stride = ss_sample_work_doubles(U);
  const size_t per_sample = (size_t(U) * size_t(2 * D + 1) + size_t(N)) * 8 + size_t(n) * h->es;
  const size_t per_chunk = per_sample * size_t(SC) + stride * 8;
  const int64_t chunks = (S + SC - 1) / SC;
  const int64_t gchunks = std::min<int64_t>(chunks, std::max<int64_t>(1, int64_t(kSsSampleGroupBytes / per_chunk)));
  const int64_t G = std::min<int64_t>(S, gchunks * SC);   // samples per group
  const size_t nb = size_t(n) * h->es;
  if ((rc = h->ts.reserve(ctx, nb, "the test times")) != SVGP_OK) return rc;
  for (DevBuf* b : {&h->tm, &h->dm, &h->rm})
    if ((rc = b->reserve(ctx, size_t(U) * 8, "the union of data and test points")) != SVGP_OK) return rc;
  if ((rc = h->slot.reserve(ctx, size_t(U) * sizeof(int), "the test points' slots")) != SVGP_OK) return rc;
  if ((rc = h->ident.reserve(ctx, size_t(U) * sizeof(int), "the points' identities")) != SVGP_OK) return rc;
  if ((rc = reserve_scan(ctx, h, U)) != SVGP_OK) return rc;
  if ((rc = h->sz.reserve(ctx, size_t(G) * size_t(U) * size_t(D) * 8, "the state draws")) != SVGP_OK) return rc;
  if ((rc = h->seps.reserve(ctx, size_t(G) * size_t(N) * 8, "the noise draws")) != SVGP_OK) return rc;
  if ((rc = h->sft.reserve(ctx, size_t(G) * size_t(U) * 8, "the prior paths")) != SVGP_OK) return rc;
  if ((rc = h->smf.reserve(ctx, size_t(G) * size_t(U) * size_t(D) * 8, "the residuals' filtered means")) != SVGP_OK) return rc;
  if ((rc = h->swork.reserve(ctx, size_t(gchunks) * stride * 8, "the sampler's aggregates")) != SVGP_OK) return rc;
  if ((rc = h->sout.reserve(ctx, size_t(G) * nb, "the sample paths")) != SVGP_OK) return rc;
  HIPC(ctx, hipMemcpyAsync(h->ts.p, t_host, nb, hipMemcpyHostToDevice, s));
  SsSample a{};
  a.t = h->tm.as<double>(); a.dl = h->dm.as<double>(); a.r = h->rm.as<double>(); a.fm = h->fm.as<double>();
  a.z = h->sz.as<double>(); a.eps = h->seps.as<double>();
  a.ident = h->ident.as<int>(); a.slot = h->slot.as<int>();
  a.ft = h->sft.as<double>(); a.mf = h->smf.as<double>(); a.work = h->swork.as<double>(); a.out = h->sout.p;
  a.n = U; a.N = N; a.nt = n;
  a.f32 = h->dtype == SVGP_F32;
  a.mean_const = h->mean_const;
  float ms_total = 0;
  for (int64_t g0 = 0; g0 < S; g0 += G) {
    const int64_t ns = std::min<int64_t>(G, S - g0);
    HIPC(ctx, hipMemcpyAsync(h->sz.p, z_host + size_t(g0) * size_t(U) * size_t(D), size_t(ns) * size_t(U) * size_t(D) * 8, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(h->seps.p, eps_host + size_t(g0) * size_t(N), size_t(ns) * size_t(N) * 8, hipMemcpyHostToDevice, s));
    TREC(ctx, ctx->ev[0], s);
    if (g0 == 0) {   // the union, its filtered covariances (they do not depend on the data or the draws) and the points' identities: once
      launch_ss_merge(h->dtype, s, h->t.as<double>(), h->dl.as<double>(), h->r.as<double>(), N, h->ts.p, n, h->tm.as<double>(), h->dm.as<double>(),
                      h->rm.as<double>(), h->slot.as<int>());
      launch_ss_filter(s, h->family, h->variance, h->inv_lengthscale, h->tm.as<double>(), h->dm.as<double>(), h->rm.as<double>(), U,
                       h->work.as<double>(), h->fm.as<double>(), U);
      launch_ss_ident(h->dtype, s, h->tm.as<double>(), h->slot.as<int>(), h->ts.p, n, N, h->ident.as<int>());
    }
    a.ns = int(ns);
    launch_ss_sample(s, h->family, h->variance, h->inv_lengthscale, a);
    TREC(ctx, ctx->ev[1], s);
    KCHECK(ctx, "ss (sample)");
    HIPC(ctx, hipMemcpyAsync(static_cast<char*>(out) + size_t(g0) * nb, h->sout.p, size_t(ns) * nb, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    float ms = 0;
    (void)elapsed_ms(ctx, &ms, ctx->ev[0], ctx->ev[1]);
    ms_total += ms;
  }
  ctx->timing = svgp_timing{};
  ctx->timing.ms_total = ms_total;   // the kernels of every group; the draws' uploads lie between the groups and are not counted
  return SVGP_OK;
}

}  // extern "C"
