// api.hip — the C-ABI of libsvgp_mi355x.so (include/svgp_mi355x.h), lifecycle part: contexts, models, data, the group calls.
// Host orchestration only, like its sibling units api_forward.hip / api_grad.hip / api_qopt.hip / api_predictive.hip (host.hpp
// declares what crosses them): every number is produced by the HIP kernels; there is no CPU compute path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/svgp_mi355x.h"
#include "host.hpp"

using namespace svgp;

namespace svgp {

// Golub–Welsch: nodes/weights of the n-point Gauss–Hermite rule (weight exp(-x²)), as
// FastGaussQuadrature.gausshermite(n).  Symmetric tridiagonal QL with implicit shifts on the Jacobi matrix.
int gauss_hermite(int n, double* xs, double* ws) {
  if (n < 1 || n > 512) return SVGP_INVALID_ARG;
  std::vector<double> d(n, 0.0), e(n, 0.0), z(n, 0.0);
  for (int i = 1; i < n; ++i) e[i - 1] = std::sqrt(0.5 * i);
  z[0] = 1.0;  // first row of the eigenvector matrix
  for (int l = 0; l < n; ++l) {
    int iter = 0, m;
    do {
      for (m = l; m < n - 1; ++m) {
        const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
        if (std::fabs(e[m]) <= 2.3e-16 * dd) break;
      }
      if (m != l) {
        if (++iter > 200) return SVGP_INVALID_ARG;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = std::hypot(g, 1.0);
        g = d[m] - d[l] + e[l] / (g + (g >= 0 ? std::fabs(r) : -std::fabs(r)));
        double s = 1.0, c = 1.0, p = 0.0;
        int i;
        for (i = m - 1; i >= l; --i) {
          double f = s * e[i], b = c * e[i];
          r = std::hypot(f, g);
          e[i + 1] = r;
          if (r == 0.0) {
            d[i + 1] -= p;
            e[m] = 0.0;
            break;
          }
          s = f / r;
          c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * b;
          p = s * r;
          d[i + 1] = g + p;
          g = c * r - b;
          f = z[i + 1];
          z[i + 1] = s * z[i] + c * f;
          z[i] = c * z[i] - s * f;
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p;
        e[l] = g;
        e[m] = 0.0;
      }
    } while (m != l);
  }
  // sort ascending
  std::vector<int> idx(n);
  for (int i = 0; i < n; ++i) idx[i] = i;
  for (int i = 1; i < n; ++i) {
    int k = idx[i], j = i - 1;
    while (j >= 0 && d[idx[j]] > d[k]) {
      idx[j + 1] = idx[j];
      --j;
    }
    idx[j + 1] = k;
  }
  const double mu0 = 1.7724538509055160273;  // sqrt(pi)
  for (int i = 0; i < n; ++i) {
    xs[i] = d[idx[i]];
    ws[i] = mu0 * z[idx[i]] * z[idx[i]];
  }
  // symmetrise (the rule is exactly symmetric)
  for (int i = 0; i < n / 2; ++i) {
    const double a = 0.5 * (xs[n - 1 - i] - xs[i]);
    xs[i] = -a;
    xs[n - 1 - i] = a;
    const double w = 0.5 * (ws[i] + ws[n - 1 - i]);
    ws[i] = ws[n - 1 - i] = w;
  }
  if (n % 2) xs[n / 2] = 0.0;
  return SVGP_OK;
}

}  // namespace svgp

namespace {

size_t esize(int dtype) { return dtype == SVGP_F64 ? 8 : 4; }

int validate_desc(svgp_ctx* ctx, const svgp_model_desc* d, bool need_q = true) {   // need_q false: d->m / d->Lq are not read (svgp_model_update_keep_q)
  if (!d) return fail(ctx, SVGP_INVALID_ARG, "null model descriptor");
  if (d->dtype != SVGP_F64 && d->dtype != SVGP_F32) return fail(ctx, SVGP_INVALID_ARG, "dtype must be SVGP_F64 or SVGP_F32");
  if (d->kernel < 0 || d->kernel > SVGP_KERNEL_MATERN52) return fail(ctx, SVGP_UNSUPPORTED, "unsupported kernel family");
  if (d->likelihood < 0 || d->likelihood > SVGP_LIK_BERNOULLI_NORMCDF) return fail(ctx, SVGP_UNSUPPORTED, "unsupported likelihood");
  if (d->parametrization != SVGP_NONCENTERED && d->parametrization != SVGP_CENTERED)
    return fail(ctx, SVGP_INVALID_ARG, "parametrization must be SVGP_NONCENTERED or SVGP_CENTERED");
  if (d->d < 1 || d->d > SVGP_MAX_D) return fail(ctx, SVGP_UNSUPPORTED, "input dimension must be in 1..64");
  if (d->M < 1) return fail(ctx, SVGP_INVALID_ARG, "M must be >= 1");
  if (d->layout_z < 0 || d->layout_z > SVGP_VEC) return fail(ctx, SVGP_INVALID_ARG, "bad layout_z");
  if (d->layout_z == SVGP_VEC && d->d != 1) return fail(ctx, SVGP_INVALID_ARG, "SVGP_VEC layout requires d == 1");
  if (d->quadrature_n < 0 || d->quadrature_n > 512) return fail(ctx, SVGP_INVALID_ARG, "quadrature_n must be in 0..512");
  if (!d->inv_lengthscale || !d->z || (need_q && (!d->m || !d->Lq))) return fail(ctx, SVGP_INVALID_ARG, "null parameter array");
  if (!(d->variance > 0)) return fail(ctx, SVGP_INVALID_ARG, "kernel variance must be positive");
  if (d->likelihood == SVGP_LIK_GAUSSIAN && !(d->lik_sigma2 > 0)) return fail(ctx, SVGP_INVALID_ARG, "Gaussian likelihood needs sigma2 > 0");
  if (d->likelihood == SVGP_LIK_GAMMA_EXP && !(d->lik_sigma2 > 0)) return fail(ctx, SVGP_INVALID_ARG, "Gamma likelihood needs shape alpha > 0");
  return SVGP_OK;
}

int effective_gh(const svgp_model_desc& d) {
  if (d.quadrature_n > 0) return d.quadrature_n;
  if (d.likelihood != SVGP_LIK_BERNOULLI_LOGISTIC && d.likelihood != SVGP_LIK_BERNOULLI_NORMCDF) return 0;  // closed forms [GPLikelihoods AnalyticExpectation]
  return 20;  // DefaultExpectationMethod -> GaussHermiteExpectation(20)  [GPLikelihoods]
}

int upload_params(svgp_ctx* ctx, svgp_model* m, const svgp_model_desc* d, bool keep_q = false) {   // keep_q: the device-resident m / Lq stay
  const size_t es = m->es;
  m->desc = *d;
  m->invl_host.assign(d->inv_lengthscale, d->inv_lengthscale + d->d);
  m->desc.inv_lengthscale = m->invl_host.data();
  m->desc.z = m->desc.m = m->desc.Lq = nullptr;  // host pointers are borrowed for the call only
  HIPC(ctx, hipMemcpyAsync(m->z_raw.p, d->z, size_t(m->M) * m->d * es, hipMemcpyHostToDevice, ctx->stream));
  if (!keep_q) {
    HIPC(ctx, hipMemcpyAsync(m->m_raw.p, d->m, size_t(m->M) * es, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(m->Lq_raw.p, d->Lq, size_t(m->M) * m->M * es, hipMemcpyHostToDevice, ctx->stream));
  }
  if (m->dtype == SVGP_F64) {
    HIPC(ctx, hipMemcpyAsync(m->invl.p, m->invl_host.data(), m->d * 8, hipMemcpyHostToDevice, ctx->stream));
  } else {
    std::vector<float> f(m->invl_host.begin(), m->invl_host.end());
    HIPC(ctx, hipMemcpyAsync(m->invl.p, f.data(), m->d * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
  }
  const int gh = effective_gh(*d);
  if (gh != m->gh_n) {   // gh_n names the rule on the device only once both arrays hold it: a failure leaves 0 and no arrays
    m->gh_x.release();
    m->gh_w.release();
    m->gh_n = 0;
    if (gh > 0) {
      std::vector<double> xs(gh), ws(gh);
      if (gauss_hermite(gh, xs.data(), ws.data()) != SVGP_OK) return fail(ctx, SVGP_INVALID_ARG, "Gauss-Hermite rule failed to converge");
      for (auto& w : ws) w /= 1.7724538509055160273;
      hipError_t e = m->gh_x.alloc(gh * 8);
      if (e == hipSuccess) e = m->gh_w.alloc(gh * 8);
      if (e == hipSuccess) e = hipMemcpy(m->gh_x.p, xs.data(), gh * 8, hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipMemcpy(m->gh_w.p, ws.data(), gh * 8, hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        m->gh_x.release();
        m->gh_w.release();
        return fail(ctx, e == hipErrorOutOfMemory ? SVGP_OOM : SVGP_HIP_ERROR, std::string("upload of the Gauss-Hermite rule: ") + hipGetErrorString(e));
      }
    }
    m->gh_n = gh;
  }
  HIPC(ctx, hipStreamSynchronize(ctx->stream));  // host buffers may be released by the caller
  m->prepared = false;
  return SVGP_OK;
}

}  // namespace

namespace svgp {

int make_data(svgp_ctx* ctx, int dtype, int layout, int d, int64_t n, const void* x_host, const void* y_host,
              svgp_data** out) {
  if (!out) return fail(ctx, SVGP_INVALID_ARG, "null out pointer");
  if (dtype != SVGP_F64 && dtype != SVGP_F32) return fail(ctx, SVGP_INVALID_ARG, "bad dtype");
  if (d > SVGP_MAX_D) return fail(ctx, SVGP_UNSUPPORTED, "input dimension beyond SVGP_MAX_D");   // as the model: the host falls back
  if (d < 1 || n < 1 || !x_host) return fail(ctx, SVGP_INVALID_ARG, "bad data shape");
  if (layout < 0 || layout > SVGP_VEC || (layout == SVGP_VEC && d != 1)) return fail(ctx, SVGP_INVALID_ARG, "bad layout");
  const size_t es = esize(dtype);
  std::unique_ptr<svgp_data> D(new (std::nothrow) svgp_data());
  if (!D) return SVGP_OOM;
  D->dtype = dtype;
  D->d = d;
  D->n = n;
  D->ldx = n;
  hipStream_t s = ctx->stream;
  hipError_t e = D->x.alloc(size_t(n) * d * es);
  if (e == hipSuccess && y_host) e = D->y.alloc(size_t(n) * es);
  if (e != hipSuccess) return alloc_failed(ctx, "for data");
  if (layout == SVGP_COLVECS && d > 1) {
    DevBuf tmp;
    HIPC(ctx, tmp.alloc(size_t(n) * d * es));
    HIPC(ctx, hipMemcpyAsync(tmp.p, x_host, size_t(n) * d * es, hipMemcpyHostToDevice, s));
    launch_transpose_colvecs(dtype, s, tmp.p, d, n, D->ldx, D->x.p);
    HIPC(ctx, hipStreamSynchronize(s));
  } else {
    HIPC(ctx, hipMemcpyAsync(D->x.p, x_host, size_t(n) * d * es, hipMemcpyHostToDevice, s));
  }
  if (y_host) HIPC(ctx, hipMemcpyAsync(D->y.p, y_host, size_t(n) * es, hipMemcpyHostToDevice, s));
  HIPC(ctx, hipStreamSynchronize(s));
  *out = D.release();
  return SVGP_OK;
}

}  // namespace svgp

// ================================================================================================
extern "C" {

int32_t svgp_version(void) { return SVGP_ABI_VERSION; }

int32_t svgp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t svgp_gausshermite(int32_t n, double* nodes_out, double* weights_out) {
  if (!nodes_out || !weights_out) return SVGP_INVALID_ARG;
  return gauss_hermite(n, nodes_out, weights_out);
}

// work(n, M, d) of one evaluation in host flops (2 M^2 n for trsm + trmm, M^3 / 3 for the Cholesky, plus
// the Kuf assembly and the elementwise reductions the reference materialises, ~ (3 d + 30) per element of Kuf)
double svgp_offload_work(int64_t n, int64_t M, int32_t d) {
  if (n < 0 || M < 0 || d < 0) return 0.0;
  const double nd = double(n), Md = double(M);
  return nd * Md * (2.0 * Md + 3.0 * double(d) + 30.0) + Md * Md * Md / 3.0;
}

int32_t svgp_offload_advice(int64_t n, int64_t M, int32_t d, int32_t /*dtype*/, int32_t /*want_gradient*/) {
  // One threshold for both forms: the device floor of a value-and-gradient call is ~2.5x the forward floor (600 vs 250 us
  // through the one-shot route), and so is the host's reverse-mode cost (profiles/round3/small_problems.md)
  const char* e = getenv("SVGP_OFFLOAD_MIN_WORK");   // read on every call: hosts (and the tests) change it at run time
  double min_work = 3.0e6;
  if (e && *e) {   // a value that does not parse as a non-negative number is ignored (atof gave 0 = "always offload")
    char* end = nullptr;
    const double v = strtod(e, &end);
    while (end && (*end == ' ' || *end == '\t')) ++end;
    if (end && end != e && *end == '\0' && v >= 0.0 && v == v) min_work = v;
  }
  return svgp_offload_work(n, M, d) >= min_work ? 1 : 0;
}

#ifdef SVGP_EXPERIMENTS
// only the experiments build (tools/build_experiments.sh) exports this: tools and tests tell the two libraries apart by it
int svgp_debug_experiments(void) { return 1; }
#endif

int32_t svgp_ctx_create(int32_t device_id, void* stream, svgp_ctx** out) {
  if (!out) return SVGP_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return SVGP_HIP_ERROR;  // no GPU: the library has no CPU path
  if (device_id < 0 || device_id >= n) return SVGP_INVALID_ARG;
  svgp_ctx* c = new (std::nothrow) svgp_ctx();
  if (!c) return SVGP_OOM;
  c->device = device_id;
  read_knobs(c->kn);   // the operational variables (knobs.hpp), once per context
  c->timing_on = c->kn.timing != 0;
  if (hipSetDevice(device_id) != hipSuccess) { delete c; return SVGP_HIP_ERROR; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->num_cus = prop.multiProcessorCount;
  if (stream) {
    c->stream.borrow(stream);
  } else if (c->stream.create(hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return SVGP_HIP_ERROR;
  }
  for (auto& e : c->ev)
    if (e.create(kTimingEvent) != hipSuccess) { delete c; return SVGP_HIP_ERROR; }
  for (auto& e : c->ev_chol)
    if (e.create(kTimingEvent) != hipSuccess) { delete c; return SVGP_HIP_ERROR; }
  if (c->d_res.alloc(16 * sizeof(double)) != hipSuccess || c->d_coll.alloc(8 * sizeof(double)) != hipSuccess || c->counter.alloc(64) != hipSuccess ||
      c->partial.alloc(1024 * sizeof(double)) != hipSuccess || c->negcnt.alloc(1024 * sizeof(unsigned)) != hipSuccess) { delete c; return SVGP_OOM; }
  *out = c;
  return SVGP_OK;
}

int32_t svgp_ctx_destroy(svgp_ctx* c) {
  if (!c) return SVGP_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  if (c->comm) (void)svgp_ctx_detach_comm(c);
  delete c->gws;
  delete c->cws;
  delete c;
  return SVGP_OK;
}

const char* svgp_last_error(const svgp_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// the v2 / v3 layout only (48 bytes): a host compiled against an older header sized its buffer for that
int32_t svgp_last_timing(const svgp_ctx* ctx, svgp_timing* out) {
  if (!ctx || !out) return SVGP_INVALID_ARG;
  static_assert(offsetof(svgp_timing, ms_chol) == SVGP_TIMING_V3_BYTES, "the fields appended since v3 start at byte 48");
  memcpy(out, &ctx->timing, SVGP_TIMING_V3_BYTES);
  return SVGP_OK;
}

int32_t svgp_last_timing_sized(const svgp_ctx* ctx, void* out, int64_t out_bytes) {
  if (!ctx || !out || out_bytes < 0) return SVGP_INVALID_ARG;
  const size_t n = size_t(out_bytes) < sizeof(svgp_timing) ? size_t(out_bytes) : sizeof(svgp_timing);
  memcpy(out, &ctx->timing, n);
  return SVGP_OK;
}

int32_t svgp_data_upload(svgp_ctx* ctx, int32_t dtype, int32_t layout, int32_t d, int64_t n, const void* x_host,
                         const void* y_host, svgp_data** out) {
  if (!ctx) return SVGP_INVALID_ARG;
  HIPC(ctx, hipSetDevice(ctx->device));
  return make_data(ctx, dtype, layout, d, n, x_host, y_host, out);
}

int32_t svgp_data_wrap_device(svgp_ctx* ctx, int32_t dtype, int32_t d, int64_t n, int64_t ldx, const void* x_dev,
                              const void* y_dev, svgp_data** out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (d > SVGP_MAX_D) return fail(ctx, SVGP_UNSUPPORTED, "input dimension beyond SVGP_MAX_D");
  if (!out || !x_dev || d < 1 || n < 1 || ldx < n) return fail(ctx, SVGP_INVALID_ARG, "bad wrap arguments");
  if (dtype != SVGP_F64 && dtype != SVGP_F32) return fail(ctx, SVGP_INVALID_ARG, "bad dtype");
  svgp_data* D = new (std::nothrow) svgp_data();
  if (!D) return SVGP_OOM;
  D->dtype = dtype;
  D->d = d;
  D->n = n;
  D->ldx = ldx;
  D->x.borrow(x_dev);
  D->y.borrow(y_dev);
  *out = D;
  return SVGP_OK;
}

int32_t svgp_data_free(svgp_ctx* ctx, svgp_data* D) {
  if (!D) return SVGP_OK;
  if (ctx) (void)hipSetDevice(ctx->device);
  delete D;
  return SVGP_OK;
}

int32_t svgp_model_free(svgp_ctx* ctx, svgp_model* m) {
  if (!m) return SVGP_OK;
  if (ctx) (void)hipSetDevice(ctx->device);
  delete m;
  return SVGP_OK;
}

int32_t svgp_model_create(svgp_ctx* ctx, const svgp_model_desc* desc, svgp_model** out) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!out) return fail(ctx, SVGP_INVALID_ARG, "null out pointer");
  *out = nullptr;
  int rc = validate_desc(ctx, desc);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  svgp_model* m = new (std::nothrow) svgp_model();
  if (!m) return SVGP_OOM;
  m->M = desc->M;
  m->Mp = (desc->M + 127) / 128 * 128;
  m->dtype = desc->dtype;
  m->d = desc->d;
  m->es = esize(desc->dtype);
  const size_t es = m->es, M = size_t(m->M), Mp = size_t(m->Mp);
  struct { DevBuf* b; size_t bytes; } allocs[] = {
      {&m->z_raw, M * m->d * es}, {&m->m_raw, M * es},     {&m->Lq_raw, M * M * es}, {&m->invl, size_t(m->d) * es},
      {&m->zs, Mp * m->d * es},   {&m->L, Mp * Mp * es},   {&m->T, Mp * Mp * es},    {&m->U, Mp * Mp * es},
      {&m->mp, Mp * es},          {&m->scal, (8 + Mp) * sizeof(double)},             {&m->info, info_bytes(Mp)},
      {&m->B, desc->parametrization == SVGP_CENTERED ? Mp * Mp * es : 0},
  };
  for (auto& a : allocs)
    if (a.bytes && a.b->alloc(a.bytes) != hipSuccess) {
      svgp_model_free(ctx, m);
      return alloc_failed(ctx, "for model buffers");
    }
  if (hipMemsetAsync(m->T.p, 0, Mp * Mp * es, ctx->stream) != hipSuccess) {   // launch_potrf's contract: T zero above the diagonal
    svgp_model_free(ctx, m);
    return fail(ctx, SVGP_HIP_ERROR, "hipMemsetAsync failed for the model's T buffer");
  }
  rc = upload_params(ctx, m, desc);
  if (rc) {
    svgp_model_free(ctx, m);
    return rc;
  }
  *out = m;
  return SVGP_OK;
}

int32_t svgp_model_update(svgp_ctx* ctx, svgp_model* m, const svgp_model_desc* desc) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!m) return fail(ctx, SVGP_INVALID_ARG, "null model");
  int rc = validate_desc(ctx, desc);
  if (rc) return rc;
  if (desc->M != m->M || desc->d != m->d || desc->dtype != m->dtype || desc->parametrization != m->desc.parametrization)
    return fail(ctx, SVGP_INVALID_ARG, "svgp_model_update: M, d, dtype and parametrization must not change");
  HIPC(ctx, hipSetDevice(ctx->device));
  return upload_params(ctx, m, desc);
}

// svgp_model_update without the upload of q: desc->m / desc->Lq are ignored (they may be NULL), the device-resident q - what the model
// was created or last updated with, or what svgp_collapsed_q / svgp_natgrad_step wrote - stays
int32_t svgp_model_update_keep_q(svgp_ctx* ctx, svgp_model* m, const svgp_model_desc* desc) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!m) return fail(ctx, SVGP_INVALID_ARG, "null model");
  int rc = validate_desc(ctx, desc, false);
  if (rc) return rc;
  if (desc->M != m->M || desc->d != m->d || desc->dtype != m->dtype || desc->parametrization != m->desc.parametrization)
    return fail(ctx, SVGP_INVALID_ARG, "svgp_model_update_keep_q: M, d, dtype and parametrization must not change");
  HIPC(ctx, hipSetDevice(ctx->device));
  return upload_params(ctx, m, desc, true);
}

}  // extern "C"

// ================================================================================================
// One process, several GPUs (the shape of a Julia host): the group's member contexts each hold one shard of the data and
// a replica of the model; an evaluation enqueues every device, then issues the members' all-reduces as ONE ncclGroup,
// then reads device 0.  Same kernels, same collective, same result as the process-per-GPU path.
extern "C" {

int32_t svgp_group_data_upload(svgp_group* g, int32_t dtype, int32_t layout, int32_t d, int64_t n, const void* x_host,
                               const void* y_host, svgp_data** shards_out) {
  if (!g || !shards_out || !x_host || n < int64_t(g->ctxs.size())) return SVGP_INVALID_ARG;
  if (dtype != SVGP_F64 && dtype != SVGP_F32) return SVGP_INVALID_ARG;
  const int W = int(g->ctxs.size());
  const size_t es = esize(dtype);
  for (int i = 0; i < W; ++i) shards_out[i] = nullptr;
  int rc = SVGP_OK;
  for (int i = 0; i < W && rc == SVGP_OK; ++i) {
    // contiguous shard [lo, hi): the first n % W members get one more point
    const int64_t base = n / W, rem = n % W, lo = i * base + (i < rem ? i : rem), cnt = base + (i < rem ? 1 : 0);
    const char* xp = static_cast<const char*>(x_host);
    const char* yp = static_cast<const char*>(y_host);
    std::vector<char> gather;
    const void* xs = nullptr;
    if (layout == SVGP_ROWVECS && d > 1) {   // n x d column-major: a shard's rows are strided; gather them
      gather.resize(size_t(cnt) * d * es);
      for (int f = 0; f < d; ++f) memcpy(gather.data() + size_t(f) * cnt * es, xp + (size_t(f) * n + lo) * es, size_t(cnt) * es);
      xs = gather.data();
    } else {
      xs = xp + size_t(lo) * (layout == SVGP_COLVECS ? d : 1) * es;
    }
    rc = svgp_data_upload(g->ctxs[size_t(i)], dtype, layout, d, cnt, xs, yp ? yp + size_t(lo) * es : nullptr, &shards_out[i]);
    if (rc) g->err = svgp_last_error(g->ctxs[size_t(i)]);
  }
  if (rc != SVGP_OK)
    for (int i = 0; i < W; ++i) {
      svgp_data_free(g->ctxs[size_t(i)], shards_out[i]);
      shards_out[i] = nullptr;
    }
  return rc;
}

int32_t svgp_group_model_create(svgp_group* g, const svgp_model_desc* desc, svgp_model** models_out) {
  if (!g || !models_out) return SVGP_INVALID_ARG;
  const int W = int(g->ctxs.size());
  for (int i = 0; i < W; ++i) models_out[i] = nullptr;
  int rc = SVGP_OK;
  for (int i = 0; i < W && rc == SVGP_OK; ++i) {
    rc = svgp_model_create(g->ctxs[size_t(i)], desc, &models_out[i]);
    if (rc) g->err = svgp_last_error(g->ctxs[size_t(i)]);
  }
  if (rc != SVGP_OK)
    for (int i = 0; i < W; ++i) {
      svgp_model_free(g->ctxs[size_t(i)], models_out[i]);
      models_out[i] = nullptr;
    }
  return rc;
}

int32_t svgp_group_model_update(svgp_group* g, svgp_model* const* models, const svgp_model_desc* desc) {
  if (!g || !models) return SVGP_INVALID_ARG;
  for (size_t i = 0; i < g->ctxs.size(); ++i) {
    const int rc = svgp_model_update(g->ctxs[i], models[i], desc);
    if (rc) { g->err = svgp_last_error(g->ctxs[i]); return rc; }
  }
  return SVGP_OK;
}

const char* svgp_group_last_error(const svgp_group* g) { return g ? g->err.c_str() : "null group"; }

// elbo over the members' batches: member i evaluates points [offs[i], offs[i] + lens[i]) of shards[i]
int32_t svgp_group_elbo(svgp_group* g, svgp_model* const* models, const svgp_data* const* shards, const int64_t* offs,
                        const int64_t* lens, double num_data, double* elbo_out, svgp_terms* terms_out) {
  if (!g || !models || !shards || !offs || !lens) return SVGP_INVALID_ARG;
  const size_t W = g->ctxs.size();
  std::vector<int> rcs(W, SVGP_OK);
  // one process knows every member: a member that cannot take part is found BEFORE anything is enqueued and nothing touches
  // the communicator (a failing member used to leave the others' all-reduces waiting for it inside one ncclGroup)
  for (size_t i = 0; i < W; ++i) {
    const int rci = check_batch(g->ctxs[i], models[i], shards[i], offs[i], lens[i], true);
    if (rci != SVGP_OK) { g->err = svgp_last_error(g->ctxs[i]); return rci; }
  }
  for (size_t i = 0; i < W; ++i) rcs[i] = elbo_enqueue(g->ctxs[i], models[i], shards[i], offs[i], lens[i]);
  int rc = comm_group_start(g->ctxs[0]);
  if (rc == SVGP_OK) {
    for (size_t i = 0; i < W; ++i) rcs[i] = elbo_collective(g->ctxs[i], rcs[i]);
    rc = comm_group_end(g->ctxs[0]);
  }
  ElboRead r0;
  for (size_t i = 0; i < W; ++i) {
    ElboRead r;
    if (rcs[i] == SVGP_OK) rcs[i] = elbo_finish(g->ctxs[i], models[i], &r);
    if (i == 0) r0 = r;
    if (rcs[i] != SVGP_OK && rc == SVGP_OK) { rc = rcs[i]; g->err = svgp_last_error(g->ctxs[i]); }
  }
  if (rc != SVGP_OK) return rc;
  svgp_model* m = models[0];
  const double scale = (num_data > 0 ? num_data : r0.n_points) / r0.n_points;
  const double elbo = r0.E * scale - m->kl;
  fill_terms(terms_out, m, elbo, r0, scale);
  rc = status_of(g->ctxs[0], m, r0.n_neg, r0.bad_chol, r0.failed);
  if (rc) g->err = svgp_last_error(g->ctxs[0]);
  if (elbo_out) *elbo_out = (rc == SVGP_OK) ? elbo : NAN;
  return rc;
}

// value and gradient of the same global ELBO; the host knows the global batch size, so only the final grouped all-reduce runs
int32_t svgp_group_elbo_grad(svgp_group* g, svgp_model* const* models, const svgp_data* const* shards, const int64_t* offs,
                             const int64_t* lens, double num_data, double* elbo_out, svgp_terms* terms_out,
                             svgp_grads* grads_out) {
  if (!g || !models || !shards || !offs || !lens || !grads_out) return SVGP_INVALID_ARG;
  const size_t W = g->ctxs.size();
  int64_t n_global = 0;
  for (size_t i = 0; i < W; ++i) n_global += lens[i];
  if (n_global < 1) return SVGP_INVALID_ARG;
  std::vector<int> rcs(W, SVGP_OK);
  std::vector<GradCall> gcs(W);
  // validate EVERY member (arguments and gradient workspace) before anything is enqueued: if one cannot join, no member
  // issues a collective and the error is returned with the communicator untouched (the others used to hang)
  for (size_t i = 0; i < W; ++i) {
    int rci = check_batch(g->ctxs[i], models[i], shards[i], offs[i], lens[i], true);
    if (rci == SVGP_OK && hipSetDevice(g->ctxs[i]->device) != hipSuccess) rci = fail(g->ctxs[i], SVGP_HIP_ERROR, "hipSetDevice failed");
    if (rci == SVGP_OK) rci = grad_workspace(g->ctxs[i], models[i], lens[i], &gcs[i].w);
    if (rci != SVGP_OK) { g->err = svgp_last_error(g->ctxs[i]); return rci; }
  }
  for (size_t i = 0; i < W; ++i) {
    GradCall& gc = gcs[i];
    gc.scale = (num_data > 0 ? num_data : double(n_global)) / double(n_global);
    gc.klw = 1.0 / double(W);
    gc.num_data = num_data;
    gc.collective = false;   // scale known on the host: no batch-size all-reduce
    rcs[i] = grad_enqueue(g->ctxs[i], models[i], shards[i], offs[i], lens[i], gc);
    gc.collective = true;    // ... but the final reduction and the global bookkeeping of grad_finish apply
  }
  int rc = comm_group_start(g->ctxs[0]);
  if (rc == SVGP_OK) {
    for (size_t i = 0; i < W; ++i) rcs[i] = grad_collective(g->ctxs[i], models[i], gcs[i], rcs[i]);
    rc = comm_group_end(g->ctxs[0]);
  }
  svgp_grads scratch{};   // members other than 0 only need their status
  for (size_t i = 0; i < W; ++i) {
    if (rcs[i] == SVGP_OK) {
      svgp_grads* out = (i == 0) ? grads_out : &scratch;
      rcs[i] = grad_finish(g->ctxs[i], models[i], gcs[i], i == 0 ? elbo_out : nullptr, i == 0 ? terms_out : nullptr, out);
    }
    if (rcs[i] != SVGP_OK && rc == SVGP_OK) { rc = rcs[i]; g->err = svgp_last_error(g->ctxs[i]); }
  }
  return rc;
}

}  // extern "C"
