// collapsed.hip — the collapsed (Titsias 2009, eqs. 11 / 12) bound of sparse GP regression and the optimal q(u): the kernels that are
// NOT the data pass (strip.hip: trsm_pm_kernel gives A = Lk \ Kuf point-major and sum A^2 per point; grad.hip: syrk_async_kernel gives
// C = A A').  api_qopt.hip: collapsed_run is the schedule.  The reference builds the same q on the host (test/test_utils.jl:7-17,
// optimal_variational_posterior) and compares it with AbstractGPs' VFE posterior (test/SparseVariationalApproximationModule.jl:99-134).
//   data-sized   b = A r, rr = r'r, t = sum_j |A_j|^2 over the resident point-major chunk          collapsed_reduce_kernel
//                with per-point noise / prior mean offsets (svgp_collapsed_*_with_noise):
//                w_j = 1 / (sigma^2 + s_j) for the window, the count of sigma_j^2 <= 0               collapsed_weights_kernel
//                b = A (w r), rr = sum w r^2, sum w |A_j|^2, sum w, sum log sigma_j^2; r reads mux    collapsed_reduce_w_kernel
//                the gradient pass's point stage with sigma_j^2: g_mu, g_v, s_bar, mux_bar           collapsed_point_grad_kernel
//   M-sized      B = I + C / sigma^2 (fp64, from the SYRK's slices), c~ = b / sigma^2              collapsed_form_b_kernel
//                cholesky(B), c = LB \ c~, m_w = LB' \ c, B^-1 = LBinv' LBinv, cholesky(B^-1)      prep.hip / grad.hip launchers, fp64
//                sum log diag LB, c'c                                                              collapsed_scal_kernel
//                q in the model's parametrisation and layout                                       collapsed_write_q_kernel
// The M-sized tail runs in fp64 whatever the model's dtype: cond(B) = 1 + lambda_max(C) / sigma^2 grows with the number of points
// (~ n variance / sigma^2: 1e7 at n = 1e6), so eps_fp32 cond(B) reaches 1 long before the headline size.
// Every sum has a fixed split and a fixed order: results are bitwise repeatable, no floating-point atomics.
#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {
namespace {

// bpart[s][k] (+)= sum_{j in split s} A_kj r_j,  spart[s] (+)= {sum r_j^2, sum ssq_j} over the same points; r_j = y_j - mean_const.
// At point-major [n][Mp]: a thread owns one k, a workgroup 128 consecutive k (coalesced rows), gridDim.y = kCollapsedSplit splits of
// the chunk's n points.  first: overwrite (the first chunk of a call), else add to what the previous chunks left - the chunks follow
// each other on one stream, so the order of the additions is fixed.
template <typename T>
__global__ void __launch_bounds__(128) collapsed_reduce_kernel(const T* __restrict__ At, const T* __restrict__ y, const double* __restrict__ ssq,
                                                               int64_t Mp, int64_t off, int64_t n, double mean_const, int first,
                                                               double* __restrict__ bpart, double* __restrict__ spart) {
  const int64_t k = int64_t(blockIdx.x) * 128 + threadIdx.x;
  const int64_t per = (n + gridDim.y - 1) / gridDim.y;
  const int64_t j0 = int64_t(blockIdx.y) * per;
  int64_t j1 = j0 + per;
  j1 = j1 < n ? j1 : n;
  double acc = 0.0;
#pragma unroll 4
  for (int64_t j = j0; j < j1; ++j) acc = fma(double(At[j * Mp + k]), double(y[off + j]) - mean_const, acc);
  double* bp = bpart + int64_t(blockIdx.y) * Mp + k;
  *bp = first ? acc : *bp + acc;
  if (blockIdx.x == 0) {
    __shared__ double sh[2][128];
    double rr = 0.0, t = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 128) {
      const double r = double(y[off + j]) - mean_const;
      rr = fma(r, r, rr);
      t += ssq[j];
    }
    sh[0][threadIdx.x] = rr;
    sh[1][threadIdx.x] = t;
    __syncthreads();
    for (int w = 64; w > 0; w >>= 1) {
      if (int(threadIdx.x) < w) {
        sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
        sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
      }
      __syncthreads();
    }
    if (threadIdx.x < 2) {
      double* sp = spart + int64_t(blockIdx.y) * 2 + threadIdx.x;
      *sp = first ? sh[threadIdx.x][0] : *sp + sh[threadIdx.x][0];
    }
  }
}

// Per-point noise (svgp_collapsed_*_with_noise): sigma_j^2 = sigma2 + s[j] over the whole window, once per call.  w[j] = 1 / sigma_j^2 in
// the model's dtype (the weighted SYRK's operand) and in fp64 (wd: the reductions'), zeros from n up to pad_to (the SYRK reads the
// last chunk padded to 128 points); *nbad (zeroed by the host) counts sigma_j^2 <= 0 - an integer count, order-free.  A NaN s[j] is
// not counted: it travels through w into C, b and rr (NaN results, SVGP_OK).
template <typename T>
__global__ void __launch_bounds__(k256) collapsed_weights_kernel(const T* __restrict__ s, double sigma2, int64_t n, int64_t pad_to,
                                                                 T* __restrict__ w, double* __restrict__ wd, int* __restrict__ nbad) {
  const int64_t i = int64_t(blockIdx.x) * k256 + threadIdx.x;
  int bad = 0;
  if (i < n) {
    const double v = sigma2 + double(s[i]);
    bad = v <= 0.0 ? 1 : 0;
    const double wi = 1.0 / v;
    w[i] = T(wi);
    wd[i] = wi;
  } else if (i < pad_to) {
    w[i] = T(0);
    wd[i] = 0.0;
  }
  const int cnt = __syncthreads_count(bad);
  if (threadIdx.x == 0 && cnt != 0) atomicAdd(nbad, cnt);
}

// collapsed_reduce_kernel with a prior mean and weights: r_j = (y_j - mean_const) - mux[j] (mux nullable), w_j = wd[j] (nullable: 1).
//   bpart[s][k] (+)= sum_j A_kj w_j r_j,   spart[s] (+)= {sum w_j r_j^2, sum w_j ssq_j},   spart2[s] (+)= {sum log(sigma2 + s[j]), sum w_j}
// mux, sv, wd: the chunk's own elements (element j <-> point j of the chunk).  Same grid, splits and order as collapsed_reduce_kernel.
template <typename T>
__global__ void __launch_bounds__(128) collapsed_reduce_w_kernel(const T* __restrict__ At, const T* __restrict__ y, const T* __restrict__ mux,
                                                                 const T* __restrict__ sv, const double* __restrict__ wd,
                                                                 const double* __restrict__ ssq, int64_t Mp, int64_t off, int64_t n,
                                                                 double mean_const, double sigma2, int first, double* __restrict__ bpart,
                                                                 double* __restrict__ spart, double* __restrict__ spart2) {
  const int64_t k = int64_t(blockIdx.x) * 128 + threadIdx.x;
  const int64_t per = (n + gridDim.y - 1) / gridDim.y;
  const int64_t j0 = int64_t(blockIdx.y) * per;
  int64_t j1 = j0 + per;
  j1 = j1 < n ? j1 : n;
  double acc = 0.0;
#pragma unroll 4
  for (int64_t j = j0; j < j1; ++j) {
    double r = double(y[off + j]) - mean_const;
    if (mux) r -= double(mux[j]);
    if (wd) r *= wd[j];
    acc = fma(double(At[j * Mp + k]), r, acc);
  }
  double* bp = bpart + int64_t(blockIdx.y) * Mp + k;
  *bp = first ? acc : *bp + acc;
  if (blockIdx.x == 0) {
    __shared__ double sh[4][128];
    double rr = 0.0, t = 0.0, ld = 0.0, sw = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 128) {
      double r = double(y[off + j]) - mean_const;
      if (mux) r -= double(mux[j]);
      const double wj = wd ? wd[j] : 1.0;
      rr = fma(wj * r, r, rr);
      t = fma(wj, ssq[j], t);
      sw += wj;
      if (sv) ld += log(sigma2 + double(sv[j]));
    }
    sh[0][threadIdx.x] = rr;
    sh[1][threadIdx.x] = t;
    sh[2][threadIdx.x] = ld;
    sh[3][threadIdx.x] = sw;
    __syncthreads();
    for (int w = 64; w > 0; w >>= 1) {
      if (int(threadIdx.x) < w) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
      }
      __syncthreads();
    }
    if (threadIdx.x < 4) {
      double* sp = (threadIdx.x < 2 ? spart : spart2) + int64_t(blockIdx.y) * 2 + (threadIdx.x & 1);
      *sp = first ? sh[threadIdx.x][0] : *sp + sh[threadIdx.x][0];
    }
  }
}

// scal[6] = sum log sigma_j^2, scal[7] = sum w_j: the split partials of collapsed_reduce_w_kernel in split order (one workgroup)
__global__ void collapsed_extra_kernel(const double* __restrict__ spart2, int nsplit, double* __restrict__ scal) {
  if (threadIdx.x < 2) {
    double q = 0.0;
    for (int s = 0; s < nsplit; ++s) q += spart2[2 * s + threadIdx.x];
    scal[6 + threadIdx.x] = q;
  }
}

// The point stage of the gradient pass with per-point noise: point_grad_kernel (strip.hip) for the Gaussian likelihood in closed form,
// sigma_i^2 = sigma2 + noise[i] (noise nullable).  Same outputs, same per-block sums {E, sum g_mu, sum g_v, dE/dsigma2, n_neg} in the
// same fixed order (LDS tree), the same two fills riding along (the head of the strips' queue, the padding of g_mu | g_v), and
// noise_bar[i] = scale dE_i/dsigma_i^2 = scale (-1 / (2 sigma_i^2) + ((y_i - mu_i)^2 + v_i) / (2 sigma_i^4)) next to mux_bar (gmu_copy).
// A kernel of its own so that strip.hip - the strips' translation unit - is compiled exactly as before.
template <typename T>
__global__ void __launch_bounds__(k256) collapsed_point_grad_kernel(double sigma2, int clamp_neg_var, const double* __restrict__ mom_mu,
                                                                    const double* __restrict__ mom_var, const T* __restrict__ y, int64_t off,
                                                                    int64_t len, double scale, const T* __restrict__ noise,
                                                                    T* __restrict__ gmu_out, T* __restrict__ gv_out,
                                                                    double* __restrict__ part5, unsigned* __restrict__ strip_queue,
                                                                    int64_t pad_to, T* __restrict__ gmu_copy, T* __restrict__ noise_bar) {
  __shared__ double sh[5][k256];
  const int64_t i = int64_t(blockIdx.x) * k256 + threadIdx.x;
  if (strip_queue && blockIdx.x == 0 && threadIdx.x == 0) *strip_queue = 0u;
  if (i >= len && i < pad_to) { gmu_out[i] = T(0); gv_out[i] = T(0); }
  double e5[5] = {0, 0, 0, 0, 0};
  if (i < len) {
    const double mu = mom_mu[i];
    double v = mom_var[i] + kDefaultSigma2;                 // FiniteGP(f_post, x, 1e-18) -> marginals
    bool bad = v < 0.0;
    if (bad) {
      e5[4] = 1.0;
      if (clamp_neg_var) { v = 0.0; bad = false; }
    }
    if (!bad) {
      const double s2 = noise ? sigma2 + double(noise[i]) : sigma2;
      const double r = double(y[off + i]) - mu;
      e5[0] = -0.5 * (1.8378770664093453 + log(s2) + (r * r + v) / s2);
      e5[1] = r / s2 * scale;
      e5[2] = -0.5 / s2 * scale;
      e5[3] = -0.5 * (1.0 / s2 - (r * r + v) / (s2 * s2)) * scale;
    }
    gmu_out[i] = T(e5[1]);
    gv_out[i] = T(e5[2]);
    if (gmu_copy) gmu_copy[i] = T(e5[1]);     // mux_bar
    if (noise_bar) noise_bar[i] = T(e5[3]);   // s_bar
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) sh[q][threadIdx.x] = e5[q];
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) {
#pragma unroll
      for (int q = 0; q < 5; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 5) part5[int64_t(blockIdx.x) * 5 + threadIdx.x] = sh[threadIdx.x][0];
}

// Bm (fp64, Mp x Mp, full and exactly symmetric) = I + (sum of the SYRK's slices) / sigma^2: entry (r, c) reads the lower-tile entry
// (max, min) of every slice in slice order.  Row 0's workgroups also close the reductions: cvec[k] = sum_s bpart[s][k] / sigma^2,
// scal[0] = rr, scal[1] = t.
template <typename T>
__global__ void __launch_bounds__(k256) collapsed_form_b_kernel(const T* __restrict__ G, int nslices, int64_t Mp, double inv_sigma2,
                                                                const double* __restrict__ bpart, const double* __restrict__ spart, int nsplit,
                                                                double* __restrict__ Bm, double* __restrict__ cvec, double* __restrict__ scal) {
  const int64_t c = int64_t(blockIdx.x) * k256 + threadIdx.x, r = blockIdx.y;
  if (c >= Mp) return;
  const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
  double v = 0.0;
  for (int s = 0; s < nslices; ++s) v += double(G[int64_t(s) * Mp * Mp + hi * Mp + lo]);
  Bm[r * Mp + c] = (r == c ? 1.0 : 0.0) + v * inv_sigma2;
  if (r == 0) {
    double b = 0.0;
    for (int s = 0; s < nsplit; ++s) b += bpart[int64_t(s) * Mp + c];
    cvec[c] = b * inv_sigma2;
    if (c < 2) {
      double q = 0.0;
      for (int s = 0; s < nsplit; ++s) q += spart[2 * s + c];
      scal[c] = q;
    }
  }
}

// scal[2] = sum log diag LB, scal[3] = c'c, scal[4] = info of cholesky(B), scal[5] = info of cholesky(B^-1) (nullable), one workgroup
__global__ void __launch_bounds__(k256) collapsed_scal_kernel(const double* __restrict__ LB, const double* __restrict__ c, int64_t Mp,
                                                              const int* __restrict__ info_b, const int* __restrict__ info_s,
                                                              double* __restrict__ scal) {
  __shared__ double sh[2][k256];
  double ld = 0.0, cc = 0.0;
  for (int64_t i = threadIdx.x; i < Mp; i += k256) {
    ld += log(LB[i * (Mp + 1)]);
    cc = fma(c[i], c[i], cc);
  }
  sh[0][threadIdx.x] = ld;
  sh[1][threadIdx.x] = cc;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    scal[2] = sh[0][0];
    scal[3] = sh[1][0];
    scal[4] = double(*info_b);
    scal[5] = info_s ? double(*info_s) : 0.0;
  }
}

// *first_bad = 0, or the 1-based index of the first pivot of Lk (diagonal entry squared) at or below 4 eps (i + 1) kdiag, the rounding
// noise of kdiag - sum_k L_ik^2 in the model's dtype (kdiag = variance + jitter), or NaN.  cholesky(Kuu) itself reports only pivots
// <= 0, as LAPACK does; an exactly repeated inducing point at jitter 0 leaves +-1e-16 there, of either sign, and A = Lk \ Kuf built on
// such a pivot is noise.  One workgroup.
template <typename T>
__global__ void __launch_bounds__(k256) collapsed_pivot_check_kernel(const T* __restrict__ Lk, int64_t M, int64_t Mp, double kdiag,
                                                                     int* __restrict__ first_bad) {
  __shared__ int sh[k256];
  const double eps = sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-7;
  int bad = 0x7fffffff;
  for (int64_t i = threadIdx.x; i < M; i += k256) {
    const double l = double(Lk[i * (Mp + 1)]);
    if (!(l * l > 4.0 * eps * double(i + 1) * kdiag) && int(i + 1) < bad) bad = int(i + 1);
  }
  sh[threadIdx.x] = bad;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w && sh[threadIdx.x + w] < sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *first_bad = sh[0] == 0x7fffffff ? 0 : sh[0];
}

// The optimal q into the model's own arrays (user layout: m [M], Lq M x M column-major, upper triangle zeroed).
//   NonCentered: m = m_w, Lq = Lq_w;   Centered: m = mean_const + muz + Lk m_w, Lq = Lk Lq_w (lower triangular, positive diagonal);
//   muz (nullable, model dtype, [M]): the inducing points' prior mean offsets (svgp_collapsed_*_with_noise).
// Lqw: the fp64 factor of B^-1 (column-major, ld Mp, lower part valid); Lk: the model's factor (model dtype, column-major, ld Mp).
// Nothing is written when either factorisation failed (the model keeps its q); a NaN in the data sums (scal[0], scal[1]: a NaN
// coordinate or observation) writes NaN, as the reference's arithmetic would.  gridDim.y = M columns, threads along the rows.
template <typename T>
__global__ void __launch_bounds__(k256) collapsed_write_q_kernel(const double* __restrict__ Lqw, const double* __restrict__ mw,
                                                                 const T* __restrict__ Lk, int64_t M, int64_t Mp, int centered,
                                                                 double mean_const, const double* __restrict__ scal,
                                                                 const int* __restrict__ info_b, const int* __restrict__ info_s,
                                                                 const T* __restrict__ muz, T* __restrict__ m_out, T* __restrict__ Lq_out) {
  const int64_t i = int64_t(blockIdx.x) * k256 + threadIdx.x, j = blockIdx.y;
  if (i >= M) return;
  const bool nan_in = (scal[0] != scal[0]) || (scal[1] != scal[1]);
  if (!nan_in && (*info_b != 0 || *info_s != 0)) return;
  const double qnan = scal[0] + scal[1];   // NaN when nan_in
  double v = 0.0;
  if (i >= j) {
    if (!centered) {
      v = Lqw[i + j * Mp];
    } else {
      for (int64_t k = j; k <= i; ++k) v = fma(double(Lk[i + k * Mp]), Lqw[k + j * Mp], v);
    }
    if (nan_in) v = qnan;
  }
  Lq_out[i + j * M] = T(v);
  if (j == 0) {
    double mv = mw[i];
    if (centered) {
      mv = 0.0;
      for (int64_t k = 0; k <= i; ++k) mv = fma(double(Lk[i + k * Mp]), mw[k], mv);
      mv += mean_const;
      if (muz) mv += double(muz[i]);
    }
    m_out[i] = T(nan_in ? qnan : mv);
  }
}

}  // namespace

void launch_collapsed_reduce(int dtype, hipStream_t s, const void* At, const void* y, const double* ssq, int64_t Mp, int64_t off, int64_t n,
                             double mean_const, int first, double* bpart, double* spart) {
  const dim3 grid((unsigned)(Mp / 128), (unsigned)kCollapsedSplit);
  if (dtype == 0)
    hipLaunchKernelGGL(collapsed_reduce_kernel<double>, grid, dim3(128), 0, s, (const double*)At, (const double*)y, ssq, Mp, off, n, mean_const,
                       first, bpart, spart);
  else
    hipLaunchKernelGGL(collapsed_reduce_kernel<float>, grid, dim3(128), 0, s, (const float*)At, (const float*)y, ssq, Mp, off, n, mean_const,
                       first, bpart, spart);
}

void launch_collapsed_weights(int dtype, hipStream_t s, const void* sv, double sigma2, int64_t n, int64_t pad_to, void* w, double* wd, int* nbad) {
  const dim3 grid((unsigned)((pad_to + k256 - 1) / k256));
  if (dtype == 0)
    hipLaunchKernelGGL(collapsed_weights_kernel<double>, grid, dim3(k256), 0, s, (const double*)sv, sigma2, n, pad_to, (double*)w, wd, nbad);
  else
    hipLaunchKernelGGL(collapsed_weights_kernel<float>, grid, dim3(k256), 0, s, (const float*)sv, sigma2, n, pad_to, (float*)w, wd, nbad);
}

void launch_collapsed_reduce_w(int dtype, hipStream_t s, const void* At, const void* y, const void* mux, const void* sv, const double* wd,
                               const double* ssq, int64_t Mp, int64_t off, int64_t n, double mean_const, double sigma2, int first,
                               double* bpart, double* spart, double* spart2) {
  const dim3 grid((unsigned)(Mp / 128), (unsigned)kCollapsedSplit);
  if (dtype == 0)
    hipLaunchKernelGGL(collapsed_reduce_w_kernel<double>, grid, dim3(128), 0, s, (const double*)At, (const double*)y, (const double*)mux,
                       (const double*)sv, wd, ssq, Mp, off, n, mean_const, sigma2, first, bpart, spart, spart2);
  else
    hipLaunchKernelGGL(collapsed_reduce_w_kernel<float>, grid, dim3(128), 0, s, (const float*)At, (const float*)y, (const float*)mux,
                       (const float*)sv, wd, ssq, Mp, off, n, mean_const, sigma2, first, bpart, spart, spart2);
}

void launch_collapsed_extra(hipStream_t s, const double* spart2, double* scal) {
  hipLaunchKernelGGL(collapsed_extra_kernel, dim3(1), dim3(64), 0, s, spart2, kCollapsedSplit, scal);
}

void launch_point_grads_noise(int dtype, hipStream_t s, double sigma2, int clamp_neg_var, const double* mom_mu, const double* mom_var,
                              const void* y, int64_t off, int64_t len, double scale, const void* noise, void* gmu_out, void* gv_out,
                              double* part5, unsigned* strip_queue, int64_t pad_to, void* gmu_copy, void* noise_bar) {
  const int nb = point_grad_blocks(len);   // (pad_to <= the 256-point blocks of the launch, as launch_point_grads)
  if (dtype == 0)
    hipLaunchKernelGGL(collapsed_point_grad_kernel<double>, dim3(nb), dim3(k256), 0, s, sigma2, clamp_neg_var, mom_mu, mom_var, (const double*)y,
                       off, len, scale, (const double*)noise, (double*)gmu_out, (double*)gv_out, part5, strip_queue, pad_to, (double*)gmu_copy,
                       (double*)noise_bar);
  else
    hipLaunchKernelGGL(collapsed_point_grad_kernel<float>, dim3(nb), dim3(k256), 0, s, sigma2, clamp_neg_var, mom_mu, mom_var, (const float*)y,
                       off, len, scale, (const float*)noise, (float*)gmu_out, (float*)gv_out, part5, strip_queue, pad_to, (float*)gmu_copy,
                       (float*)noise_bar);
}

void launch_collapsed_pivot_check(int dtype, hipStream_t s, const void* Lk, int64_t M, int64_t Mp, double kdiag, int* first_bad) {
  if (dtype == 0) hipLaunchKernelGGL(collapsed_pivot_check_kernel<double>, dim3(1), dim3(k256), 0, s, (const double*)Lk, M, Mp, kdiag, first_bad);
  else hipLaunchKernelGGL(collapsed_pivot_check_kernel<float>, dim3(1), dim3(k256), 0, s, (const float*)Lk, M, Mp, kdiag, first_bad);
}

void launch_collapsed_form_b(int dtype, hipStream_t s, const void* G, int nslices, int64_t Mp, double sigma2, const double* bpart,
                             const double* spart, double* Bm, double* cvec, double* scal) {
  const dim3 grid((unsigned)((Mp + k256 - 1) / k256), (unsigned)Mp);
  if (dtype == 0)
    hipLaunchKernelGGL(collapsed_form_b_kernel<double>, grid, dim3(k256), 0, s, (const double*)G, nslices, Mp, 1.0 / sigma2, bpart, spart,
                       kCollapsedSplit, Bm, cvec, scal);
  else
    hipLaunchKernelGGL(collapsed_form_b_kernel<float>, grid, dim3(k256), 0, s, (const float*)G, nslices, Mp, 1.0 / sigma2, bpart, spart,
                       kCollapsedSplit, Bm, cvec, scal);
}

void launch_collapsed_scal(hipStream_t s, const double* LB, const double* c, int64_t Mp, const int* info_b, const int* info_s, double* scal) {
  hipLaunchKernelGGL(collapsed_scal_kernel, dim3(1), dim3(k256), 0, s, LB, c, Mp, info_b, info_s, scal);
}

void launch_collapsed_write_q(int dtype, hipStream_t s, const double* Lqw, const double* mw, const void* Lk, int64_t M, int64_t Mp, int centered,
                              double mean_const, const double* scal, const int* info_b, const int* info_s, const void* muz, void* m_out,
                              void* Lq_out) {
  const dim3 grid((unsigned)((M + k256 - 1) / k256), (unsigned)M);
  if (dtype == 0)
    hipLaunchKernelGGL(collapsed_write_q_kernel<double>, grid, dim3(k256), 0, s, Lqw, mw, (const double*)Lk, M, Mp, centered, mean_const, scal,
                       info_b, info_s, (const double*)muz, (double*)m_out, (double*)Lq_out);
  else
    hipLaunchKernelGGL(collapsed_write_q_kernel<float>, grid, dim3(k256), 0, s, Lqw, mw, (const float*)Lk, M, Mp, centered, mean_const, scal,
                       info_b, info_s, (const float*)muz, (float*)m_out, (float*)Lq_out);
}

}  // namespace svgp
