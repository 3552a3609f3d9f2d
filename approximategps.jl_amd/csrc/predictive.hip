// predictive.hip — the predictive distribution of the OBSERVATION behind a latent marginal N(mu_i, v_i) (svgp_predictive,
// svgp_lik_predictive): per point  log p(y_i | D) = log int p(y_i | f) N(f; mu_i, v_i) df  and  (E[y_i], Var[y_i])  (lik.hpp:
// predictive_logdensity_point, predictive_moments_point), and their sums.  The data-sized work in front of it - Kuf -> trsm -> trmm
// strips, column sums - is the forward pass's, unchanged: this kernel stands where expect_kernel stands and reads the same moments.
//   predictive_kernel         one point per thread, grid-stride; per-block sums {sum lpd, sum (y - E[y])^2, n_neg} by a fixed LDS tree
//   predictive_reduce_kernel  the blocks' sums in a fixed order -> out[0..3)
// Every sum has a fixed split and a fixed order: bitwise repeatable, no atomics.
#include "device_common.hpp"
#include "kernels.hpp"
#include "lik.hpp"

namespace svgp {
namespace {

// var_shift: kDefaultSigma2 for the moments the strips left (FiniteGP(f_post, x, 1e-18) -> marginals, as expect_kernel), 0 for a
// caller's marginals (svgp_lik_predictive: svgp_marginals' variances hold it already).  The negative-variance policy is expect_kernel's:
// a point with v < 0 is counted; clamped to v = 0 where the model says so, else left out of both sums with NaN outputs.
// y may be NULL (moments only: no lpd, no sums); lpd_out / ymean_out / yvar_out may each be NULL.
template <typename T>
__global__ void __launch_bounds__(k256, 2) predictive_kernel(LikParams lp, const double* __restrict__ mom_mu,
                                                          const double* __restrict__ mom_var, const T* __restrict__ y, int64_t off,
                                                          int64_t len, double var_shift, double* __restrict__ part3,
                                                          double* __restrict__ lpd_out, double* __restrict__ ymean_out,
                                                          double* __restrict__ yvar_out) {
  __shared__ double sh[3][k256];
  double s_lpd = 0.0, s_sq = 0.0, neg = 0.0;
#pragma unroll 1
  for (int64_t i = int64_t(blockIdx.x) * k256 + threadIdx.x; i < len; i += int64_t(gridDim.x) * k256) {
    const double mu = mom_mu[i];
    double v = mom_var[i] + var_shift;
    bool bad = v < 0.0;
    if (bad) {
      neg += 1.0;
      if (lp.clamp_neg_var) { v = 0.0; bad = false; }
    }
    double lpd = NAN, ym = NAN, yv = NAN;
    if (!bad) {
      predictive_moments_point(lp, mu, v, ym, yv);
      if (y) {
        const double yi = double(y[off + i]);
        lpd = predictive_logdensity_point(lp, mu, v, yi);
        s_lpd += lpd;
        s_sq += (yi - ym) * (yi - ym);
      }
    }
    if (lpd_out) lpd_out[i] = lpd;
    if (ymean_out) ymean_out[i] = ym;
    if (yvar_out) yvar_out[i] = yv;
  }
  sh[0][threadIdx.x] = s_lpd;
  sh[1][threadIdx.x] = s_sq;
  sh[2][threadIdx.x] = neg;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) {
#pragma unroll
      for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) part3[int64_t(blockIdx.x) * 3 + threadIdx.x] = sh[threadIdx.x][0];
}

// out[q] = sum over the nb blocks of part3[b][q], q < 3: thread t takes blocks t, t + 256, ..., then a fixed LDS tree
__global__ void __launch_bounds__(k256) predictive_reduce_kernel(const double* __restrict__ part3, int nb, double* __restrict__ out) {
  __shared__ double sh[3][k256];
  double a[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += k256) {
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] += part3[int64_t(b) * 3 + q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] = a[q];
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) {
#pragma unroll
      for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) out[threadIdx.x] = sh[threadIdx.x][0];
}

}  // namespace

void launch_predictive(int dtype, hipStream_t s, const LikParams& lp, const double* mom_mu, const double* mom_var, const void* y,
                       int64_t off, int64_t len, double var_shift, double* part3, double* sums3, double* lpd_out, double* ymean_out,
                       double* yvar_out) {
  const int nb = expect_blocks(len);
  if (dtype == 0)
    hipLaunchKernelGGL(predictive_kernel<double>, dim3(nb), dim3(k256), 0, s, lp, mom_mu, mom_var, (const double*)y, off, len, var_shift,
                       part3, lpd_out, ymean_out, yvar_out);
  else
    hipLaunchKernelGGL(predictive_kernel<float>, dim3(nb), dim3(k256), 0, s, lp, mom_mu, mom_var, (const float*)y, off, len, var_shift,
                       part3, lpd_out, ymean_out, yvar_out);
  hipLaunchKernelGGL(predictive_reduce_kernel, dim3(1), dim3(k256), 0, s, part3, nb, sums3);
}

}  // namespace svgp
