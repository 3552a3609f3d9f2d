// laplace.hip — the Laplace approximation (reference src/LaplaceApproximationModule.jl, RW = Rasmussen & Williams 2006):
//   posterior(la, lfx, y)   :39-49      approx_lml(la, lfx, y)   :157-165, :250-254
//   Newton mode finding      :256-276 (_newton_inner_loop, RW Alg. 3.1), one step = _laplace_train_intermediates :201-240
//   predictions              :425-463 (RW 3.21 / 3.29)
//   d approx_lml / d (variance, inverse lengthscales): the reference differentiates through the implicit-function rrule of
//   newton_inner_loop (:330-369); here its closed form, RW Alg. 5.1 generalised to any likelihood through d3 log p.
// One Newton step on the device, everything padded to Np = ceil(N / 128) * 128 (padding: W = 0, so B = I there, K = 0):
//   point kernel        g = dll, W = -d2ll, sW = sqrt(W), b = W f + g, d3ll               lp_point_kernel
//   B = I + sW K sW     (K stays intact for the GEMVs and the gradient)                   lp_assemble_b_kernel
//   L = chol(B)         the blocked MFMA factorisation of the SVGP path, in place        launch_potrf
//   L^-1                recursive doubling from its inverted diagonal blocks              launch_linv
//   a = b - sW L^-T L^-1 (sW K b),  fnew = K a                                           lp_gemv_kernel, launch_linv_t_gemv
//   fp32: a += r - sW L^-T L^-1 (sW K r), r = b - a - W K a (one refinement step)        lp_resid_kernel, lp_refine_kernel
//   isapprox(f, fnew), -a'f / 2, sum ll, sum log diag L: one workgroup, one read-back    lp_stats_kernel
// The solves are GEMVs with the explicit inverse: every one of them runs across the chip (the one-workgroup trsv_kernel of the
// SVGP posterior streams the triangle through one CU).  The gradient reuses that inverse:
//   R = sW L^-T L^-1 sW                   gemm_pm (SYRK shape, MFMA), lp_scale_r_kernel
//   K R                                   gemm_pm (MFMA)
//   Sigma_ii = K_ii - (K R K)_ii          lp_diag_krk_kernel;  s2 = Sigma_ii d3ll / 2,  u = s2 - R (K s2)
//   d lml / d theta = sum_ik P_ik dK_ik / d theta,  P = a a' / 2 - R / 2 + (u g' + g u') / 2, kernel derivatives generated on the
//   fly from x                            lp_kgrad_kernel (one fused reduction for the variance and every inverse lengthscale)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "device_common.hpp"
#include "kernels.hpp"
#include "lik.hpp"

namespace svgp {
namespace {

#define LP_DISPATCH(dtype, T, ...)      \
  do {                                  \
    if ((dtype) == 0) {                 \
      using T = double;                 \
      __VA_ARGS__;                      \
    } else {                            \
      using T = float;                  \
      __VA_ARGS__;                      \
    }                                   \
  } while (0)

// xs[f][i] = x[f][i] * invl[f] for i < n, 0 for n <= i < np  (x feature-major [d][ldx])
template <typename T>
__global__ void lp_scale_kernel(const T* __restrict__ x, int64_t ldx, int64_t n, int64_t np, const T* __restrict__ invl,
                                T* __restrict__ xs) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int f = blockIdx.y;
  if (i >= np) return;
  xs[int64_t(f) * np + i] = i < n ? x[int64_t(f) * ldx + i] * invl[f] : T(0);
}

// out[i + j ldo] = k(xa_i, xb_j) (+ jitter when i == j and add_jitter) for i < na, j < nb; 0 for na <= i < rows
template <typename T>
__global__ void lp_kcross_kernel(int family, int d, T variance, const T* __restrict__ xa, int64_t lda, int64_t na, int64_t rows,
                                 const T* __restrict__ xb, int64_t ldb, int64_t nb, T jitter, int add_jitter, T* __restrict__ out,
                                 int64_t ldo) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t j = blockIdx.y;
  if (i >= rows) return;
  T v = T(0);
  if (i < na && j < nb) {
    T r2 = T(0);
    for (int f = 0; f < d; ++f) {
      const T df = xa[int64_t(f) * lda + i] - xb[int64_t(f) * ldb + j];
      r2 = fma(df, df, r2);
    }
    v = kappa(family, r2, variance);
    if (add_jitter && i == j) v += jitter;
  }
  out[i + j * ldo] = v;
}

// log p(y|f) and its derivatives at every point (_laplace_train_intermediates :210-221); padding: all zero
template <typename T>
__global__ void lp_point_kernel(int lik, double sigma2, const T* __restrict__ f, const T* __restrict__ y, int64_t n, int64_t np,
                                T* __restrict__ g, T* __restrict__ W, T* __restrict__ sW, T* __restrict__ b, T* __restrict__ d3) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double gi = 0.0, wi = 0.0, d3i = 0.0, fi = 0.0;
  if (i < n) {
    fi = double(f[i]);
    const double yi = double(y[i]);
    double d2;
    gi = dloglik_point(lik, fi, yi, sigma2);
    d23loglik_point(lik, fi, yi, sigma2, d2, d3i);
    wi = -d2;
  }
  const T wt = T(wi);
  g[i] = T(gi);
  W[i] = wt;
  sW[i] = T(sqrt(fmax(double(wt), 0.0)));
  b[i] = T(fma(double(wt), fi, gi));
  d3[i] = T(d3i);
}

// B = I + sW_i K_ij sW_j, lower 128-tiles only (the factorisation and L^-1 never read above them)
template <typename T>
__global__ void lp_assemble_b_kernel(const T* __restrict__ K, const T* __restrict__ sW, int64_t np, T* __restrict__ B) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t j = blockIdx.y;
  if (i >= np || i / kNB < j / kNB) return;
  const int64_t e = i + j * np;
  B[e] = sW[i] * K[e] * sW[j] + (i == j ? T(1) : T(0));
}

// out = M v for a full np x np column-major M: workgroup (bx, by) takes rows [64 bx, 64 bx + 64) against the 128 columns of
// panel by (thread (r, g): columns by 128 + g, + 4, ...; a column segment is read contiguously), fp64 partials per panel
template <typename T>
__global__ void __launch_bounds__(k256) lp_gemv_kernel(const T* __restrict__ M, const T* __restrict__ v, int64_t np,
                                                       double* __restrict__ part) {
  __shared__ double sh[4][64];
  const int rl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t r = int64_t(blockIdx.x) * 64 + rl, k0 = int64_t(blockIdx.y) * kNB;
  double acc = 0.0;
#pragma unroll 8
  for (int kk = g; kk < kNB; kk += 4) {
    const int64_t k = k0 + kk;
    acc = fma(double(M[k * np + r]), double(v[k]), acc);
  }
  sh[g][rl] = acc;
  __syncthreads();
  if (g == 0) part[int64_t(blockIdx.y) * np + r] = ((sh[0][rl] + sh[1][rl]) + sh[2][rl]) + sh[3][rl];
}
// out[r] = s (mode 0),  sc[r] s (mode 1),  base[r] - sc[r] s (mode 2),  base[r] - s (mode 3);  s = sum of the panel partials
template <typename T>
__global__ void lp_gemv_finish_kernel(const double* __restrict__ part, int npan, int64_t np, int mode, const T* __restrict__ sc,
                                      const T* __restrict__ base, T* __restrict__ out) {
  const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= np) return;
  double s = 0.0;
  for (int q = 0; q < npan; ++q) s += part[int64_t(q) * np + r];
  double o = s;
  if (mode == 1) o = double(sc[r]) * s;
  else if (mode == 2) o = double(base[r]) - double(sc[r]) * s;
  else if (mode == 3) o = double(base[r]) - s;
  out[r] = T(o);
}
// out[r] = b[r] - sc[r] v[r]
template <typename T>
__global__ void lp_sub_scaled_kernel(const T* __restrict__ b, const T* __restrict__ sc, const T* __restrict__ v, int64_t np, T* __restrict__ out) {
  const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r < np) out[r] = T(double(b[r]) - double(sc[r]) * double(v[r]));
}

// The fp32 refinement of a (lp_step): r = b - a - W (K a), K a from the fp64 panel partials
template <typename T>
__global__ void lp_resid_kernel(const double* __restrict__ part, int npan, int64_t np, const T* __restrict__ b, const T* __restrict__ a,
                                const T* __restrict__ W, T* __restrict__ r) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double s = 0.0;
  for (int q = 0; q < npan; ++q) s += part[int64_t(q) * np + i];
  r[i] = T((double(b[i]) - double(a[i])) - double(W[i]) * s);
}
// a[i] += r[i] - sc[i] v[i]
template <typename T>
__global__ void lp_refine_kernel(T* __restrict__ a, const T* __restrict__ r, const T* __restrict__ sc, const T* __restrict__ v, int64_t np) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < np) a[i] = T(double(a[i]) + (double(r[i]) - double(sc[i]) * double(v[i])));
}

// ll[i] = log p(y_i | f_i) (its own launch: the lgamma / erfcx bodies stay out of the reduction's registers)
template <typename T>
__global__ void lp_ll_kernel(int lik, double sigma2, const T* __restrict__ f, const T* __restrict__ y, int64_t n, double* __restrict__ ll) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) ll[i] = loglik_point(lik, double(f[i]), double(y[i]), sigma2, log(sigma2));
}

// res = {|f - fnew|^2, |f|^2, |fnew|^2, a'f, sum ll(f), sum log diag L, chol info}: one workgroup, fixed summation order
template <typename T>
__global__ void __launch_bounds__(k256) lp_stats_kernel(const T* __restrict__ f, const T* __restrict__ fnew, const T* __restrict__ a,
                                                        const double* __restrict__ ll, const T* __restrict__ L, int64_t n, int64_t np,
                                                        const int* __restrict__ info, double* __restrict__ res) {
  __shared__ double sh[6][k256];
  const int t = threadIdx.x;
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = t; i < n; i += k256) {
    const double fi = double(f[i]), fn = double(fnew[i]), dd = fi - fn;
    s[0] = fma(dd, dd, s[0]);
    s[1] = fma(fi, fi, s[1]);
    s[2] = fma(fn, fn, s[2]);
    s[3] = fma(double(a[i]), fi, s[3]);
    s[4] += ll[i];
    s[5] += log(double(L[i + i * np]));
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) sh[q][t] = s[q];
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (t < w)
#pragma unroll
      for (int q = 0; q < 6; ++q) sh[q][t] += sh[q][t + w];
    __syncthreads();
  }
  if (t < 6) res[t] = sh[t][0];
  if (t == 6) res[6] = double(info[0]);
}

// R_ik = sW_i G_ik sW_k (G = L^-T L^-1, symmetric)
template <typename T>
__global__ void lp_scale_r_kernel(T* __restrict__ R, const T* __restrict__ sW, int64_t np) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t k = blockIdx.y;
  if (i < np) R[i + k * np] = T(double(sW[i]) * double(R[i + k * np]) * double(sW[k]));
}

// part[c][i] = sum over the columns k of chunk c of (K R)_ik K_ik  (X = K R column-major): (K R K)_ii
template <typename T>
__global__ void lp_diag_krk_kernel(const T* __restrict__ X, const T* __restrict__ K, int64_t np, int64_t chunk,
                                   double* __restrict__ part) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const int64_t k0 = int64_t(blockIdx.y) * chunk, k1 = k0 + chunk < np ? k0 + chunk : np;
  double s = 0.0;
  for (int64_t k = k0; k < k1; ++k) s = fma(double(X[i + k * np]), double(K[i + k * np]), s);
  part[int64_t(blockIdx.y) * np + i] = s;
}
// s2_i = (K_ii - (K R K)_ii) d3_i / 2 for i < n, 0 on the padding: d lml / d f_opt_i through -log det B / 2 (dW / df = -d3)
template <typename T>
__global__ void lp_s2_kernel(const double* __restrict__ part, int nchunk, const T* __restrict__ K, const T* __restrict__ d3, int64_t n,
                             int64_t np, T* __restrict__ s2) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; ++c) s += part[int64_t(c) * np + i];
  s2[i] = i < n ? T(0.5 * (double(K[i + i * np]) - s) * double(d3[i])) : T(0);
}

// unit-variance kernel kappa(r2) and d kappa / d r2
__device__ __forceinline__ void lp_kappa_d(int family, double r2, double& k, double& dk) {
  if (family == KSE) {
    k = exp(-0.5 * r2);
    dk = -0.5 * k;
  } else if (family == KM32) {
    const double s = 1.7320508075688772935 * sqrt(r2), e = exp(-s);
    k = (1.0 + s) * e;
    dk = -1.5 * e;
  } else {
    const double s = 2.2360679774997896964 * sqrt(r2), e = exp(-s);
    k = (1.0 + s + (5.0 / 3.0) * r2) * e;
    dk = -(5.0 / 6.0) * (1.0 + s) * e;
  }
}

// The fused kernel-parameter reduction.  Workgroup (ti, tk, fc): the 64 x 64 pair tile (ti, tk), tk <= ti (an off-diagonal tile
// counts twice: P and dK are symmetric), features [8 fc, 8 fc + 8).  Thread (il, q): row i = 64 ti + il, columns k = 64 tk + q,
// + 4, ...  Per pair: P_ik = (a_i a_k - R_ik + u_i g_k + g_i u_k) / 2,
//   slot 0 (fc == 0):  sum P_ik kappa_ik                                   (d K / d variance, K without the jitter)
//   slot 1 + f:        sum P_ik variance kappa'(r2) 2 invl_f (x_if - x_kf)^2   (d K / d invl_f)
// part[block][9]: fixed order, summed by lp_kgrad_finish_kernel.
constexpr int kLpFc = 8;
template <typename T>
__global__ void __launch_bounds__(k256) lp_kgrad_kernel(int family, int d, double variance, const double* __restrict__ invl,
                                                        const T* __restrict__ x, int64_t ldx, int64_t n, int64_t np,
                                                        const T* __restrict__ R, const T* __restrict__ a, const T* __restrict__ g,
                                                        const T* __restrict__ u, double* __restrict__ part) {
  __shared__ double xi_s[SVGP_MAX_D][64];
  __shared__ double vk[3][64];
  __shared__ double red[4][1 + kLpFc];
  const int ti = blockIdx.x, tk = blockIdx.y, fc = blockIdx.z, t = threadIdx.x, il = t & 63, q = t >> 6;
  const int64_t blk = (int64_t(blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  double acc[1 + kLpFc];
#pragma unroll
  for (int s = 0; s < 1 + kLpFc; ++s) acc[s] = 0.0;
  if (tk <= ti) {
    for (int e = t; e < d * 64; e += k256) {
      const int f = e / 64, c = e % 64;
      const int64_t ii = int64_t(ti) * 64 + c;
      xi_s[f][c] = ii < n ? double(x[int64_t(f) * ldx + ii]) : 0.0;
    }
    if (t < 64) {
      const int64_t kk = int64_t(tk) * 64 + t;
      vk[0][t] = kk < np ? double(a[kk]) : 0.0;
      vk[1][t] = kk < np ? double(g[kk]) : 0.0;
      vk[2][t] = kk < np ? double(u[kk]) : 0.0;
    }
    __syncthreads();
    const int64_t i = int64_t(ti) * 64 + il;
    const double ai = i < np ? double(a[i]) : 0.0, gi = i < np ? double(g[i]) : 0.0, ui = i < np ? double(u[i]) : 0.0;
    const double mult = ti == tk ? 0.5 : 1.0;   // (1/2 of P) x (2 for the mirrored tile)
    const int f0 = fc * kLpFc;
    for (int c = q; c < 64; c += 4) {   // k is wave-uniform: x_k is a broadcast load
      const int64_t k = int64_t(tk) * 64 + c;
      if (i >= n || k >= n) continue;
      double r2 = 0.0;
      for (int f = 0; f < d; ++f) {
        const double df = invl[f] * (xi_s[f][il] - double(x[int64_t(f) * ldx + k]));
        r2 = fma(df, df, r2);
      }
      double kap, dk;
      lp_kappa_d(family, r2, kap, dk);
      const double P = mult * (ai * vk[0][c] - double(R[i + k * np]) + ui * vk[1][c] + gi * vk[2][c]);
      if (fc == 0) acc[0] = fma(P, kap, acc[0]);
      const double c2 = P * variance * dk * 2.0;
#pragma unroll
      for (int s = 0; s < kLpFc; ++s) {
        const int f = f0 + s;
        if (f < d) {
          const double df = xi_s[f][il] - double(x[int64_t(f) * ldx + k]);
          acc[1 + s] = fma(c2 * invl[f], df * df, acc[1 + s]);
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 1 + kLpFc; ++s) {
    double v = acc[s];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (il == 0) red[q][s] = v;
  }
  __syncthreads();
  if (t < 1 + kLpFc) part[blk * (1 + kLpFc) + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}
// out[0] = d / d variance, out[1 + f] = d / d invl_f: the block partials in a fixed order
__global__ void __launch_bounds__(k256) lp_kgrad_finish_kernel(const double* __restrict__ part, int64_t nblk_xy, int nfc, int d,
                                                               double* __restrict__ out) {
  __shared__ double sh[k256];
  const int slot = blockIdx.x, t = threadIdx.x;   // slot 0: variance; 1 + f: feature f
  const int fc = slot == 0 ? 0 : (slot - 1) / kLpFc, s = slot == 0 ? 0 : 1 + (slot - 1) % kLpFc;
  double acc = 0.0;
  if (fc < nfc)
    for (int64_t b = t; b < nblk_xy; b += k256) acc += part[(int64_t(fc) * nblk_xy + b) * (1 + kLpFc) + s];
  sh[t] = acc;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  if (t == 0 && slot <= d) out[slot] = sh[0];
}

// ---- predictions -----------------------------------------------------------------------------------------------
// out[j] = sum_i Kx(i, j) g_i (mode 0: RW 3.21)   or   variance - sum_i V(i, j)^2 (mode 1: RW 3.29 |> diag); one workgroup per j
template <typename T>
__global__ void __launch_bounds__(k256) lp_colreduce_kernel(const T* __restrict__ X, int64_t ldx, int64_t rows, const T* __restrict__ g,
                                                            int mode, double variance, T* __restrict__ out) {
  __shared__ double sh[k256];
  const int64_t j = blockIdx.x;
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int64_t i = t; i < rows; i += k256) {
    const double v = double(X[i + j * ldx]);
    acc = mode == 0 ? fma(v, double(g[i]), acc) : fma(v, v, acc);
  }
  sh[t] = acc;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  if (t == 0) out[j] = T(mode == 0 ? sh[0] : variance - sh[0]);
}
// X[i + j ld] *= sc[i]
template <typename T>
__global__ void lp_rowscale_kernel(T* __restrict__ X, int64_t ld, int64_t rows, const T* __restrict__ sc) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t j = blockIdx.y;
  if (i < rows) X[i + j * ld] = T(double(X[i + j * ld]) * double(sc[i]));
}
// out(i, j) (=|-=) sum_k A(i, k) B(k, j), A(i, k) = A[i sai + k sak], B(k, j) = B[k sbk + j sbj], out(i, j) = out[i + j ldo];
// 64 x 64 output tiles, 16 x 16 threads of 4 x 4 outputs, fp64 accumulation (the O(N^2 n*) products of the predictions)
template <typename T>
__global__ void __launch_bounds__(k256) lp_gemm_kernel(int64_t m, int64_t nn, int64_t kd, const T* __restrict__ A, int64_t sai, int64_t sak,
                                                       const T* __restrict__ B, int64_t sbk, int64_t sbj, T* __restrict__ out, int64_t ldo,
                                                       int subtract) {
  __shared__ double As[16][65], Bs[16][65];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, t = threadIdx.x;
  const int64_t i0 = int64_t(blockIdx.x) * 64, j0 = int64_t(blockIdx.y) * 64;
  double acc[4][4] = {};
  for (int64_t k0 = 0; k0 < kd; k0 += 16) {
    // consecutive threads walk the operand's contiguous index (unit stride): row / column of the tile, or k
    for (int e = t; e < 1024; e += k256) {
      const int ra = sai == 1 ? (e & 63) : (e >> 4), ka = sai == 1 ? (e >> 6) : (e & 15);
      const int rb = sbj == 1 ? (e & 63) : (e >> 4), kb = sbj == 1 ? (e >> 6) : (e & 15);
      const int64_t i = i0 + ra, j = j0 + rb;
      As[ka][ra] = (i < m && k0 + ka < kd) ? double(A[i * sai + (k0 + ka) * sak]) : 0.0;
      Bs[kb][rb] = (j < nn && k0 + kb < kd) ? double(B[(k0 + kb) * sbk + j * sbj]) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) acc[p][qq] = fma(As[kk][tx + 16 * p], Bs[kk][ty + 16 * qq], acc[p][qq]);
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int64_t i = i0 + tx + 16 * p, j = j0 + ty + 16 * qq;
      if (i < m && j < nn) out[i + j * ldo] = subtract ? T(double(out[i + j * ldo]) - acc[p][qq]) : T(acc[p][qq]);
    }
}

inline unsigned nblk(int64_t n, int b = 256) { return unsigned((n + b - 1) / b); }

}  // namespace
}  // namespace svgp

// ================================================================================================
using namespace svgp;

struct svgp_laplace {
  const svgp_data* data = nullptr;
  int dtype = 0, d = 0;
  int64_t N = 0, Np = 0;
  size_t es = 8;
  DevBuf K, B, T, LinvRM, LinvCM, Ytmp;
  DevBuf xs, invl_t, f, fnew, g, W, sW, b, d3, a, t1, t2, t3;
  DevBuf part;     // (Np / 128) x Np fp64 GEMV partials
  DevBuf res;      // [16 + SVGP_MAX_D] fp64 step statistics / gradient slots (1 + d)
  DevBuf invl_d;   // [d] fp64 inverse lengthscales (gradient kernel)
  DevBuf llv;      // [Np] fp64 log p(y_i | f_i) of the step
  DevBuf info;     // (int) chol info + the factorisation's hand-over counters
  DevBuf R, X;     // gradient: R and K R (allocated on first use)
  DevBuf gpart;    // (fp64) the gradient's partial sums, grown on demand
  Event ev[5];
  // the last fit: its parameters (predictions), whether a mode exists (warm start)
  bool have_mode = false;
  int family = 0, lik = 0;
  double variance = 1.0, jitter = 0.0, lik_sigma2 = 1.0;
  std::vector<double> invl;
};

namespace {

inline size_t lp_info_bytes(int64_t Np) { return (sizeof(int) * size_t(1 + 2 * (Np / 128)) + 255) / 256 * 256; }
inline int64_t lp_max_n(int dtype) { return dtype == SVGP_F64 ? 8192 : 16384; }   // the sizes the device Cholesky is tested at

int check_desc(svgp_ctx* ctx, const svgp_laplace* la, const svgp_laplace_desc* ds) {
  if (!ds) return fail(ctx, SVGP_INVALID_ARG, "null Laplace descriptor");
  if (ds->dtype != la->dtype) return fail(ctx, SVGP_INVALID_ARG, "descriptor dtype differs from the data's");
  if (ds->d != la->d) return fail(ctx, SVGP_INVALID_ARG, "descriptor d differs from the data's");
  if (ds->kernel < SVGP_KERNEL_SE || ds->kernel > SVGP_KERNEL_MATERN52) return fail(ctx, SVGP_INVALID_ARG, "bad kernel");
  if (ds->likelihood < SVGP_LIK_GAUSSIAN || ds->likelihood > SVGP_LIK_BERNOULLI_NORMCDF) return fail(ctx, SVGP_INVALID_ARG, "bad likelihood");
  if (ds->maxiter < 1) return fail(ctx, SVGP_INVALID_ARG, "maxiter must be >= 1 (_newton_inner_loop :257)");
  if (ds->warm_start != 0 && ds->warm_start != 1) return fail(ctx, SVGP_INVALID_ARG, "warm_start must be 0 or 1");
  if (ds->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved field must be 0");
  if (!ds->inv_lengthscale) return fail(ctx, SVGP_INVALID_ARG, "null inv_lengthscale");
  if (!(ds->variance > 0.0)) return fail(ctx, SVGP_INVALID_ARG, "variance must be > 0");
  if (!(ds->jitter >= 0.0)) return fail(ctx, SVGP_INVALID_ARG, "jitter must be >= 0");
  if ((ds->likelihood == SVGP_LIK_GAUSSIAN || ds->likelihood == SVGP_LIK_GAMMA_EXP) && !(ds->lik_sigma2 > 0.0))
    return fail(ctx, SVGP_INVALID_ARG, "likelihood parameter must be > 0");
  return SVGP_OK;
}

// K = k(x, x) + jitter I from the descriptor (and the scaled inputs it needs)
int lp_prepare(svgp_ctx* ctx, svgp_laplace* la, const svgp_laplace_desc* ds) {
  hipStream_t s = ctx->stream;
  la->family = ds->kernel;
  la->lik = ds->likelihood;
  la->variance = ds->variance;
  la->jitter = ds->jitter;
  la->lik_sigma2 = (ds->likelihood == SVGP_LIK_GAUSSIAN || ds->likelihood == SVGP_LIK_GAMMA_EXP) ? ds->lik_sigma2 : 1.0;
  la->invl.assign(ds->inv_lengthscale, ds->inv_lengthscale + la->d);
  HIPC(ctx, hipMemcpyAsync(la->invl_d.as<double>(), la->invl.data(), size_t(la->d) * 8, hipMemcpyHostToDevice, s));
  const int64_t N = la->N, Np = la->Np;
  LP_DISPATCH(la->dtype, T, {
    std::vector<T> iv(la->invl.begin(), la->invl.end());
    HIPC(ctx, hipMemcpyAsync(la->invl_t.p, iv.data(), size_t(la->d) * sizeof(T), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(lp_scale_kernel<T>, dim3(nblk(Np), (unsigned)la->d), dim3(256), 0, s, (const T*)la->data->x.p, la->data->ldx, N, Np,
                       (const T*)la->invl_t.p, (T*)la->xs.p);
    hipLaunchKernelGGL(lp_kcross_kernel<T>, dim3(nblk(Np), (unsigned)Np), dim3(256), 0, s, la->family, la->d, T(la->variance),
                       (const T*)la->xs.p, Np, N, Np, (const T*)la->xs.p, Np, N, T(la->jitter), 1, (T*)la->K.p, Np);
    HIPC(ctx, hipStreamSynchronize(s));   // iv leaves scope
  });
  KCHECK(ctx, "lp_prepare");
  return SVGP_OK;
}

// one step at la->f: the intermediates (g, W, sW, b, d3, L, L^-1, a), fnew, and the statistics in st[7]
int lp_step(svgp_ctx* ctx, svgp_laplace* la, double st[7], double ms[4]) {
  hipStream_t s = ctx->stream;
  const int64_t N = la->N, Np = la->Np;
  const int npan = int(Np / kNB);
  const bool timed = ctx->timing_on;
  if (timed) HIPC(ctx, hipEventRecord(la->ev[0], s));
  LP_DISPATCH(la->dtype, T, {
    hipLaunchKernelGGL(lp_point_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->lik, la->lik_sigma2, (const T*)la->f.p, (const T*)la->data->y.p,
                       N, Np, (T*)la->g.p, (T*)la->W.p, (T*)la->sW.p, (T*)la->b.p, (T*)la->d3.p);
    hipLaunchKernelGGL(lp_assemble_b_kernel<T>, dim3(nblk(Np), (unsigned)Np), dim3(256), 0, s, (const T*)la->K.p, (const T*)la->sW.p, Np, (T*)la->B.p);
  });
  KCHECK(ctx, "lp_point / lp_assemble_b");
  if (timed) HIPC(ctx, hipEventRecord(la->ev[1], s));
  HIPC(ctx, hipMemsetAsync(la->info.as<int>(), 0, lp_info_bytes(Np), s));
  launch_potrf(la->dtype, s, la->B.p, la->T.p, Np, la->info.as<int>(), reinterpret_cast<unsigned*>(la->info.as<int>() + 1), ctx->num_cus);
  KCHECK(ctx, "potrf");
  if (timed) HIPC(ctx, hipEventRecord(la->ev[2], s));
  launch_linv(la->dtype, s, la->B.p, la->T.p, Np, la->LinvRM.p, la->LinvCM.p, la->Ytmp.p);
  KCHECK(ctx, "linv");
  if (timed) HIPC(ctx, hipEventRecord(la->ev[3], s));
  LP_DISPATCH(la->dtype, T, {
    // t1 = sW (K b)
    hipLaunchKernelGGL(lp_gemv_kernel<T>, dim3(unsigned(Np / 64), unsigned(npan)), dim3(k256), 0, s, (const T*)la->K.p, (const T*)la->b.p, Np, la->part.as<double>());
    hipLaunchKernelGGL(lp_gemv_finish_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->part.as<double>(), npan, Np, 1, (const T*)la->sW.p, (const T*)nullptr, (T*)la->t1.p);
    // t2 = L^-1 t1, t3 = L^-T t2 (= B \ t1)
    launch_linv_t_gemv(la->dtype, s, la->LinvCM.p, la->t1.p, Np, la->t2.p, la->part.as<double>(), 1);
    launch_linv_t_gemv(la->dtype, s, la->LinvRM.p, la->t2.p, Np, la->t3.p, la->part.as<double>(), 0);
    // a = b - sW t3
    hipLaunchKernelGGL(lp_sub_scaled_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, (const T*)la->b.p, (const T*)la->sW.p, (const T*)la->t3.p, Np, (T*)la->a.p);
    // fp32: one refinement step of a against (I + W K) a = b, the system the solve above answers.  The fp32 factor of B leaves
    // a few 1e-6 of error in a, smooth enough in x to survive K a and then add up in the predictive mean k*' g (a cancelling sum
    // of g); the residual comes from the fp64 GEMV partials, the correction from the same L^-1 (r lives in fnew until then).
    if (la->dtype != SVGP_F64) {
      hipLaunchKernelGGL(lp_gemv_kernel<T>, dim3(unsigned(Np / 64), unsigned(npan)), dim3(k256), 0, s, (const T*)la->K.p, (const T*)la->a.p, Np, la->part.as<double>());
      hipLaunchKernelGGL(lp_resid_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->part.as<double>(), npan, Np, (const T*)la->b.p, (const T*)la->a.p, (const T*)la->W.p, (T*)la->fnew.p);
      hipLaunchKernelGGL(lp_gemv_kernel<T>, dim3(unsigned(Np / 64), unsigned(npan)), dim3(k256), 0, s, (const T*)la->K.p, (const T*)la->fnew.p, Np, la->part.as<double>());
      hipLaunchKernelGGL(lp_gemv_finish_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->part.as<double>(), npan, Np, 1, (const T*)la->sW.p, (const T*)nullptr, (T*)la->t1.p);
      launch_linv_t_gemv(la->dtype, s, la->LinvCM.p, la->t1.p, Np, la->t2.p, la->part.as<double>(), 1);
      launch_linv_t_gemv(la->dtype, s, la->LinvRM.p, la->t2.p, Np, la->t3.p, la->part.as<double>(), 0);
      hipLaunchKernelGGL(lp_refine_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, (T*)la->a.p, (const T*)la->fnew.p, (const T*)la->sW.p, (const T*)la->t3.p, Np);
    }
    // fnew = K a
    hipLaunchKernelGGL(lp_gemv_kernel<T>, dim3(unsigned(Np / 64), unsigned(npan)), dim3(k256), 0, s, (const T*)la->K.p, (const T*)la->a.p, Np, la->part.as<double>());
    hipLaunchKernelGGL(lp_gemv_finish_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->part.as<double>(), npan, Np, 0, (const T*)nullptr, (const T*)nullptr, (T*)la->fnew.p);
  });
  KCHECK(ctx, "solves");
  if (timed) HIPC(ctx, hipEventRecord(la->ev[4], s));
  LP_DISPATCH(la->dtype, T, {
    hipLaunchKernelGGL(lp_ll_kernel<T>, dim3(nblk(N)), dim3(256), 0, s, la->lik, la->lik_sigma2, (const T*)la->f.p, (const T*)la->data->y.p, N,
                       la->llv.as<double>());
    hipLaunchKernelGGL(lp_stats_kernel<T>, dim3(1), dim3(k256), 0, s, (const T*)la->f.p, (const T*)la->fnew.p, (const T*)la->a.p,
                       (const double*)la->llv.as<double>(), (const T*)la->B.p, N, Np, (const int*)la->info.as<int>(), la->res.as<double>());
  });
  KCHECK(ctx, "lp_stats");
  HIPC(ctx, hipMemcpyAsync(st, la->res.as<double>(), 7 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  if (timed) {
    float e[4] = {0, 0, 0, 0};
    for (int q = 0; q < 4; ++q) HIPC(ctx, hipEventElapsedTime(&e[q], la->ev[q], la->ev[q + 1]));
    for (int q = 0; q < 4; ++q) ms[q] += e[q];
  }
  return SVGP_OK;
}

}  // namespace

namespace {

int lp_fail_null(svgp_ctx* ctx) { return fail(ctx, SVGP_INVALID_ARG, "null argument"); }

// the Newton loop (_newton_inner_loop :256-276) and the lml at its result (:157-165, :250-254).  On return the intermediates
// (g, W, sW, a, L, L^-1, d3) belong to la->f = f_opt: when the loop converges it keeps f, whose step computed them; after maxiter
// steps f is the last fnew and one more step recomputes them there (the reference's laplace_lml does the same).
int lp_fit(svgp_ctx* ctx, svgp_laplace* la, const svgp_laplace_desc* ds, const void* f_init, double* lml_out, svgp_laplace_info* info) {
  // a call that returns an error, a rejected argument included, leaves the handle without a mode: the next warm start is cold
  const bool had_mode = la->have_mode;
  la->have_mode = false;
  int rc = check_desc(ctx, la, ds);
  if (rc) return rc;
  if (!lml_out) return lp_fail_null(ctx);
  hipStream_t s = ctx->stream;
  const size_t vb = size_t(la->Np) * la->es;
  const bool warm = ds->warm_start == 1 && had_mode && !f_init;
  rc = lp_prepare(ctx, la, ds);
  if (rc) return rc;
  if (!warm) {
    HIPC(ctx, hipMemsetAsync(la->f.p, 0, vb, s));
    if (f_init) HIPC(ctx, hipMemcpyAsync(la->f.p, f_init, size_t(la->N) * la->es, hipMemcpyHostToDevice, s));
  }
  const double rtol = std::sqrt(la->dtype == SVGP_F64 ? 2.220446049250313e-16 : 1.1920928955078125e-07);   // isapprox: sqrt(eps(T))
  double st[7] = {}, ms[4] = {0, 0, 0, 0};
  int it = 0, converged = 0;
  for (it = 1; it <= ds->maxiter; ++it) {
    rc = lp_step(ctx, la, st, ms);
    if (rc) return rc;
    if (st[6] != 0.0) break;
    if (std::sqrt(st[0]) <= rtol * std::max(std::sqrt(st[1]), std::sqrt(st[2]))) {
      converged = 1;
      break;
    }
    std::swap(la->f.p, la->fnew.p);   // (equal sizes: the two buffers trade places)
  }
  if (st[6] == 0.0 && !converged) {   // f = the last fnew: its intermediates
    it = ds->maxiter;
    rc = lp_step(ctx, la, st, ms);
    if (rc) return rc;
  }
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->iterations = std::min(it, ds->maxiter);
    info->converged = converged;
    info->chol_info = int32_t(st[6]);
    info->ms_point = ms[0];
    info->ms_chol = ms[1];
    info->ms_linv = ms[2];
    info->ms_gemv = ms[3];
  }
  if (st[6] != 0.0) {
    *lml_out = NAN;
    return fail(ctx, SVGP_NOT_POSDEF, "cholesky(I + sW K sW) failed: info " + std::to_string(int(st[6])));
  }
  *lml_out = -0.5 * st[3] + st[4] - st[5];   // _laplace_lml :250-254
  if (info) info->lml = *lml_out;
  la->have_mode = true;
  return SVGP_OK;
}

}  // namespace

extern "C" {

int32_t svgp_laplace_create(svgp_ctx* ctx, const svgp_data* data, svgp_laplace** out) {
  if (!ctx || !data || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!data->y.p) return fail(ctx, SVGP_INVALID_ARG, "the Laplace approximation needs y");
  if (data->n < 1) return fail(ctx, SVGP_INVALID_ARG, "empty data");
  if (data->n > lp_max_n(data->dtype)) return fail(ctx, SVGP_UNSUPPORTED, "N beyond the tested size of the device Cholesky");
  auto* la = new (std::nothrow) svgp_laplace();
  if (!la) return SVGP_OOM;
  la->data = data;
  la->dtype = data->dtype;
  la->d = data->d;
  la->N = data->n;
  la->Np = (data->n + kNB - 1) / kNB * kNB;
  la->es = data->dtype == SVGP_F64 ? 8 : 4;
  const size_t mb = size_t(la->Np) * la->Np * la->es, vb = size_t(la->Np) * la->es;
  hipError_t e = hipSuccess;
  struct { DevBuf* b; size_t bytes; } req[] = {
      {&la->K, mb}, {&la->B, mb}, {&la->T, mb}, {&la->LinvRM, mb}, {&la->LinvCM, mb}, {&la->Ytmp, mb},
      {&la->xs, vb * la->d}, {&la->invl_t, size_t(la->d) * la->es},
      {&la->f, vb}, {&la->fnew, vb}, {&la->g, vb}, {&la->W, vb}, {&la->sW, vb}, {&la->b, vb}, {&la->d3, vb}, {&la->a, vb},
      {&la->t1, vb}, {&la->t2, vb}, {&la->t3, vb},
      {&la->part, size_t(la->Np / kNB) * la->Np * 8}, {&la->res, (16 + SVGP_MAX_D) * 8}, {&la->invl_d, size_t(la->d) * 8},
      {&la->llv, size_t(la->Np) * 8}, {&la->info, lp_info_bytes(la->Np)}};
  for (auto& r : req)
    if (e == hipSuccess) e = r.b->alloc(r.bytes);
  for (Event& ev : la->ev)
    if (e == hipSuccess) e = ev.create(hipEventDefault);
  // T above the diagonal and L^-1 above its block diagonal are never written and must read as zero
  if (e == hipSuccess) e = hipMemsetAsync(la->T.p, 0, mb, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(la->LinvRM.p, 0, mb, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(la->LinvCM.p, 0, mb, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(la->B.p, 0, mb, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    delete la;
    return fail(ctx, e == hipErrorOutOfMemory ? SVGP_OOM : SVGP_HIP_ERROR, std::string("svgp_laplace_create: ") + hipGetErrorString(e));
  }
  *out = la;
  return SVGP_OK;
}

int32_t svgp_laplace_free(svgp_ctx* ctx, svgp_laplace* la) {
  if (!la) return SVGP_OK;
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete la;
  return SVGP_OK;
}

int32_t svgp_laplace_fit(svgp_ctx* ctx, svgp_laplace* la, const svgp_laplace_desc* desc, const void* f_init, double* lml_out,
                         svgp_laplace_info* info) {
  if (!ctx || !la) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  return lp_fit(ctx, la, desc, f_init, lml_out, info);
}

int32_t svgp_laplace_lml_grad(svgp_ctx* ctx, svgp_laplace* la, const svgp_laplace_desc* desc, const void* f_init, double* lml_out,
                              svgp_laplace_info* info, double* d_variance, double* d_inv_lengthscale) {
  if (!ctx || !la) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!d_variance || !d_inv_lengthscale) {
    la->have_mode = false;
    if (desc) {
      const int rc = check_desc(ctx, la, desc);
      if (rc) return rc;
    }
    return lp_fail_null(ctx);
  }
  int rc = lp_fit(ctx, la, desc, f_init, lml_out, info);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const int64_t N = la->N, Np = la->Np;
  const int npan = int(Np / kNB), d = la->d;
  const size_t mb = size_t(Np) * Np * la->es;
  rc = la->R.reserve(ctx, mb, "the Laplace gradient's R");
  if (rc == SVGP_OK) rc = la->X.reserve(ctx, mb, "the Laplace gradient's K R");
  if (rc) return rc;
  const int nt = int(Np / 64), nfc = (d + kLpFc - 1) / kLpFc;
  const int64_t nchunk = 16, chunk = (Np + nchunk - 1) / nchunk;
  const size_t gb = std::max(size_t(nt) * nt * nfc * (1 + kLpFc), size_t(nchunk) * Np) * 8;
  rc = la->gpart.reserve(ctx, gb, "the Laplace gradient's partial sums");
  if (rc) return rc;
  // R = sW (L^-T L^-1) sW: sum_j Linv[j][r] Linv[j][c] on the MFMA product kernel; X = K R (column-major)
  // Linv[j][r] = 0 for j < r: the contraction of tile (r, c) starts at the later of the two diagonal tiles (kMmXLow | kMmYLow)
  launch_gemm_pm(la->dtype, s, la->LinvRM.p, la->LinvRM.p, nullptr, 1.0, Np, Np, Np, 1, la->R.p, 1, kMmFull | kMmXLow | kMmYLow);
  KCHECK(ctx, "gemm_pm (R)");
  LP_DISPATCH(la->dtype, T, {
    hipLaunchKernelGGL(lp_scale_r_kernel<T>, dim3(nblk(Np), (unsigned)Np), dim3(256), 0, s, (T*)la->R.p, (const T*)la->sW.p, Np);
  });
  launch_gemm_pm(la->dtype, s, la->R.p, la->K.p, nullptr, 1.0, Np, Np, Np, 1, la->X.p, 1, kMmFull);
  KCHECK(ctx, "gemm_pm (K R)");
  LP_DISPATCH(la->dtype, T, {
    hipLaunchKernelGGL(lp_diag_krk_kernel<T>, dim3(nblk(Np), (unsigned)nchunk), dim3(256), 0, s, (const T*)la->X.p, (const T*)la->K.p, Np, chunk, la->gpart.as<double>());
    hipLaunchKernelGGL(lp_s2_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->gpart.as<double>(), int(nchunk), (const T*)la->K.p, (const T*)la->d3.p, N, Np, (T*)la->t1.p);
    // u = s2 - R (K s2)   (t1 = s2, t2 = K s2, t3 = u)
    hipLaunchKernelGGL(lp_gemv_kernel<T>, dim3(unsigned(Np / 64), unsigned(npan)), dim3(k256), 0, s, (const T*)la->K.p, (const T*)la->t1.p, Np, la->part.as<double>());
    hipLaunchKernelGGL(lp_gemv_finish_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->part.as<double>(), npan, Np, 0, (const T*)nullptr, (const T*)nullptr, (T*)la->t2.p);
    hipLaunchKernelGGL(lp_gemv_kernel<T>, dim3(unsigned(Np / 64), unsigned(npan)), dim3(k256), 0, s, (const T*)la->R.p, (const T*)la->t2.p, Np, la->part.as<double>());
    hipLaunchKernelGGL(lp_gemv_finish_kernel<T>, dim3(nblk(Np)), dim3(256), 0, s, la->part.as<double>(), npan, Np, 3, (const T*)nullptr, (const T*)la->t1.p, (T*)la->t3.p);
    hipLaunchKernelGGL(lp_kgrad_kernel<T>, dim3((unsigned)nt, (unsigned)nt, (unsigned)nfc), dim3(k256), 0, s, la->family, d, la->variance,
                       (const double*)la->invl_d.as<double>(), (const T*)la->data->x.p, la->data->ldx, N, Np, (const T*)la->R.p, (const T*)la->a.p,
                       (const T*)la->g.p, (const T*)la->t3.p, la->gpart.as<double>());
  });
  hipLaunchKernelGGL(lp_kgrad_finish_kernel, dim3((unsigned)(1 + d)), dim3(k256), 0, s, la->gpart.as<double>(), int64_t(nt) * nt, nfc, d, la->res.as<double>());
  KCHECK(ctx, "laplace gradient");
  double out[1 + SVGP_MAX_D];
  HIPC(ctx, hipMemcpyAsync(out, la->res.as<double>(), size_t(1 + d) * 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  *d_variance = out[0];
  for (int f = 0; f < d; ++f) d_inv_lengthscale[f] = out[1 + f];
  return SVGP_OK;
}

int32_t svgp_laplace_mode(svgp_ctx* ctx, svgp_laplace* la, void* f_out, void* dll_out, void* W_out) {
  if (!ctx || !la) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!la->have_mode) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_laplace_fit on this handle yet");
  const size_t b = size_t(la->N) * la->es;
  hipStream_t s = ctx->stream;
  if (f_out) HIPC(ctx, hipMemcpyAsync(f_out, la->f.p, b, hipMemcpyDeviceToHost, s));
  if (dll_out) HIPC(ctx, hipMemcpyAsync(dll_out, la->g.p, b, hipMemcpyDeviceToHost, s));
  if (W_out) HIPC(ctx, hipMemcpyAsync(W_out, la->W.p, b, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

}  // extern "C"

namespace {

// V = L^-1 (sW k(x, x*)) for uploaded test inputs (RW 3.29), optionally the mean k(x, x*)' dll (RW 3.21); V: Np x n column-major.
// xs_out: the scaled test inputs [d][n] (the prior block of cov needs them)
int lp_pred_v(svgp_ctx* ctx, svgp_laplace* la, const svgp_data* P, void* mean, DevBuf& xs_out, DevBuf& V) {
  hipStream_t s = ctx->stream;
  const int64_t N = la->N, Np = la->Np, n = P->n;
  DevBuf Kx, mdev;
  HIPC(ctx, xs_out.alloc(size_t(n) * la->d * la->es));
  HIPC(ctx, Kx.alloc(size_t(Np) * n * la->es));
  HIPC(ctx, V.alloc(size_t(Np) * n * la->es));
  if (mean) HIPC(ctx, mdev.alloc(size_t(n) * la->es));
  LP_DISPATCH(la->dtype, T, {
    hipLaunchKernelGGL(lp_scale_kernel<T>, dim3(nblk(n), (unsigned)la->d), dim3(256), 0, s, (const T*)P->x.p, P->ldx, n, n,
                       (const T*)la->invl_t.p, (T*)xs_out.p);
    hipLaunchKernelGGL(lp_kcross_kernel<T>, dim3(nblk(Np), (unsigned)n), dim3(256), 0, s, la->family, la->d, T(la->variance),
                       (const T*)la->xs.p, Np, N, Np, (const T*)xs_out.p, n, n, T(0), 0, (T*)Kx.p, Np);
    if (mean)
      hipLaunchKernelGGL(lp_colreduce_kernel<T>, dim3((unsigned)n), dim3(k256), 0, s, (const T*)Kx.p, Np, Np, (const T*)la->g.p, 0, 0.0, (T*)mdev.p);
    hipLaunchKernelGGL(lp_rowscale_kernel<T>, dim3(nblk(Np), (unsigned)n), dim3(256), 0, s, (T*)Kx.p, Np, Np, (const T*)la->sW.p);
    // V(i, j) = sum_k Linv(i, k) S(k, j): LinvCM column-major
    hipLaunchKernelGGL(lp_gemm_kernel<T>, dim3(unsigned((Np + 63) / 64), unsigned((n + 63) / 64)), dim3(k256), 0, s, Np, n, Np,
                       (const T*)la->LinvCM.p, int64_t(1), Np, (const T*)Kx.p, int64_t(1), Np, (T*)V.p, Np, 0);
  });
  KCHECK(ctx, "laplace predict");
  if (mean) HIPC(ctx, hipMemcpyAsync(mean, mdev.p, size_t(n) * la->es, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

struct DataHold {   // test inputs uploaded for one call
  svgp_ctx* ctx;
  svgp_data* D = nullptr;
  ~DataHold() { if (D) svgp_data_free(ctx, D); }
};

// cov(x*, y*) = k(x*, y*) - Vx' Vy  (:458-463) into a device buffer
int lp_cov(svgp_ctx* ctx, svgp_laplace* la, const void* xs_a, int64_t na, const void* Va, const void* xs_b, int64_t nb, const void* Vb,
           void* host_out) {
  hipStream_t s = ctx->stream;
  const int64_t Np = la->Np;
  DevBuf C;
  HIPC(ctx, C.alloc(size_t(na) * nb * la->es));
  LP_DISPATCH(la->dtype, T, {
    hipLaunchKernelGGL(lp_kcross_kernel<T>, dim3(nblk(na), (unsigned)nb), dim3(256), 0, s, la->family, la->d, T(la->variance),
                       (const T*)xs_a, na, na, na, (const T*)xs_b, nb, nb, T(0), 0, (T*)C.p, na);
    hipLaunchKernelGGL(lp_gemm_kernel<T>, dim3(unsigned((na + 63) / 64), unsigned((nb + 63) / 64)), dim3(k256), 0, s, na, nb, Np,
                       (const T*)Va, Np, int64_t(1), (const T*)Vb, int64_t(1), Np, (T*)C.p, na, 1);
  });
  KCHECK(ctx, "laplace cov");
  HIPC(ctx, hipMemcpyAsync(host_out, C.p, size_t(na) * nb * la->es, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

}  // namespace

extern "C" {

int32_t svgp_laplace_predict(svgp_ctx* ctx, svgp_laplace* la, int32_t layout, int64_t n, const void* x_host, void* mean_out, void* var_out,
                             void* cov_out) {
  if (!ctx || !la || !x_host) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!la->have_mode) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_laplace_fit on this handle yet");
  DataHold h{ctx};
  int rc = svgp_data_upload(ctx, la->dtype, layout, la->d, n, x_host, nullptr, &h.D);
  if (rc) return rc;
  DevBuf xs, V;
  rc = lp_pred_v(ctx, la, h.D, mean_out, xs, V);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  if (var_out) {
    DevBuf vd;
    HIPC(ctx, vd.alloc(size_t(n) * la->es));
    LP_DISPATCH(la->dtype, T, {
      hipLaunchKernelGGL(lp_colreduce_kernel<T>, dim3((unsigned)n), dim3(k256), 0, s, (const T*)V.p, la->Np, la->Np, (const T*)nullptr, 1,
                         la->variance, (T*)vd.p);
    });
    KCHECK(ctx, "laplace var");
    HIPC(ctx, hipMemcpyAsync(var_out, vd.p, size_t(n) * la->es, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
  }
  if (cov_out) return lp_cov(ctx, la, xs.p, n, V.p, xs.p, n, V.p, cov_out);
  return SVGP_OK;
}

int32_t svgp_laplace_predict_cross_cov(svgp_ctx* ctx, svgp_laplace* la, int32_t layout, int64_t nx, const void* x_host, int64_t ny,
                                       const void* y_host, void* cov_out) {
  if (!ctx || !la || !x_host || !y_host || !cov_out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!la->have_mode) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_laplace_fit on this handle yet");
  DataHold hx{ctx}, hy{ctx};
  int rc = svgp_data_upload(ctx, la->dtype, layout, la->d, nx, x_host, nullptr, &hx.D);
  if (!rc) rc = svgp_data_upload(ctx, la->dtype, layout, la->d, ny, y_host, nullptr, &hy.D);
  if (rc) return rc;
  DevBuf xsa, Va, xsb, Vb;
  rc = lp_pred_v(ctx, la, hx.D, nullptr, xsa, Va);
  if (!rc) rc = lp_pred_v(ctx, la, hy.D, nullptr, xsb, Vb);
  if (rc) return rc;
  return lp_cov(ctx, la, xsa.p, nx, Va.p, xsb.p, ny, Vb.p, cov_out);
}

}  // extern "C"
