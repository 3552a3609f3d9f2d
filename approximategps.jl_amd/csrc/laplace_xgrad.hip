// laplace_xgrad.hip — the gradient of the Laplace approximation's approx_lml with respect to the data inputs
// (svgp_laplace_lml_grad_inputs: laplace.hip holds the host side).  With the pair weight of lp_kgrad_kernel,
//   P_ik = (a_i a_k - R_ik + u_i g_k + g_i u_k) / 2      (the implicit term d f_opt / d x is in it through u),
// s = invl .* x and kappa' = d kappa / d r2 of the unit-variance kernel:
//   x_bar[f, i] = d lml / d x_if = 4 variance invl_f sum_k P_ik kappa'(r2_ik) (s_if - s_kf)
// (2 for d r2 / d s_if, 2 for the row and the column of the symmetric P o dK; the jitter does not depend on x).
//
// Work split.  Workgroup (ti, seg): the 64 rows of tile ti against the column tiles of segment seg, the full square, in ascending
// order.  Two phases per 64 x 64 tile, both on the same 256 threads:
//   A  thread (il, q) holds row i = 64 ti + il and the 16 columns c = q, q + 4, ..., four at a time: the R tile is read coalesced
//      (the only N^2 operand), r2 is summed from per-entry differences of the scaled coordinates (row tile and column tile staged in LDS in fp64,
//      the column's a, g, u beside them), kappa' comes from one evaluation per entry, and H_ik = P_ik kappa'_ik goes to LDS.
//      Padded rows and columns get H = 0 by selection.
//   B  thread (il, q) holds row i and the features f = q, q + 4, ... (at most DQ = ceil(d / 4) rounded up to 2, 4, 8 or 16 of them,
//      in registers with their accumulators): acc_f += H_ic (s_if - s_cf) over the 64 columns in ascending order, the difference
//      taken per entry BEFORE the product.  The diagonal entry contributes exactly 0: s_if - s_if = 0 and H_ii is finite.
// So H is generated once per tile whatever d is, every x_bar[f, i] of a segment is summed by one thread in a fixed order, and no
// reduction across threads exists.  The segments' sums go to part[seg][f][i] (fp64); lp_xgrad_finish_kernel adds them in ascending
// order, scales and rounds once to the data dtype.  No atomics: repeated calls are bitwise equal.
// r2 by differences and not by the MFMA distance form |s_i|^2 + |s_k|^2 - 2 s_i's_k: phase B needs the differences anyway, they cost
// one LDS broadcast read and two fp64 operations per feature beside the exponential and the N^2 read of R, and the Matern kappa' has
// a sqrt(r2) that the expanded square's cancellation near r2 = 0 would disturb.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {

namespace {

constexpr int kLpxT = 64;   // rows and columns of a tile

// d kappa / d r2 of the unit-variance kernel (the dk of laplace.hip's lp_kappa_d): finite at r2 = 0 for every family
__device__ __forceinline__ double lpx_dkappa(int family, double r2) {
  if (family == KSE) return -0.5 * exp(-0.5 * r2);
  if (family == KM32) return -1.5 * exp(-1.7320508075688772935 * sqrt(r2));
  const double s = 2.2360679774997896964 * sqrt(r2);
  return -(5.0 / 6.0) * (1.0 + s) * exp(-s);
}

// LDS of the kernel in doubles: xi[4 DQ][64], xk[64][4 DQ + 2], vk[3][64], H[64][64]
template <int DQ>
constexpr int lpx_lds_doubles() {
  return kLpxT * 4 * DQ + kLpxT * (4 * DQ + 2) + 3 * kLpxT + kLpxT * kLpxT;
}

// Feature f lives in slot (f & 3) DQ + (f >> 2): the features of wave q are the DQ consecutive slots from q DQ.  Slots of features
// >= d hold 0 in both tiles and add 0.
template <typename T, int DQ>
__global__ void __launch_bounds__(k256) lp_xgrad_kernel(LpXgradArgs p) {
  constexpr int DP = 4 * DQ, XLD = DP + 2, NJ = kLpxT / 4, JG = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* xi_s = reinterpret_cast<double*>(smem_raw);   // [slot][il]
  double* xk_s = xi_s + kLpxT * DP;                     // [c][slot], row stride XLD
  double* vk_s = xk_s + kLpxT * XLD;                    // a, g, u of the columns
  double* H_s = vk_s + 3 * kLpxT;                       // [c][il]
  const T* __restrict__ x = static_cast<const T*>(p.x);
  const T* __restrict__ R = static_cast<const T*>(p.R);
  const T* __restrict__ av = static_cast<const T*>(p.a);
  const T* __restrict__ gv = static_cast<const T*>(p.g);
  const T* __restrict__ uv = static_cast<const T*>(p.u);
  const double* __restrict__ invl = p.invl;
  const int t = threadIdx.x, il = t & 63, q = __builtin_amdgcn_readfirstlane(t >> 6);
  const int d = p.d, family = p.family;
  const int64_t n = p.n, np = p.np;
  const int64_t i = int64_t(blockIdx.x) * kLpxT + il;   // < np: the grid has np / 64 row tiles
  const int seg = blockIdx.y;

  for (int e = t; e < kLpxT * DP; e += k256) {   // the row tile's scaled coordinates, once
    const int s = e >> 6, c = e & 63, f = (s / DQ) + 4 * (s % DQ);
    const int64_t ii = int64_t(blockIdx.x) * kLpxT + c;
    xi_s[e] = (f < d && ii < n) ? double(x[int64_t(f) * p.ldx + ii]) * invl[f] : 0.0;
  }
  const double ai = double(av[i]), gi = double(gv[i]), ui = double(uv[i]);
  __syncthreads();
  double xr[DQ], acc[DQ];
#pragma unroll
  for (int m = 0; m < DQ; ++m) {
    xr[m] = xi_s[(q * DQ + m) * kLpxT + il];
    acc[m] = 0.0;
  }

  const int64_t ntc = (n + kLpxT - 1) / kLpxT;   // column tiles that hold a point
  const int64_t tk0 = int64_t(seg) * p.tps;
  const int64_t tk1 = int64_t(blockIdx.x) * kLpxT >= n ? tk0 : (tk0 + p.tps < ntc ? tk0 + p.tps : ntc);   // a row tile of padding: nothing
  for (int64_t tk = tk0; tk < tk1; ++tk) {
    const int64_t k0 = tk * kLpxT;
    __syncthreads();   // phase B of the previous tile has read xk_s and H_s
    for (int e = t; e < kLpxT * DP; e += k256) {
      const int s = e >> 6, c = e & 63, f = (s / DQ) + 4 * (s % DQ);
      const int64_t k = k0 + c;
      xk_s[c * XLD + s] = (f < d && k < n) ? double(x[int64_t(f) * p.ldx + k]) * invl[f] : 0.0;
    }
    if (t < 3 * kLpxT) {
      const int w = t >> 6;
      const T* __restrict__ v = w == 0 ? av : (w == 1 ? gv : uv);
      vk_s[t] = double(v[k0 + il]);   // k0 + il < np
    }
    __syncthreads();
    // phase A, four columns at a time (the registers of four exponentials, not sixteen)
#pragma unroll 1
    for (int j0 = 0; j0 < NJ; j0 += JG) {
      T Rv[JG];   // issued first: the loads fly under the distance loop
      double r2[JG];
#pragma unroll
      for (int j = 0; j < JG; ++j) {
        Rv[j] = R[i + (k0 + q + 4 * (j0 + j)) * np];
        r2[j] = 0.0;
      }
      for (int f = 0; f < d; ++f) {
        const int s = (f & 3) * DQ + (f >> 2);
        const double xv = xi_s[s * kLpxT + il];
#pragma unroll
        for (int j = 0; j < JG; ++j) {
          const double df = xv - xk_s[(q + 4 * (j0 + j)) * XLD + s];
          r2[j] = fma(df, df, r2[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < JG; ++j) {
        const int c = q + 4 * (j0 + j);
        const double P = 0.5 * (ai * vk_s[c] - double(Rv[j]) + ui * vk_s[kLpxT + c] + gi * vk_s[2 * kLpxT + c]);
        const double h = P * lpx_dkappa(family, r2[j]);
        H_s[c * kLpxT + il] = (i < n && k0 + c < n) ? h : 0.0;
      }
    }
    __syncthreads();
    // phase B
#pragma unroll 4
    for (int c = 0; c < kLpxT; ++c) {
      const double h = H_s[c * kLpxT + il];
      const double* __restrict__ xc = xk_s + c * XLD + q * DQ;
#pragma unroll
      for (int m = 0; m < DQ; ++m) acc[m] = fma(h, xr[m] - xc[m], acc[m]);
    }
  }
  if (i < n) {
#pragma unroll
    for (int m = 0; m < DQ; ++m) {
      const int f = q + 4 * m;
      if (f < d) p.part[(int64_t(seg) * d + f) * np + i] = acc[m];
    }
  }
}

// out[f ldo + i] = T(4 variance invl_f sum over the segments, ascending, of part[seg][f][i])
template <typename T>
__global__ void lp_xgrad_finish_kernel(const double* __restrict__ part, int nseg, int d, int64_t n, int64_t np, double variance,
                                       const double* __restrict__ invl, T* __restrict__ out, int64_t ldo) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int f = blockIdx.y;
  if (i >= n) return;
  double s = 0.0;
  for (int b = 0; b < nseg; ++b) s += part[(int64_t(b) * d + f) * np + i];
  out[int64_t(f) * ldo + i] = T(4.0 * variance * invl[f] * s);
}

// out[f ldo + i] = v for i < n, f < d
template <typename T>
__global__ void lp_xfill_kernel(int64_t n, T v, T* __restrict__ out, int64_t ldo) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[int64_t(blockIdx.y) * ldo + i] = v;
}

template <typename T, int DQ>
void launch_lpx_d(hipStream_t s, const LpXgradArgs& a, int nseg) {
  constexpr int lds = lpx_lds_doubles<DQ>() * 8;
  set_max_lds(reinterpret_cast<const void*>(lp_xgrad_kernel<T, DQ>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL((lp_xgrad_kernel<T, DQ>), dim3(unsigned(a.np / kLpxT), unsigned(nseg)), dim3(k256), lds, s, a);
}

template <typename T>
void launch_lpx_t(hipStream_t s, const LpXgradArgs& a0, void* out, int64_t ldo) {
  LpXgradArgs a = a0;
  int nseg = 0;
  lp_xgrad_plan(a.np, &nseg, &a.tps);
  if (a.d <= 8) launch_lpx_d<T, 2>(s, a, nseg);
  else if (a.d <= 16) launch_lpx_d<T, 4>(s, a, nseg);
  else if (a.d <= 32) launch_lpx_d<T, 8>(s, a, nseg);
  else launch_lpx_d<T, 16>(s, a, nseg);
  hipLaunchKernelGGL(lp_xgrad_finish_kernel<T>, dim3(unsigned((a.n + 255) / 256), unsigned(a.d)), dim3(256), 0, s, (const double*)a.part, nseg,
                     a.d, a.n, a.np, a.variance, a.invl, (T*)out, ldo);
}

}  // namespace

// The column segments of a row tile: enough workgroups to fill the chip at every N (about 1024), at most one per column tile.  From Np alone
void lp_xgrad_plan(int64_t np, int* nseg, int* tps) {
  const int nt = int(np / kLpxT);
  int want = (1024 + nt - 1) / nt;
  want = want < 1 ? 1 : (want > nt ? nt : want);
  *tps = (nt + want - 1) / want;
  *nseg = (nt + *tps - 1) / *tps;
}

void launch_lp_xgrad(int dtype, hipStream_t s, const LpXgradArgs& a, void* out, int64_t ldo) {
  if (dtype == 0) launch_lpx_t<double>(s, a, out, ldo); else launch_lpx_t<float>(s, a, out, ldo);
}

void launch_lp_xfill(int dtype, hipStream_t s, int64_t n, int d, double v, void* out, int64_t ldo) {
  const dim3 grid(unsigned((n + 255) / 256), unsigned(d));
  if (dtype == 0) hipLaunchKernelGGL(lp_xfill_kernel<double>, grid, dim3(256), 0, s, n, v, (double*)out, ldo);
  else hipLaunchKernelGGL(lp_xfill_kernel<float>, grid, dim3(256), 0, s, n, float(v), (float*)out, ldo);
}

}  // namespace svgp
