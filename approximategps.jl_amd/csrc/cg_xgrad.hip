// cg_xgrad.hip — the gradient of the exact GP's log marginal likelihood with respect to the data inputs (svgp_cg_lml_grad_inputs:
// cg_api.hip holds the host side).  With U = [alpha, w_1 .. w_T], P = [alpha, p_1 .. p_T] of the fit (p_t = z_t, or P^-1 z_t with a
// preconditioner), g = d kappa / d(r^2), the left panel Lp = [alpha, w_t .., p_t ..] and the right panel Rp = [alpha, -p_t / 2T ..,
// -w_t / 2T ..] of 2T + 1 columns each:
//   x_bar[c, i] = d lml / d x_ic = invl_c sum_s Lp[i, s] sum_j 2 g(r_ij^2) (xs_ic - xs_jc) Rp[j, s]
// cg_xgrad_kernel is the gradient form of cg_sample_kernel (cg_sample.hip) over the data rows alone, with the points the data themselves:
// every 16 x 16 tile of K(X, X) is generated TRANSPOSED on the MFMA once per (column block, coordinate block), kappa and 2 g come from
// one argument, the coordinate difference is taken per ENTRY before the product (no expanded square, no division by r), and one MFMA
// product with the right panel's column block runs per coordinate of the block; the fp32 d <= 8 by-differences path is kept, and r^2 of
// the diagonal entry is exactly 0 (kmv_kernel's P = R rule), so that entry contributes exactly nothing.  The epilogue contracts the
// accumulators with the left panel IN REGISTERS: a lane holds out'[s][i] for its four columns s and its point i, multiplies by
// Lp[i, s], sums its four products, and the four lanes of a point are added in ascending order; nothing S x d x N is ever written.
// The partial sums of a column block go to part[block][c][i] in fp64; cg_xgrad_sum_kernel adds the blocks in ascending order, scales by
// invl_c and rounds once to the data dtype.  No atomics, every sum has a fixed order: repeated calls are bitwise equal.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {

namespace {

constexpr int kCgxKC = 32;   // contraction rows per LDS chunk (Np is a multiple of it)

// the coordinate block and the groups of 16 points a wave owns, for two waves per SIMD (<= 256 VGPRs + AGPRs) without spills:
// profiles/cg/kernel_resources_xgrad.txt.  cg_sample_kernel's gradient-form rules (this kernel carries no value accumulator)
template <typename T, int DREG>
constexpr int cgx_coord_block() {
  return (sizeof(T) == 8 && DREG > 32) ? 4 : 8;
}
template <typename T, int DREG>
constexpr int cgx_point_groups() {
  return (sizeof(T) == 8 || DREG == 8) ? 1 : 2;
}

// One workgroup = 4 waves; a wave owns PG groups of 16 points, one 16-column block of the panels (a.s0) and the coordinates
// e0 .. e0 + CB - 1.  The data rows hold -2 xs_j (then xs_j = -rows / 2, exact) or, for fp32 with d <= 8 (DIFF), x_j itself
// (launch_kmv_prep, raw).  Point i is row i.
template <typename T, int DREG, int CB>
__global__ void __launch_bounds__(256, 2) cg_xgrad_kernel(CgXgradArgs a) {
  constexpr int KS = DREG / 4, KC = kCgxKC, NW = 4;
  constexpr int PG = cgx_point_groups<T, DREG>();
  constexpr int ZLD = KC + 16, PLD = 16 + 4;
  constexpr bool DIFF = sizeof(T) == 4 && DREG <= 8;
  static_assert(!DIFF || DREG <= CB, "the by-differences form keeps every coordinate in one block");
  using acc_t = typename Mfma16<T>::acc_t;
  __shared__ T zc[DREG * ZLD];   // [f][kk]  rows of the chunk (MFMA A operand of the generation)
  __shared__ T pc[KC * PLD];     // [kk][j]  right panel rows of the chunk, the launch's column block
  __shared__ T tc[KC];           // [kk]     bias |xs_j|^2
  const T* __restrict__ rows = static_cast<const T*>(a.rows);
  const T* __restrict__ bias = static_cast<const T*>(a.bias);
  const T* __restrict__ invl = static_cast<const T*>(a.invl);
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ Lp = static_cast<const T*>(a.Lp);
  const T* __restrict__ Rp = static_cast<const T*>(a.Rp) + a.s0 * a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
  const int d = a.d, family = a.family, e0 = a.e0;
  const int ne = d - e0 < CB ? d - e0 : CB;   // coordinates of this launch
  const int64_t N = a.N, Np = a.Np;
  const int ncol = int(a.S - a.s0 < 16 ? a.S - a.s0 : 16);   // columns of this launch
  const T variance = T(a.variance);
  const int64_t p0 = (int64_t(blockIdx.x) * NW + wave) * (PG * 16);
  T xb[PG][KS], xn[PG];
  T xall[DIFF ? PG : 1][DIFF ? DREG : 1];                  // DIFF: every feature of point c, unscaled
  T il[DIFF ? DREG : 1];
  [[maybe_unused]] T xsb[DIFF ? 1 : PG][DIFF ? 1 : CB];    // otherwise: the block's scaled coordinates of point c
  if constexpr (DIFF) {
#pragma unroll
    for (int f = 0; f < DREG; ++f) il[f] = (f < d) ? invl[f] : T(0);
  }
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    int64_t pt = p0 + g * 16 + c;
    pt = pt < N ? pt : N - 1;
    if constexpr (DIFF) {
#pragma unroll
      for (int f = 0; f < DREG; ++f) xall[g][f] = (f < d) ? x[int64_t(f) * a.ldx + pt] : T(0);
    } else {
#pragma unroll
      for (int e = 0; e < CB; ++e) xsb[g][e] = (e < ne) ? x[int64_t(e0 + e) * a.ldx + pt] * invl[e0 + e] : T(0);
    }
    T s2 = T(0);
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int f = 4 * q + kq;
      const T v = (f < d) ? x[int64_t(f) * a.ldx + pt] * invl[f] : T(0);
      xb[g][q] = v;
      s2 = fma(v, v, s2);
    }
    s2 += __shfl_xor(s2, 16);
    s2 += __shfl_xor(s2, 32);
    xn[g] = s2;
  }
  acc_t gacc[PG][CB];
#pragma unroll
  for (int g = 0; g < PG; ++g)
#pragma unroll
    for (int e = 0; e < CB; ++e) gacc[g][e] = acc_t{0, 0, 0, 0};

  for (int64_t k0 = 0; k0 < Np; k0 += KC) {
    __syncthreads();   // the previous chunk has been read
    for (int idx = tid; idx < DREG * KC; idx += 256) {
      const int f = idx / KC, kk = idx % KC;
      zc[f * ZLD + kk] = (f < d) ? rows[int64_t(f) * Np + k0 + kk] : T(0);
    }
    for (int idx = tid; idx < KC * 16; idx += 256) {   // the panel is column-major: kk runs fastest over the threads
      const int j = idx / KC, kk = idx % KC;
      pc[kk * PLD + j] = (j < ncol && k0 + kk < N) ? Rp[int64_t(j) * N + k0 + kk] : T(0);
    }
    if (tid < KC) tc[tid] = bias[k0 + tid];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < KC / 16; ++h) {
      T za[KS], pa[4], tb[4];
      int kr[4];
#pragma unroll
      for (int q = 0; q < KS; ++q) za[q] = zc[(4 * q + kq) * ZLD + h * 16 + c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        kr[r] = h * 16 + Mfma16<T>::row(lane, r);   // the row this lane's register r holds after the generation
        tb[r] = tc[kr[r]];
        pa[r] = pc[kr[r] * PLD + c];
      }
      [[maybe_unused]] T zr[DIFF ? 4 : 1][DIFF ? DREG : 1];   // DIFF: every feature of the lane's four rows (the chunk holds x itself)
      if constexpr (DIFF) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int f = 0; f < DREG; ++f) zr[r][f] = zc[f * ZLD + kr[r]];
      }
#pragma unroll
      for (int g = 0; g < PG; ++g) {
        if (p0 + g * 16 >= N) break;   // wave-uniform
        acc_t t;
        [[maybe_unused]] T dfr[DIFF ? 4 : 1][DIFF ? DREG : 1];   // DIFF: (x_f - X_f) invl_f of the lane's four entries
        if constexpr (DIFF) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T s2 = T(0);
#pragma unroll
            for (int f = 0; f < DREG; ++f) {
              const T df = (xall[g][f] - zr[r][f]) * il[f];
              dfr[r][f] = df;
              s2 = fma(df, df, s2);
            }
            t[r] = s2;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = tb[r] + xn[g];
#pragma unroll
          for (int q = 0; q < KS; ++q) t = Mfma16<T>::mma(za[q], xb[g][q], t);
        }
        acc_t td;   // 2 g of the tile
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          T r2 = t[r] < T(0) ? T(0) : t[r];
          // point i is row i: r^2 of the diagonal is exactly 0 (kmv_kernel's rule), and its coordinate differences are exactly 0 too
          if (k0 + kr[r] == p0 + g * 16 + c) r2 = T(0);
          td[r] = kappa_2g<T>(family, r2, variance, kappa<T>(family, r2, variance));
        }
#pragma unroll
        for (int e = 0; e < CB; ++e) {
          if (e >= ne) break;   // wave-uniform
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T bv = td[r];
            if constexpr (DIFF) {
              bv *= dfr[r][e < DREG ? e : 0];
            } else {
              bv *= fma(T(0.5), zc[(e0 + e) * ZLD + kr[r]], xsb[g][e]);   // xs_ic - xs_jc from the row -2 xs_jc, rounded once
            }
            gacc[g][e] = Mfma16<T>::mma(pa[r], bv, gacc[g][e]);
          }
        }
      }
    }
  }
  // the contraction with the left panel: register r of gacc[g][e] is out'[s0 + row(lane, r)][point c of group g]
  double* __restrict__ o = static_cast<double*>(a.part) + int64_t(a.blk) * d * N;
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    if (p0 + g * 16 >= N) break;   // wave-uniform: every lane of the wave takes part in the exchanges below
    const int64_t pi = p0 + g * 16 + c;
    const int64_t pt = pi < N ? pi : N - 1;
    double lp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int sl = Mfma16<T>::row(lane, r);
      lp[r] = sl < ncol ? double(Lp[(a.s0 + sl) * N + pt]) : 0.0;
    }
#pragma unroll
    for (int e = 0; e < CB; ++e) {
      if (e >= ne) break;   // wave-uniform
      double v = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) v = fma(double(gacc[g][e][r]), lp[r], v);
      const double v0 = __shfl(v, c), v1 = __shfl(v, c + 16), v2 = __shfl(v, c + 32), v3 = __shfl(v, c + 48);
      if (kq == 0 && pi < N) o[int64_t(e0 + e) * N + pi] = ((v0 + v1) + v2) + v3;
    }
  }
}

// out[c ldo + i] = T(invl_c sum over the column blocks, ascending, of part[blk][c][i]), in fp64
template <typename T>
__global__ void cg_xgrad_sum_kernel(const double* __restrict__ part, int nblk, int d, int64_t N, const T* __restrict__ invl, T* __restrict__ out,
                                    int64_t ldo) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= N) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t(b) * d + c) * N + i];
  out[int64_t(c) * ldo + i] = T(double(invl[c]) * s);
}

template <typename T, int DREG>
void launch_cgx_d(hipStream_t s, const CgXgradArgs& a0, void* out, int64_t ldo) {
  CgXgradArgs a = a0;
  constexpr int CB = cgx_coord_block<T, DREG>();
  const int64_t per = 4 * 16 * cgx_point_groups<T, DREG>();   // points per workgroup
  const dim3 grid((unsigned)((a.N + per - 1) / per));
  int nblk = 0;
  for (int64_t s0 = 0; s0 < a.S; s0 += 16, ++nblk)   // one 16-column block of the panels
    for (int e0 = 0; e0 < a.d; e0 += CB) {           // and one block of coordinates per launch
      a.s0 = s0;
      a.blk = nblk;
      a.e0 = e0;
      hipLaunchKernelGGL((cg_xgrad_kernel<T, DREG, CB>), grid, dim3(256), 0, s, a);
    }
  hipLaunchKernelGGL(cg_xgrad_sum_kernel<T>, dim3((unsigned)((a.N + 255) / 256), (unsigned)a.d), dim3(256), 0, s, (const double*)a.part, nblk, a.d,
                     a.N, (const T*)a.invl, (T*)out, ldo);
}

template <typename T>
void launch_cgx_t(hipStream_t s, const CgXgradArgs& a, void* out, int64_t ldo) {   // the DREG of launch_kmv_p: the data rows' layout follows it
  if (a.d <= 4) launch_cgx_d<T, 4>(s, a, out, ldo);
  else if (a.d <= 8) launch_cgx_d<T, 8>(s, a, out, ldo);
  else if (a.d <= 16) launch_cgx_d<T, 16>(s, a, out, ldo);
  else if (a.d <= 32) launch_cgx_d<T, 32>(s, a, out, ldo);
  else launch_cgx_d<T, 64>(s, a, out, ldo);
}

}  // namespace

void launch_cg_xgrad(int dtype, hipStream_t s, const CgXgradArgs& a, void* out, int64_t ldo) {
  if (dtype == 0) launch_cgx_t<double>(s, a, out, ldo); else launch_cgx_t<float>(s, a, out, ldo);
}

}  // namespace svgp
