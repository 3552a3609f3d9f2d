// sample_grad.hip — input gradients of the pathwise function samples (svgp_sampler_eval_grad: sample_api.hip holds the host side).
//   d f_s / d x_c (x) = invl_c [ - sum_l sin(phase_l) omega_lc (amp w_sl) + 2 sum_i g(r_i^2) (xs_c - zs_ic) V_is ],    g = variance dkappa / d(r^2)
// The kernel follows sample_eval_kernel (sample.hip): one contraction index k over the L features, then the Mp inducing points; every
// 16 x 16 tile is generated transposed on the MFMA and fed straight back to it as the B operand, nothing reaches LDS or memory.  Per tile
// it generates TWO functions of the same argument - cos and -sin of the phase (one range reduction), kappa and 2 g of r^2 (one exp) - and
// accumulates 1 + CB products: the value (the very chain of sample_eval_kernel: same phase, same kcos / kappa, k ascending, so the values
// are bitwise svgp_sampler_eval's) and one per coordinate c of the launch's coordinate block:
//   feature row   A = panel[k][s] omega_kc,   B = -sin(phase)             (the row's omega is already in LDS: it is the generation's A operand)
//   inducing row  A = panel[k][s] = V_is,     B = 2 g(r^2) (xs_c - zs_kc)  (the difference per ENTRY, before the product: x_c sum g V - sum g z_c V
//                                                                         cancels absolutely at eps |xs| |sum g V|)
// invl_c multiplies the finished sum.  A wave owns one 16-column block of the panel (NSB = 1): the accumulators are (1 + CB) PG blocks, and
// with one generation per (column block, coordinate block) pair, ceil(S / 16) ceil(d / CB) regenerations are as few as any other split of
// the same registers gives when d >= S / 16.  Fixed-order sums, no atomics; a point's gradient depends on its own MFMA column alone.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {

namespace {

// the value path's own functions and constants (sample.hip keeps its copies in an unnamed namespace)
__device__ __forceinline__ double kcos(double v) { return cos(v); }
__device__ __forceinline__ float kcos(float v) { return cosf(v); }
// the sine on its own: a fused sincos is not guaranteed to return cos's bits, and the values must be svgp_sampler_eval's.  The compiler
// merges the two calls' range reductions where they are the same instructions
__device__ __forceinline__ double ksin(double v) { return sin(v); }
__device__ __forceinline__ float ksin(float v) { return sinf(v); }

constexpr int kGradKC = 32;   // contraction rows per LDS chunk: sample.hip's kSampleKC (Lp and Mp are multiples of it)

// coordinates per launch: 8, and 4 for the widest f64 fragment (64 features: 64 registers of x and row fragments; with 8 coordinates
// the two-wave bound spilled 72 VGPRs)
template <typename T, int DREG>
constexpr int grad_coord_block() {
  return (sizeof(T) == 8 && DREG > 32) ? 4 : 8;
}

// groups of 16 points a wave owns: as many as keep the kernel at two waves per SIMD (<= 256 VGPRs + AGPRs).  A group costs (1 + CB)
// accumulator blocks, twice as wide in f64 (72 registers a group there: two groups measured 340), and in the fp32 by-differences form of
// 8 features the 8 unscaled coordinates of the point and the 32 differences of the tile (two groups: 316)
template <typename T, int DREG>
constexpr int grad_point_groups() {
  return (sizeof(T) == 8 || DREG == 8) ? 1 : 2;
}

// 2 g(r^2) = 2 variance dkappa / d(r^2): kappa_2g<T> of device_common.hpp, beside kappa<T>

// One workgroup = 4 waves; a wave owns PG groups of 16 points, the 16 samples s0 .. s0 + 15 and the coordinates e0 .. e0 + CB - 1.
// The inducing rows of the chunk hold -2 zs (then zs = -rows / 2, exact) or, for fp32 with d <= 8 (DIFF), z itself: there the scaled
// difference (x_f - z_f) invl_f that forms r^2 is the gradient's factor too, taken of the UNSCALED coordinates as sample.hip explains.
template <typename T, int DREG>
__global__ void __launch_bounds__(256, 2) sample_grad_kernel(SampleGradArgs ga) {
  constexpr int KS = DREG / 4, KC = kGradKC, NW = 4, CB = grad_coord_block<T, DREG>();
  constexpr int PG = grad_point_groups<T, DREG>();
  constexpr int ZLD = KC + 16, PLD = 16 + 4;
  constexpr bool DIFF = sizeof(T) == 4 && DREG <= 8;   // sample_eval_kernel's DIFF: the layout sample_rows_kernel gave the rows (raw)
  static_assert(!DIFF || DREG <= CB, "the by-differences form keeps every coordinate in one block");
  using acc_t = typename Mfma16<T>::acc_t;
  __shared__ T zc[DREG * ZLD];   // [f][kk]  rows of the chunk
  __shared__ T pc[KC * PLD];     // [kk][j]  panel rows of the chunk, the launch's 16 columns
  __shared__ T tc[KC];           // [kk]     bias
  const SampleEvalArgs& a = ga.v;
  const T* __restrict__ rows = static_cast<const T*>(a.rows);
  const T* __restrict__ bias = static_cast<const T*>(a.bias);
  const T* __restrict__ panel = static_cast<const T*>(a.panel);
  const T* __restrict__ invl = static_cast<const T*>(a.invl);
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ mux = static_cast<const T*>(a.mux);
  T* __restrict__ out = static_cast<T*>(a.out);
  T* __restrict__ gout = static_cast<T*>(ga.grad);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
  const int d = a.d, family = a.family, e0 = ga.e0;
  const int ne = d - e0 < CB ? d - e0 : CB;     // coordinates of this launch
  const bool val = out != nullptr && e0 == 0;   // the values go out with the first coordinate block
  const int64_t len = a.len, Kp = a.Lp + a.Mp;
  const T variance = T(a.variance);
  const int64_t p0 = (int64_t(blockIdx.x) * NW + wave) * (PG * 16);
  T xb[PG][KS], xn[PG];
  T xall[DIFF ? PG : 1][DIFF ? DREG : 1];   // DIFF: every feature of point c, unscaled
  T il[DIFF ? DREG : 1];
  T xsb[DIFF ? 1 : PG][DIFF ? 1 : CB];      // otherwise: the block's scaled coordinates of point c
  if constexpr (DIFF) {
#pragma unroll
    for (int f = 0; f < DREG; ++f) il[f] = (f < d) ? invl[f] : T(0);
  }
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    int64_t pt = p0 + g * 16 + c;
    pt = pt < len ? pt : len - 1;
    if constexpr (DIFF) {
#pragma unroll
      for (int f = 0; f < DREG; ++f) xall[g][f] = (f < d) ? x[int64_t(f) * a.ldx + a.off + pt] : T(0);
    } else {
#pragma unroll
      for (int e = 0; e < CB; ++e) xsb[g][e] = (e < ne) ? x[int64_t(e0 + e) * a.ldx + a.off + pt] * invl[e0 + e] : T(0);
    }
    T s2 = T(0);
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int f = 4 * q + kq;
      const T v = (f < d) ? x[int64_t(f) * a.ldx + a.off + pt] * invl[f] : T(0);
      xb[g][q] = v;
      s2 = fma(v, v, s2);
    }
    s2 += __shfl_xor(s2, 16);
    s2 += __shfl_xor(s2, 32);
    xn[g] = s2;
  }
  acc_t acc[PG], gacc[PG][CB];
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    acc[g] = acc_t{0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < CB; ++e) gacc[g][e] = acc_t{0, 0, 0, 0};
  }

  for (int64_t k0 = 0; k0 < Kp; k0 += KC) {
    const bool feat = k0 < a.Lp;   // a chunk holds features or inducing rows, never both
    __syncthreads();               // the previous chunk has been read
    for (int idx = tid; idx < DREG * KC; idx += 256) {
      const int f = idx / KC, kk = idx % KC;
      zc[f * ZLD + kk] = (f < d) ? rows[int64_t(f) * Kp + k0 + kk] : T(0);
    }
    for (int idx = tid; idx < KC * 16; idx += 256) {
      const int kk = idx / 16, j = idx % 16;
      pc[kk * PLD + j] = (a.s0 + j < a.Sp) ? panel[(k0 + kk) * a.Sp + a.s0 + j] : T(0);
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
      T zr[DIFF ? 4 : 1][DIFF ? DREG : 1];   // DIFF: every feature of the lane's four rows (the chunk holds z itself)
      if constexpr (DIFF) {
        if (!feat) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int f = 0; f < DREG; ++f) zr[r][f] = zc[f * ZLD + kr[r]];
        }
      }
#pragma unroll
      for (int g = 0; g < PG; ++g) {
        if (p0 + g * 16 >= len) break;   // wave-uniform
        acc_t t;
        T dfr[DIFF ? 4 : 1][DIFF ? DREG : 1];   // DIFF: (x_f - z_f) invl_f of the lane's four entries
        if (DIFF && !feat) {
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
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = feat ? tb[r] : tb[r] + xn[g];
#pragma unroll
          for (int q = 0; q < KS; ++q) t = Mfma16<T>::mma(za[q], xb[g][q], t);
        }
        acc_t tv, td;   // the value's tile and the gradient's: cos and -sin, or kappa and 2 g
        if (feat) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            tv[r] = val ? kcos(t[r]) : T(0);
            td[r] = -ksin(t[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const T r2 = t[r] < T(0) ? T(0) : t[r];
            tv[r] = kappa<T>(family, r2, variance);
            td[r] = kappa_2g<T>(family, r2, variance, tv[r]);
          }
        }
        if (val) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[g] = Mfma16<T>::mma(pa[r], tv[r], acc[g]);
        }
#pragma unroll
        for (int e = 0; e < CB; ++e) {
          if (e >= ne) break;   // wave-uniform
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T av = pa[r], bv = td[r];
            if (feat) {
              av *= zc[(e0 + e) * ZLD + kr[r]];   // omega_kc
            } else if constexpr (DIFF) {
              bv *= dfr[r][e < DREG ? e : 0];
            } else {
              bv *= fma(T(0.5), zc[(e0 + e) * ZLD + kr[r]], xsb[g][e]);   // xs_c - zs_kc from the row -2 zs_kc, rounded once
            }
            gacc[g][e] = Mfma16<T>::mma(av, bv, gacc[g][e]);
          }
        }
      }
    }
  }
  const T mc = T(a.mean_const);
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    const int64_t pt = p0 + g * 16 + c;
    if (pt >= len) continue;
    if (val) {
      const T mean = mux ? mc + mux[pt] : mc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t s = a.s0 + Mfma16<T>::row(lane, r);
        if (s < a.S) out[s * a.ldo + pt] = mean + acc[g][r];
      }
    }
#pragma unroll
    for (int e = 0; e < CB; ++e) {
      if (e >= ne) break;
      const T ile = invl[e0 + e];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t s = a.s0 + Mfma16<T>::row(lane, r);
        if (s < a.S) gout[(s * d + e0 + e) * ga.ldg + pt] = ile * gacc[g][e][r];
      }
    }
  }
}

template <typename T, int DREG>
void launch_grad_d(hipStream_t s, const SampleGradArgs& a0) {
  SampleGradArgs a = a0;
  const int64_t per = 4 * 16 * grad_point_groups<T, DREG>();   // points per workgroup
  const dim3 grid((unsigned)((a.v.len + per - 1) / per));
  for (int64_t s0 = 0; s0 < a.v.Sp; s0 += 16)          // one 16-column block of the panel
    for (int e0 = 0; e0 < a.v.d; e0 += grad_coord_block<T, DREG>()) {      // and one block of coordinates per launch
      a.v.s0 = s0;
      a.e0 = e0;
      hipLaunchKernelGGL((sample_grad_kernel<T, DREG>), grid, dim3(256), 0, s, a);
    }
}

template <typename T>
void launch_grad_t(hipStream_t s, const SampleGradArgs& a) {   // the DREG of launch_eval_t: the rows' layout follows it
  if (a.v.d <= 4) launch_grad_d<T, 4>(s, a);
  else if (a.v.d <= 8) launch_grad_d<T, 8>(s, a);
  else if (a.v.d <= 16) launch_grad_d<T, 16>(s, a);
  else if (a.v.d <= 32) launch_grad_d<T, 32>(s, a);
  else launch_grad_d<T, 64>(s, a);
}

}  // namespace

void launch_sample_grad(int dtype, hipStream_t s, const SampleGradArgs& a) {
  if (dtype == 0) launch_grad_t<double>(s, a); else launch_grad_t<float>(s, a);
}

}  // namespace svgp
