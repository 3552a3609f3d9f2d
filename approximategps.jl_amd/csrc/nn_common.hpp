// nn_common.hpp — what the translation units of the NearestNeighbors approximation share (nn.hip, nn_points.hip): the parameter block
// of a launch, the wave helpers and the squared distances of a block.  Device code only; every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ctx.hpp"
#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {

struct NnParams {
  int family, d, k;   // k: effective neighbour count min(k, N - 1)
  int64_t n, ldx;
  double variance, diag, mean_const;
  double invl[SVGP_MAX_D];
};

namespace {

constexpr int kNnNone = 0x7f7f7f7f;   // "no bad point": what hipMemsetAsync(0x7f) leaves in the first-bad-point word
constexpr int kNnGradSlots = 5;    // per point: log F, r^2 / F, (F <= 0), d / d variance, d / d diag; the d inverse lengthscales follow

// lane `l` (uniform) of v, through scalar registers
__device__ __forceinline__ float nn_rl(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double nn_rl(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double nn_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// f(integral_constant<I>) for I = I0 .. N - 1: the steps of the factorisation index the register array, so their number is a
// compile-time constant whatever the unroller's budget
template <int I, int N, typename Fn>
__device__ __forceinline__ void nn_static_for(Fn&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    nn_static_for<I + 1, N>(f);
  }
}

// d kappa / d r2 of the unit-variance kernel
template <typename T>
__device__ __forceinline__ T nn_dkappa(int family, T r2) {
  if (family == KSE) return T(-0.5) * kexp(T(-0.5) * r2);
  if (family == KM32) return T(-1.5) * kexp(-T(1.7320508075688772935) * ksqrt(r2));
  const T s = T(2.2360679774997896964) * ksqrt(r2);
  return -T(5.0 / 6.0) * (T(1) + s) * kexp(-s);
}

// A[q] = |s_q - s_j|^2 for the neighbours q, j = lane (s = x .* invl), cr2 = |s_i - s_j|^2; inactive lanes carry s = 0.
// The lane's neighbour is point base + lane (the window), or with G point `src` (a row of the neighbour table)
template <typename T, int KB, bool G = false>
__device__ __forceinline__ void nn_dist2(const NnParams& P, const T* __restrict__ x, int64_t base, int64_t i, int lane, int m, T (&A)[KB],
                                         T& cr2, int64_t src = 0) {
#pragma unroll
  for (int q = 0; q < KB; ++q) A[q] = T(0);
  cr2 = T(0);
  for (int f = 0; f < P.d; ++f) {
    const T il = T(P.invl[f]);
    const T xj = lane < m ? x[int64_t(f) * P.ldx + (G ? src : base + lane)] * il : T(0);
    const T dc = xj - x[int64_t(f) * P.ldx + i] * il;
    cr2 = fma(dc, dc, cr2);
#pragma unroll
    for (int g = 0; g < KB / 8; ++g)
      if (g * 8 < m) {
#pragma unroll
        for (int q = g * 8; q < g * 8 + 8; ++q) {
          const T df = nn_rl(xj, q) - xj;
          A[q] = fma(df, df, A[q]);
        }
      }
  }
}

// nn_dist2 with the lane's neighbour point `src` of x and the query column i of xq (ld ldq)
template <typename T, int KB>
__device__ __forceinline__ void nn_dist2_query(const NnParams& P, const T* __restrict__ x, const T* __restrict__ xq, int64_t ldq, int64_t i,
                                               int lane, int m, T (&A)[KB], T& cr2, int64_t src) {
#pragma unroll
  for (int q = 0; q < KB; ++q) A[q] = T(0);
  cr2 = T(0);
  for (int f = 0; f < P.d; ++f) {
    const T il = T(P.invl[f]);
    const T xj = lane < m ? x[int64_t(f) * P.ldx + src] * il : T(0);
    const T dc = xj - xq[int64_t(f) * ldq + i] * il;
    cr2 = fma(dc, dc, cr2);
#pragma unroll
    for (int g = 0; g < KB / 8; ++g)
      if (g * 8 < m) {
#pragma unroll
        for (int q = g * 8; q < g * 8 + 8; ++q) {
          const T df = nn_rl(xj, q) - xj;
          A[q] = fma(df, df, A[q]);
        }
      }
  }
}

// The right-looking factorisation of the block with c and dd = delta_ns riding along: F -= l'l, r -= l'z (fp64), lane p keeps
// 1 / L[p][p], l_p, z_p.  -> a pivot was "not positive": at or below floor_
template <typename T, int KB>
__device__ __forceinline__ bool nn_factor(int lane, int m, double floor_, T (&A)[KB], T& c, T& dd, double& F, double& r, T& myrs, T& lme,
                                          T& zme) {
  bool isbad = false;
  nn_static_for<0, KB>([&](auto pc) __attribute__((always_inline)) {
    constexpr int p = decltype(pc)::value;
    if (p < m) {
      const T piv = nn_rl(A[p], p);
      if (!(double(piv) > floor_)) isbad = true;
      const T rs = T(1) / ksqrt(piv);
      const T lj = A[p] * rs;                     // L[j][p] for the lanes j >= p
      const T ljm = lane > p ? lj : T(0);
      A[p] = lane >= p ? lj : A[p];               // lanes j < p: column j of the Schur complement stays (scaled in the back-substitution)
      const T lm = nn_rl(c, p) * rs, zp = nn_rl(dd, p) * rs;
      F = fma(-double(lm), double(lm), F);
      r = fma(-double(lm), double(zp), r);
      if (lane == p) { myrs = rs; lme = lm; zme = zp; }
      c = fma(-lm, ljm, c);
      dd = fma(-zp, ljm, dd);
#pragma unroll
      for (int g = (p + 1) / 8; g < KB / 8; ++g)
        if (g * 8 < m) {
#pragma unroll
          for (int q = (g * 8 > p + 1 ? g * 8 : p + 1); q < g * 8 + 8; ++q) A[q] = fma(-nn_rl(lj, q), ljm, A[q]);
        }
    }
  });
  return isbad;
}

}  // namespace
}  // namespace svgp
