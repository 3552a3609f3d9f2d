// cg.hip — the exact GP by matrix-free conjugate gradients (svgp_cg_*: cg_api.hip holds the host side).
//   out[i, s] = sum_j prof(r^2(P_i, R_j)) V[j, s]  (+ diag addv[i, s]),     prof = kappa, or 2 g (xs_ic - xs_jc)^2 of one coordinate c
// kmv_kernel is sample_eval_kernel (sample.hip) with the inducing rows replaced by the N data rows R and the resident panel by an
// N x S one read from global memory chunk by chunk: every 16 x 16 tile (16 rows j, 16 points i) is generated TRANSPOSED on the MFMA in
// the expansion form r^2 = |xs_j|^2 + |xs_i|^2 - 2 xs_j . xs_i, kappa<T> is applied in registers, and the C/D registers are the B
// operand of the second product out'[s][i] += V'[s][j] tile[j][i].  No entry of K is ever stored.  Every sum has a fixed order (j
// ascending in steps of 4 inside one accumulator chain), no atomics; an output column depends on its own panel column alone, so a
// column's value does not depend on which other columns share the launch.
// The vector stage of the solver (masked axpys, column dots) is a handful of streaming kernels; every dot is a fixed two-stage
// reduction in fp64 for both dtypes, and the per-column CG scalars live in a small fp64 state block on the device.
// The Nystrom preconditioner (svgp_cg_set_preconditioner) adds kmv_split_kernel, the row-split sibling of kmv_kernel for K(z_p, X) V with
// few points and a long reduction, and the small fp64 kernels of its k-sized stage; the other direction K(X, z_p) c is kmv_kernel itself.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {

namespace {

constexpr int kKmvKC = 32;   // rows per LDS chunk (Np is a multiple of it)

// groups of 16 points a wave owns: sample_point_groups' rule (two waves per SIMD: <= 256 VGPRs + AGPRs); the lengthscale profile
// carries the coordinate's registers as well, and its f64 form with 32 features and four column blocks measured 262 - 268 with two groups
template <typename T, int DREG, int NSB, int PROFILE>
constexpr int kmv_point_groups() {
  return (sizeof(T) == 8 && NSB > 1 && (DREG > 32 || (DREG > 16 && PROFILE != 0))) ? 1 : (DREG > 16 || NSB > 1) ? 2 : 4;
}

// One workgroup = 4 waves; a wave owns PG groups of 16 points and, per launch, NSB 16-column blocks of the panel (<= 64 columns).
// PROFILE 0: kappa.  PROFILE 1: 2 g(r^2) (xs_ic - xs_jc)^2 for the coordinate a.coord, the difference taken per ENTRY before the
// product (sample_grad.hip's design: the expanded square cancels like |xs|^2 against the difference).
template <typename T, int DREG, int NSB, int PROFILE>
__global__ void __launch_bounds__(256) kmv_kernel(KmvArgs a) {
  constexpr int KS = DREG / 4, KC = kKmvKC, NW = 4;
  constexpr int PG = kmv_point_groups<T, DREG, NSB, PROFILE>();
  constexpr int ZLD = KC + 16, PLD = NSB * 16 + 4;
  // fp32, d <= 8: r^2 by differences of the UNSCALED coordinates on the VALU, scaled afterwards (sample.hip explains why: the
  // expansion loses eps32 (|xs_i|^2 + |xs_j|^2) absolutely, and here |xs| grows with the domain while r^2 of the entries that
  // matter stays of order one).  The rows of such a handle hold x itself (kmv_prep_kernel, raw).
  constexpr bool DIFF = sizeof(T) == 4 && DREG <= 8;
  using acc_t = typename Mfma16<T>::acc_t;
  __shared__ T zc[DREG * ZLD];   // [f][kk]  rows of the chunk (MFMA A operand of the generation)
  __shared__ T pc[KC * PLD];     // [kk][j]  panel rows of the chunk, the launch's column block
  __shared__ T tc[KC];           // [kk]     bias |xs_j|^2
  const T* __restrict__ rows = static_cast<const T*>(a.rows);
  const T* __restrict__ bias = static_cast<const T*>(a.bias);
  const T* __restrict__ V = static_cast<const T*>(a.V);
  const T* __restrict__ invl = static_cast<const T*>(a.invl);
  const T* __restrict__ x = static_cast<const T*>(a.px);
  const T* __restrict__ addv = static_cast<const T*>(a.addv);
  T* __restrict__ out = static_cast<T*>(a.out);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
  const int d = a.d, family = a.family, coord = a.coord;
  const int64_t n = a.n, N = a.N, Np = a.Np;
  const T variance = T(a.variance);
  const int64_t p0 = (int64_t(blockIdx.x) * NW + wave) * (PG * 16);
  T xb[PG][KS], xn[PG];
  T xall[DIFF ? PG : 1][DIFF ? DREG : 1];   // DIFF: every feature of point c, unscaled
  T il[DIFF ? DREG : 1];
  T xc[PROFILE ? PG : 1];                   // PROFILE 1: coordinate `coord` of point c (DIFF: unscaled, otherwise scaled)
  const T ilc = PROFILE ? invl[coord] : T(0);
  if constexpr (DIFF) {
#pragma unroll
    for (int f = 0; f < DREG; ++f) il[f] = (f < d) ? invl[f] : T(0);
  }
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    int64_t pt = p0 + g * 16 + c;
    pt = pt < n ? pt : n - 1;
    if constexpr (DIFF) {
#pragma unroll
      for (int f = 0; f < DREG; ++f) xall[g][f] = (f < d) ? x[int64_t(f) * a.ldp + pt] : T(0);
    }
    if constexpr (PROFILE != 0) {
      const T v = x[int64_t(coord) * a.ldp + pt];
      xc[g] = DIFF ? v : v * ilc;
    }
    T s2 = T(0);
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int f = 4 * q + kq;
      const T v = (f < d) ? x[int64_t(f) * a.ldp + pt] * invl[f] : T(0);
      xb[g][q] = v;
      s2 = fma(v, v, s2);
    }
    s2 += __shfl_xor(s2, 16);
    s2 += __shfl_xor(s2, 32);
    xn[g] = s2;
  }
  acc_t acc[PG][NSB];
#pragma unroll
  for (int g = 0; g < PG; ++g)
#pragma unroll
    for (int b = 0; b < NSB; ++b) acc[g][b] = acc_t{0, 0, 0, 0};

  for (int64_t k0 = 0; k0 < Np; k0 += KC) {
    __syncthreads();   // the previous chunk has been read
    for (int idx = tid; idx < DREG * KC; idx += 256) {
      const int f = idx / KC, kk = idx % KC;
      zc[f * ZLD + kk] = (f < d) ? rows[int64_t(f) * Np + k0 + kk] : T(0);
    }
    for (int idx = tid; idx < KC * NSB * 16; idx += 256) {   // the panel is column-major: kk runs fastest over the threads
      const int j = idx / KC, kk = idx % KC;
      pc[kk * PLD + j] = (a.s0 + j < a.S && k0 + kk < N) ? V[(a.s0 + j) * a.ldv + k0 + kk] : T(0);
    }
    if (tid < KC) tc[tid] = bias[k0 + tid];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < KC / 16; ++h) {
      T za[KS], pa[4][NSB], tb[4];
#pragma unroll
      for (int q = 0; q < KS; ++q) za[q] = zc[(4 * q + kq) * ZLD + h * 16 + c];
      T zrc[PROFILE ? 4 : 1];   // PROFILE 1: coordinate `coord` of the lane's four rows, as the chunk holds it
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = h * 16 + Mfma16<T>::row(lane, r);   // the row this lane's register r holds after the generation
        tb[r] = tc[kk];
        if constexpr (PROFILE != 0) zrc[r] = zc[coord * ZLD + kk];
#pragma unroll
        for (int b = 0; b < NSB; ++b) pa[r][b] = pc[kk * PLD + b * 16 + c];
      }
      T zr[DIFF ? 4 : 1][DIFF ? DREG : 1];   // DIFF: every feature of the lane's four rows (the chunk holds x itself)
      if constexpr (DIFF) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int f = 0; f < DREG; ++f) zr[r][f] = zc[f * ZLD + h * 16 + Mfma16<T>::row(lane, r)];
      }
#pragma unroll
      for (int g = 0; g < PG; ++g) {
        if (p0 + g * 16 >= n) break;   // wave-uniform
        acc_t t;
        if constexpr (DIFF) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T s2 = T(0);
#pragma unroll
            for (int f = 0; f < DREG; ++f) {
              const T df = (xall[g][f] - zr[r][f]) * il[f];
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
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          T r2 = t[r] < T(0) ? T(0) : t[r];
          // P = R: the diagonal of K is exactly the variance (the expansion leaves eps (|xs_i|^2 + |xs_j|^2) there, which the square root
          // of the Matern families turns into sqrt(eps) |xs|)
          if (a.self && k0 + h * 16 + Mfma16<T>::row(lane, r) == p0 + g * 16 + c) r2 = T(0);
          const T kv = kappa<T>(family, r2, variance);
          if constexpr (PROFILE == 0) {
            t[r] = kv;
          } else {
            // scaled difference of the coordinate: the rows hold x_jc (DIFF) or -2 xs_jc
            const T dc = DIFF ? (xc[g] - zrc[r]) * ilc : fma(T(0.5), zrc[r], xc[g]);
            t[r] = kappa_2g<T>(family, r2, variance, kv) * (dc * dc);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int b = 0; b < NSB; ++b) acc[g][b] = Mfma16<T>::mma(pa[r][b], t[r], acc[g][b]);
      }
    }
  }
  const T dg = T(a.diag);
  const T* __restrict__ dvec = addv ? static_cast<const T*>(a.dvec) : nullptr;   // per-point noise: the factor of addv, per output point
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    const int64_t pt = p0 + g * 16 + c;
    if (pt >= n) continue;
    const T dgp = dvec ? dvec[pt] : dg;   // once per point group, after the row loop: no register lives across it
#pragma unroll
    for (int b = 0; b < NSB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t s = a.s0 + b * 16 + Mfma16<T>::row(lane, r);
        if (s >= a.S) continue;
        T v = acc[g][b][r];
        if (addv) v = fma(dgp, addv[s * a.lda + pt], v);
        out[s * a.ldo + pt] = v;
      }
  }
}

// The row-split form of kmv_kernel (PROFILE 0) for FEW points and a LONG reduction: K(z_p, X) V of the Nystrom preconditioner, k points
// against the N data rows.  kmv_kernel would put 64 PG points on a workgroup and walk all of Np: a handful of workgroups.  Here the
// grid is (point workgroups) x (row segments); workgroup (bx, seg) walks the whole chunks [seg seg_rows, (seg + 1) seg_rows) of the rows
// with kmv_kernel's tile generation, DIFF path and accumulator chain, and writes its partial sums part[seg][column slot][point] in the
// data dtype; kmv_segsum_kernel adds the segments in ascending order in fp64.  No atomics; the split is a function of N and the number
// of points alone (kmv_split_segments), so a column's value does not depend on its neighbours and repeated calls are bitwise equal.
template <typename T, int DREG, int NSB>
__global__ void __launch_bounds__(256) kmv_split_kernel(KmvArgs a, T* __restrict__ part, int64_t seg_rows) {
  constexpr int KS = DREG / 4, KC = kKmvKC, NW = 4;
  constexpr int PG = kmv_point_groups<T, DREG, NSB, 0>();
  constexpr int ZLD = KC + 16, PLD = NSB * 16 + 4;
  constexpr bool DIFF = sizeof(T) == 4 && DREG <= 8;
  using acc_t = typename Mfma16<T>::acc_t;
  __shared__ T zc[DREG * ZLD];
  __shared__ T pc[KC * PLD];
  __shared__ T tc[KC];
  const T* __restrict__ rows = static_cast<const T*>(a.rows);
  const T* __restrict__ bias = static_cast<const T*>(a.bias);
  const T* __restrict__ V = static_cast<const T*>(a.V);
  const T* __restrict__ invl = static_cast<const T*>(a.invl);
  const T* __restrict__ x = static_cast<const T*>(a.px);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
  const int d = a.d, family = a.family;
  const int64_t n = a.n, N = a.N, Np = a.Np;
  const T variance = T(a.variance);
  const int64_t p0 = (int64_t(blockIdx.x) * NW + wave) * (PG * 16);
  const int64_t kbeg = int64_t(blockIdx.y) * seg_rows;
  const int64_t kend = kbeg + seg_rows < Np ? kbeg + seg_rows : Np;
  T xb[PG][KS], xn[PG];
  T xall[DIFF ? PG : 1][DIFF ? DREG : 1];
  T il[DIFF ? DREG : 1];
  if constexpr (DIFF) {
#pragma unroll
    for (int f = 0; f < DREG; ++f) il[f] = (f < d) ? invl[f] : T(0);
  }
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    int64_t pt = p0 + g * 16 + c;
    pt = pt < n ? pt : n - 1;
    if constexpr (DIFF) {
#pragma unroll
      for (int f = 0; f < DREG; ++f) xall[g][f] = (f < d) ? x[int64_t(f) * a.ldp + pt] : T(0);
    }
    T s2 = T(0);
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int f = 4 * q + kq;
      const T v = (f < d) ? x[int64_t(f) * a.ldp + pt] * invl[f] : T(0);
      xb[g][q] = v;
      s2 = fma(v, v, s2);
    }
    s2 += __shfl_xor(s2, 16);
    s2 += __shfl_xor(s2, 32);
    xn[g] = s2;
  }
  acc_t acc[PG][NSB];
#pragma unroll
  for (int g = 0; g < PG; ++g)
#pragma unroll
    for (int b = 0; b < NSB; ++b) acc[g][b] = acc_t{0, 0, 0, 0};

  for (int64_t k0 = kbeg; k0 < kend; k0 += KC) {
    __syncthreads();   // the previous chunk has been read
    for (int idx = tid; idx < DREG * KC; idx += 256) {
      const int f = idx / KC, kk = idx % KC;
      zc[f * ZLD + kk] = (f < d) ? rows[int64_t(f) * Np + k0 + kk] : T(0);
    }
    for (int idx = tid; idx < KC * NSB * 16; idx += 256) {
      const int j = idx / KC, kk = idx % KC;
      pc[kk * PLD + j] = (a.s0 + j < a.S && k0 + kk < N) ? V[(a.s0 + j) * a.ldv + k0 + kk] : T(0);
    }
    if (tid < KC) tc[tid] = bias[k0 + tid];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < KC / 16; ++h) {
      T za[KS], pa[4][NSB], tb[4];
#pragma unroll
      for (int q = 0; q < KS; ++q) za[q] = zc[(4 * q + kq) * ZLD + h * 16 + c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = h * 16 + Mfma16<T>::row(lane, r);
        tb[r] = tc[kk];
#pragma unroll
        for (int b = 0; b < NSB; ++b) pa[r][b] = pc[kk * PLD + b * 16 + c];
      }
      T zr[DIFF ? 4 : 1][DIFF ? DREG : 1];
      if constexpr (DIFF) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int f = 0; f < DREG; ++f) zr[r][f] = zc[f * ZLD + h * 16 + Mfma16<T>::row(lane, r)];
      }
#pragma unroll
      for (int g = 0; g < PG; ++g) {
        if (p0 + g * 16 >= n) break;   // wave-uniform
        acc_t t;
        if constexpr (DIFF) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T s2 = T(0);
#pragma unroll
            for (int f = 0; f < DREG; ++f) {
              const T df = (xall[g][f] - zr[r][f]) * il[f];
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
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = kappa<T>(family, t[r] < T(0) ? T(0) : t[r], variance);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int b = 0; b < NSB; ++b) acc[g][b] = Mfma16<T>::mma(pa[r][b], t[r], acc[g][b]);
      }
    }
  }
  T* __restrict__ o = part + int64_t(blockIdx.y) * 64 * n;   // [segment][64 column slots][n]
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    const int64_t pt = p0 + g * 16 + c;
    if (pt >= n) continue;
#pragma unroll
    for (int b = 0; b < NSB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int sl = b * 16 + Mfma16<T>::row(lane, r);
        if (a.s0 + sl >= a.S) continue;
        o[int64_t(sl) * n + pt] = acc[g][b][r];
      }
  }
}

// out[(s0 + sl) ldo + pt] = sum over the segments, ascending, of part[seg][sl][pt], in fp64
template <typename T>
__global__ void kmv_segsum_kernel(const T* __restrict__ part, int nseg, int64_t n, int64_t s0, T* __restrict__ out, int64_t ldo) {
  const int64_t pt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, sl = blockIdx.y;
  if (pt >= n) return;
  double s = 0.0;
  for (int g = 0; g < nseg; ++g) s += double(part[(int64_t(g) * 64 + sl) * n + pt]);
  out[(s0 + sl) * ldo + pt] = T(s);
}

template <typename T, int DREG>
void launch_kmv_split_d(hipStream_t s, const KmvArgs& a0, void* part) {
  KmvArgs a = a0;
  int64_t seg_rows = 0;
  const int nseg = kmv_split_segments(a.N, a.n, &seg_rows);
  for (int64_t s0 = 0; s0 < a.S; s0 += 64) {   // column blocks of at most 64, as launch_kmv_d
    a.s0 = s0;
    const int64_t nc = a.S - s0 < 64 ? a.S - s0 : 64;
    const bool one = nc <= 16;
    const int64_t per = 4 * 16 * (one ? kmv_point_groups<T, DREG, 1, 0>() : kmv_point_groups<T, DREG, 4, 0>());
    const dim3 grid((unsigned)((a.n + per - 1) / per), (unsigned)nseg);
    if (one) hipLaunchKernelGGL((kmv_split_kernel<T, DREG, 1>), grid, dim3(256), 0, s, a, (T*)part, seg_rows);
    else hipLaunchKernelGGL((kmv_split_kernel<T, DREG, 4>), grid, dim3(256), 0, s, a, (T*)part, seg_rows);
    hipLaunchKernelGGL(kmv_segsum_kernel<T>, dim3((unsigned)((a.n + 255) / 256), (unsigned)nc), dim3(256), 0, s, (const T*)part, nseg, a.n, s0,
                       (T*)a.out, a.ldo);
  }
}

template <typename T>
void launch_kmv_split_t(hipStream_t s, const KmvArgs& a, void* part) {
  if (a.d <= 4) launch_kmv_split_d<T, 4>(s, a, part);
  else if (a.d <= 8) launch_kmv_split_d<T, 8>(s, a, part);
  else if (a.d <= 16) launch_kmv_split_d<T, 16>(s, a, part);
  else if (a.d <= 32) launch_kmv_split_d<T, 32>(s, a, part);
  else launch_kmv_split_d<T, 64>(s, a, part);
}

template <typename T, int DREG, int PROFILE>
void launch_kmv_d(hipStream_t s, const KmvArgs& a0) {
  KmvArgs a = a0;
  for (int64_t s0 = 0; s0 < a.S; s0 += 64) {   // column blocks of at most 64, one launch each
    a.s0 = s0;
    const bool one = a.S - s0 <= 16;
    const int64_t per = 4 * 16 * (one ? kmv_point_groups<T, DREG, 1, PROFILE>() : kmv_point_groups<T, DREG, 4, PROFILE>());   // points per workgroup
    const dim3 grid((unsigned)((a.n + per - 1) / per));
    if (one) hipLaunchKernelGGL((kmv_kernel<T, DREG, 1, PROFILE>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((kmv_kernel<T, DREG, 4, PROFILE>), grid, dim3(256), 0, s, a);
  }
}

template <typename T, int PROFILE>
void launch_kmv_p(hipStream_t s, const KmvArgs& a) {
  if (a.d <= 4) launch_kmv_d<T, 4, PROFILE>(s, a);
  else if (a.d <= 8) launch_kmv_d<T, 8, PROFILE>(s, a);
  else if (a.d <= 16) launch_kmv_d<T, 16, PROFILE>(s, a);
  else if (a.d <= 32) launch_kmv_d<T, 32, PROFILE>(s, a);
  else launch_kmv_d<T, 64, PROFILE>(s, a);
}

// rows[f][j] = -2 xs_jf (raw: x_jf itself), bias[j] = |xs_j|^2 from the ROUNDED xs = x invl, the product kmv_kernel forms for its points;
// zero on the padding j >= N, whose panel rows kmv_kernel reads as zero
template <typename T>
__global__ void kmv_prep_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ invl, int d, int64_t N, int64_t Np, int raw,
                                T* __restrict__ rows, T* __restrict__ bias) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= Np) return;
  T s = T(0);
  for (int f = 0; f < d; ++f) {
    const T v = (j < N) ? x[int64_t(f) * ldx + j] : T(0);
    const T xs = v * invl[f];
    rows[int64_t(f) * Np + j] = raw ? v : T(-2) * xs;
    s = fma(xs, xs, s);
  }
  bias[j] = s;
}

// ---- the vector stage --------------------------------------------------------------------------------------------------------------

// partial[col * nblk + blk] = sum over the rows of block blk of a[i, col] b[i, col], fp64: a thread sums its rows i = r0 + tid + 256 t
// ascending, then a fixed tree over the 256 threads.  The split depends on N alone
template <typename T>
__global__ void __launch_bounds__(256) cg_dot_kernel(const T* __restrict__ a, int64_t lda, const T* __restrict__ b, int64_t ldb, int64_t N,
                                                     int64_t rows_per_blk, double* __restrict__ partial) {
  __shared__ double sm[256];
  const int64_t col = blockIdx.y, r0 = int64_t(blockIdx.x) * rows_per_blk;
  const int64_t r1 = r0 + rows_per_blk < N ? r0 + rows_per_blk : N;
  double s = 0.0;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) s = fma(double(a[col * lda + i]), double(b[col * ldb + i]), s);
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[col * gridDim.x + blockIdx.x] = sm[0];
}

// out[col] = sum_blk partial[col * nblk + blk], blk ascending
__global__ void cg_colsum_kernel(const double* __restrict__ partial, int nblk, int64_t ncols, double* __restrict__ out) {
  const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (col >= ncols) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[col * nblk + b];
  out[col] = s;
}

// the per-column scalars of one column block (<= 64 columns), st = kCgStateDoubles fp64 words (kernels.hpp: CgState)
//   mode 0 (partial = b'b):  bb = rr = b'b, active = bb > 0, iterations = 0; a NaN norm marks the block bad
//   mode 1 (partial = p'q):  active columns: a = rr / p'q, recorded in hist_a[k]; a curvature that is not > 0 marks the block bad
//   mode 2 (partial = r'r):  active columns: beta = r'r / rr recorded in hist_b[k], rr = r'r, iterations = k + 1, and the column stops
//                            once r'r <= tol^2 b'b
// The preconditioned recurrence (rho non-null: [0, 64) rho = r'z of the running iteration, [64, 128) its initial value z_0' P^-1 z_0):
//   mode 3 (partial = r'z, after mode 0):  rho = rho_0 = r'z; an active column whose r'z is not > 0 marks the block bad
//   mode 1:                                a = rho / p'q
//   mode 4 (partial = r'r):  mode 2 without beta: rr, iterations, the stopping test on the TRUE residual; hist_b[k] = 0
//   mode 5 (partial = r'z, z = P^-1 r):    columns still active: beta = r'z / rho recorded in hist_b[k], rho = r'z; r'z that is not > 0
//                            marks the block bad
__global__ void cg_coef_kernel(int mode, double* __restrict__ st, const double* __restrict__ partial, int nblk, int ncols, int k, double tol2,
                               double* __restrict__ hist_a, double* __restrict__ hist_b, double* __restrict__ rho) {
  const int s = threadIdx.x;
  if (s >= 64) return;
  if (s >= ncols) {
    if (mode == 0) {
      st[CgState::BB + s] = 0.0; st[CgState::RR + s] = 0.0; st[CgState::A + s] = 0.0; st[CgState::BE + s] = 0.0;
      st[CgState::ACT + s] = 0.0; st[CgState::IT + s] = 0.0;
    }
    return;
  }
  double v = 0.0;
  for (int b = 0; b < nblk; ++b) v += partial[s * nblk + b];
  if (mode == 0) {
    st[CgState::BB + s] = v;
    st[CgState::RR + s] = v;
    st[CgState::A + s] = 0.0;
    st[CgState::BE + s] = 0.0;
    st[CgState::ACT + s] = v > 0.0 ? 1.0 : 0.0;
    st[CgState::IT + s] = 0.0;
    if (s == 0) st[CgState::BAD] = 0.0;
    __syncthreads();
    if (!(v == v)) st[CgState::BAD] = 1.0;   // (every writer stores the same word)
    return;
  }
  if (mode == 3) {
    rho[s] = v;
    rho[64 + s] = v;
    // r' P^-1 r of a nonzero r that is not > 0 (NaN included): the applied P^-1 has lost positive definiteness
    if (st[CgState::ACT + s] != 0.0 && !(v > 0.0)) st[CgState::BAD] = 1.0;
    return;
  }
  const bool act = st[CgState::ACT + s] != 0.0;
  if (mode == 1) {
    double al = 0.0;
    if (act) {
      if (v > 0.0) {
        al = (rho ? rho[s] : st[CgState::RR + s]) / v;
      } else {
        st[CgState::BAD] = 1.0;
        st[CgState::ACT + s] = 0.0;
      }
      if (hist_a) hist_a[int64_t(k) * 64 + s] = al;
    }
    st[CgState::A + s] = al;
    return;
  }
  if (mode == 4) {
    if (act) {
      if (hist_b) hist_b[int64_t(k) * 64 + s] = 0.0;
      st[CgState::RR + s] = v;
      st[CgState::IT + s] = double(k + 1);
      if (v <= tol2 * st[CgState::BB + s]) st[CgState::ACT + s] = 0.0;
    }
    st[CgState::BE + s] = 0.0;
    return;
  }
  if (mode == 5) {
    double be = 0.0;
    if (act) {
      if (v > 0.0) {
        be = v / rho[s];
      } else {   // as a curvature that is not > 0 in mode 1
        st[CgState::BAD] = 1.0;
        st[CgState::ACT + s] = 0.0;
      }
      if (hist_b) hist_b[int64_t(k) * 64 + s] = be;
      rho[s] = v;
    }
    st[CgState::BE + s] = be;
    return;
  }
  double be = 0.0;
  if (act) {
    const double rr = st[CgState::RR + s];
    be = v / rr;
    if (hist_b) hist_b[int64_t(k) * 64 + s] = be;
    st[CgState::RR + s] = v;
    st[CgState::IT + s] = double(k + 1);
    if (v <= tol2 * st[CgState::BB + s]) st[CgState::ACT + s] = 0.0;
  }
  st[CgState::BE + s] = be;
}

// active columns: x += a p, r -= a q
template <typename T>
__global__ void cg_update_xr_kernel(const double* __restrict__ st, int64_t N, T* __restrict__ x, T* __restrict__ r, const T* __restrict__ p,
                                    const T* __restrict__ q) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, col = blockIdx.y;
  if (i >= N || st[CgState::ACT + col] == 0.0) return;
  const T al = T(st[CgState::A + col]);
  const int64_t o = col * N + i;
  x[o] = fma(al, p[o], x[o]);
  r[o] = fma(-al, q[o], r[o]);
}

// columns still active after the residual check: p = r + beta p
template <typename T>
__global__ void cg_update_p_kernel(const double* __restrict__ st, int64_t N, const T* __restrict__ r, T* __restrict__ p) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, col = blockIdx.y;
  if (i >= N || st[CgState::ACT + col] == 0.0) return;
  const T be = T(st[CgState::BE + col]);
  const int64_t o = col * N + i;
  p[o] = fma(be, p[o], r[o]);
}

// dst[i, col] = T(alpha src[i, col] + beta)   (src fp64 or T)
template <typename T, typename U>
__global__ void cg_affine_kernel(const U* __restrict__ src, int64_t lds, int64_t N, double alpha, double beta, T* __restrict__ dst, int64_t ldd) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, col = blockIdx.y;
  if (i >= N) return;
  dst[col * ldd + i] = T(alpha * double(src[col * lds + i]) + beta);
}

// out[i, j] = kappa(r^2(x_i, xt_j)), r^2 by differences of the scaled coordinates: the right-hand sides k(X, x*) of the predictive variance
template <typename T>
__global__ void cg_kcols_kernel(const T* __restrict__ x, int64_t ldx, int64_t N, const T* __restrict__ xt, int64_t ldt, const T* __restrict__ invl,
                                int d, int family, double variance, T* __restrict__ out, int64_t ldo) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i >= N) return;
  T s2 = T(0);
  for (int f = 0; f < d; ++f) {
    const T df = (x[int64_t(f) * ldx + i] - xt[int64_t(f) * ldt + j]) * invl[f];
    s2 = fma(df, df, s2);
  }
  out[j * ldo + i] = kappa<T>(family, s2, T(variance));
}

// ---- the k-sized stage of the Nystrom preconditioner (fp64 for both data dtypes) ---------------------------------------------------

// dst[j ldd + i] = double(src[j lds + i])
template <typename T>
__global__ void cg_widen_kernel(const T* __restrict__ src, int64_t lds, int64_t n, double* __restrict__ dst, int64_t ldd) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < n) dst[j * ldd + i] = double(src[j * lds + i]);
}

// zs[f][i] = z[f][i] invl[f] for i < k, 0 for k <= i < Mp: launch_kuu's operand
__global__ void cg_pc_scale_kernel(const double* __restrict__ z, int64_t ldz, const double* __restrict__ invl, int64_t k, int64_t Mp,
                                   double* __restrict__ zs) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, f = blockIdx.y;
  if (i < Mp) zs[f * Mp + i] = i < k ? z[f * ldz + i] * invl[f] : 0.0;
}

// Bm = I + (A + A') / (2 sigma^2), full
__global__ void cg_pc_form_b_kernel(const double* __restrict__ A, int64_t Mp, double inv_s2, double* __restrict__ Bm) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < Mp) Bm[j * Mp + i] = (i == j ? 1.0 : 0.0) + 0.5 * inv_s2 * (A[j * Mp + i] + A[i * Mp + j]);
}

// out[0] = 2 sum_{i < k} log L_ii, i ascending
__global__ void cg_pc_logdet_kernel(const double* __restrict__ L, int64_t Mp, int64_t k, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = 0.0;
  for (int64_t i = 0; i < k; ++i) s += log(L[i * Mp + i]);
  out[0] = 2.0 * s;
}

// out[s ldo + i] = alpha sum_{j < k} Mt[j Mp + i] v[s ldv + j] for i < k (j ascending, fp64), 0 for k <= i < rows_out: the product M' v
// with a k x k matrix held in an Mp x Mp array (W is symmetric; Lu^-1 row-major gives Lu^-T v)
template <typename TI, typename TO>
__global__ void cg_pc_mm_kernel(const double* __restrict__ Mt, int64_t Mp, int64_t k, const TI* __restrict__ v, int64_t ldv, double alpha,
                                TO* __restrict__ out, int64_t ldo, int64_t rows_out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (i >= rows_out) return;
  double acc = 0.0;
  if (i < k)
    for (int64_t j = 0; j < k; ++j) acc = fma(Mt[j * Mp + i], double(v[s * ldv + j]), acc);
  out[s * ldo + i] = TO(alpha * acc);
}

// ---- per-point noise variances (svgp_cg_set_noise) -----------------------------------------------------------------------------------

// out[0] = min_i s[i] in fp64, NaN once any s[i] is NaN: one workgroup, a thread takes i = tid + 256 t ascending, then a fixed tree
template <typename T>
__global__ void __launch_bounds__(256) cg_noise_min_kernel(const T* __restrict__ sv, int64_t N, double* __restrict__ out) {
  __shared__ double sm[256];
  auto nmin = [](double a, double b) { return (a != a) ? a : (b != b) ? b : (b < a ? b : a); };
  double m = INFINITY;
  for (int64_t i = threadIdx.x; i < N; i += 256) m = nmin(m, double(sv[i]));
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) sm[threadIdx.x] = nmin(sm[threadIdx.x], sm[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sm[0];
}

// sig2 = T(diag) + s (one rounding in T), and what the preconditioner, its probes and the Gram read of it
template <typename T>
__global__ void cg_noise_prep_kernel(const T* __restrict__ sv, int64_t N, T dg, T* __restrict__ sig2, T* __restrict__ isig2, T* __restrict__ ssig2,
                                     double* __restrict__ isig64) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const T v = dg + sv[i];
  const double v64 = double(v);
  sig2[i] = v;
  isig2[i] = T(1.0 / v64);
  ssig2[i] = T(sqrt(v64));
  isig64[i] = 1.0 / v64;
}

// dst[i, col] = src[i, col] vec[i]
template <typename T>
__global__ void cg_rowscale_kernel(const T* __restrict__ src, int64_t lds, const T* __restrict__ vec, int64_t N, T* __restrict__ dst, int64_t ldd) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, col = blockIdx.y;
  if (i >= N) return;
  dst[col * ldd + i] = src[col * lds + i] * vec[i];
}

// d lml / d sigma_i^2 from the panels U = [alpha, w_t] and P = [alpha, p_t]: t ascending in fp64, rounded once
template <typename T>
__global__ void cg_sbar_kernel(const T* __restrict__ U, const T* __restrict__ P, int64_t N, int Tn, T* __restrict__ sbar) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (Tn < 1) {
    sbar[i] = T(NAN);
    return;
  }
  double tr = 0.0;
  for (int t = 1; t <= Tn; ++t) tr = fma(double(U[int64_t(t) * N + i]), double(P[int64_t(t) * N + i]), tr);
  sbar[i] = T(0.5 * (double(U[i]) * double(P[i])) - tr / (2.0 * double(Tn)));
}

// cg_dot_kernel's first stage for sum_i log sig2[i] (b NULL) or sum_i sig2[i] b[i]
template <typename T>
__global__ void __launch_bounds__(256) cg_noise_sum_kernel(const T* __restrict__ sig2, const T* __restrict__ b, int64_t N, int64_t rows_per_blk,
                                                           double* __restrict__ partial) {
  __shared__ double sm[256];
  const int64_t r0 = int64_t(blockIdx.x) * rows_per_blk;
  const int64_t r1 = r0 + rows_per_blk < N ? r0 + rows_per_blk : N;
  double s = 0.0;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) s = b ? fma(double(sig2[i]), double(b[i]), s) : s + log(double(sig2[i]));
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sm[0];
}

inline dim3 grid2(int64_t N, int64_t cols) { return dim3((unsigned)((N + 255) / 256), (unsigned)cols); }

}  // namespace

void launch_cg_noise_min(int dtype, hipStream_t s, const void* sv, int64_t N, double* out) {
  if (dtype == 0) hipLaunchKernelGGL(cg_noise_min_kernel<double>, dim3(1), dim3(256), 0, s, (const double*)sv, N, out);
  else hipLaunchKernelGGL(cg_noise_min_kernel<float>, dim3(1), dim3(256), 0, s, (const float*)sv, N, out);
}

void launch_cg_noise_prep(int dtype, hipStream_t s, const void* sv, int64_t N, double diag, void* sig2, void* isig2, void* ssig2, double* isig64) {
  const dim3 g((unsigned)((N + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(cg_noise_prep_kernel<double>, g, dim3(256), 0, s, (const double*)sv, N, diag, (double*)sig2, (double*)isig2, (double*)ssig2, isig64);
  else hipLaunchKernelGGL(cg_noise_prep_kernel<float>, g, dim3(256), 0, s, (const float*)sv, N, float(diag), (float*)sig2, (float*)isig2, (float*)ssig2, isig64);
}

void launch_cg_rowscale(int dtype, hipStream_t s, const void* src, int64_t lds, const void* vec, int64_t N, int64_t ncols, void* dst, int64_t ldd) {
  for (int64_t c0 = 0; c0 < ncols; c0 += 32768) {   // (grid.y limit)
    const int64_t nc = ncols - c0 < 32768 ? ncols - c0 : 32768;
    const dim3 g = grid2(N, nc);
    if (dtype != 1) hipLaunchKernelGGL(cg_rowscale_kernel<double>, g, dim3(256), 0, s, (const double*)src + c0 * lds, lds, (const double*)vec, N, (double*)dst + c0 * ldd, ldd);
    else hipLaunchKernelGGL(cg_rowscale_kernel<float>, g, dim3(256), 0, s, (const float*)src + c0 * lds, lds, (const float*)vec, N, (float*)dst + c0 * ldd, ldd);
  }
}

void launch_cg_sbar(int dtype, hipStream_t s, const void* U, const void* P, int64_t N, int T, void* sbar) {
  const dim3 g((unsigned)((N + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(cg_sbar_kernel<double>, g, dim3(256), 0, s, (const double*)U, (const double*)P, N, T, (double*)sbar);
  else hipLaunchKernelGGL(cg_sbar_kernel<float>, g, dim3(256), 0, s, (const float*)U, (const float*)P, N, T, (float*)sbar);
}

void launch_cg_noise_sum(int dtype, hipStream_t s, const void* sig2, const void* b, int64_t N, double* partial) {
  const int nblk = cg_dot_blocks(N);
  const int64_t per = (N + nblk - 1) / nblk;
  if (dtype == 0) hipLaunchKernelGGL(cg_noise_sum_kernel<double>, dim3((unsigned)nblk), dim3(256), 0, s, (const double*)sig2, (const double*)b, N, per, partial);
  else hipLaunchKernelGGL(cg_noise_sum_kernel<float>, dim3((unsigned)nblk), dim3(256), 0, s, (const float*)sig2, (const float*)b, N, per, partial);
}

void launch_kmv(int dtype, hipStream_t s, const KmvArgs& a) {
  if (dtype == 0) {
    if (a.profile == 0) launch_kmv_p<double, 0>(s, a); else launch_kmv_p<double, 1>(s, a);
  } else {
    if (a.profile == 0) launch_kmv_p<float, 0>(s, a); else launch_kmv_p<float, 1>(s, a);
  }
}

void launch_kmv_prep(int dtype, hipStream_t s, const void* x, int64_t ldx, const void* invl, int d, int64_t N, int64_t Np, void* rows, void* bias) {
  const dim3 grid((unsigned)((Np + 255) / 256));
  const int raw = (dtype != 0 && d <= 8) ? 1 : 0;   // DIFF of the kmv_kernel this d is dispatched to (launch_kmv_p)
  if (dtype == 0) hipLaunchKernelGGL(kmv_prep_kernel<double>, grid, dim3(256), 0, s, (const double*)x, ldx, (const double*)invl, d, N, Np, raw, (double*)rows, (double*)bias);
  else hipLaunchKernelGGL(kmv_prep_kernel<float>, grid, dim3(256), 0, s, (const float*)x, ldx, (const float*)invl, d, N, Np, raw, (float*)rows, (float*)bias);
}

int kmv_split_segments(int64_t N, int64_t n, int64_t* seg_rows) {
  const int64_t chunks = (N + kKmvKC - 1) / kKmvKC, pw = (n + 63) / 64;
  const int64_t want = (1024 + pw - 1) / pw;   // about four workgroups per CU of a 256-CU part
  int64_t cps = (chunks + want - 1) / want;
  if (cps < 8) cps = 8;                        // a segment is at least 256 rows
  *seg_rows = cps * kKmvKC;
  return int((chunks + cps - 1) / cps);
}

void launch_kmv_split(int dtype, hipStream_t s, const KmvArgs& a, void* part) {
  if (dtype == 0) launch_kmv_split_t<double>(s, a, part);
  else launch_kmv_split_t<float>(s, a, part);
}

void launch_cg_widen(int dtype, hipStream_t s, const void* src, int64_t lds, int64_t n, int64_t ncols, double* dst, int64_t ldd) {
  if (dtype == 0) hipLaunchKernelGGL(cg_widen_kernel<double>, grid2(n, ncols), dim3(256), 0, s, (const double*)src, lds, n, dst, ldd);
  else hipLaunchKernelGGL(cg_widen_kernel<float>, grid2(n, ncols), dim3(256), 0, s, (const float*)src, lds, n, dst, ldd);
}

void launch_cg_pc_scale(hipStream_t s, const double* z, int64_t ldz, const double* invl, int d, int64_t k, int64_t Mp, double* zs) {
  hipLaunchKernelGGL(cg_pc_scale_kernel, grid2(Mp, d), dim3(256), 0, s, z, ldz, invl, k, Mp, zs);
}

void launch_cg_pc_form_b(hipStream_t s, const double* A, int64_t Mp, double sigma2, double* Bm) {
  hipLaunchKernelGGL(cg_pc_form_b_kernel, grid2(Mp, Mp), dim3(256), 0, s, A, Mp, 1.0 / sigma2, Bm);
}

void launch_cg_pc_logdet(hipStream_t s, const double* L, int64_t Mp, int64_t k, double* out) {
  hipLaunchKernelGGL(cg_pc_logdet_kernel, dim3(1), dim3(64), 0, s, L, Mp, k, out);
}

void launch_cg_pc_mm(int dtype, hipStream_t s, const double* Mt, int64_t Mp, int64_t k, const void* v, int v_f64, int64_t ldv, int64_t ncols, double alpha,
                     void* out, int64_t ldo, int64_t rows_out) {
  for (int64_t c0 = 0; c0 < ncols; c0 += 32768) {   // (grid.y limit)
    const int64_t nc = ncols - c0 < 32768 ? ncols - c0 : 32768;
    const dim3 g = grid2(rows_out, nc);
    if (dtype == 0) hipLaunchKernelGGL((cg_pc_mm_kernel<double, double>), g, dim3(256), 0, s, Mt, Mp, k, (const double*)v + c0 * ldv, ldv, alpha, (double*)out + c0 * ldo, ldo, rows_out);
    else if (v_f64) hipLaunchKernelGGL((cg_pc_mm_kernel<double, float>), g, dim3(256), 0, s, Mt, Mp, k, (const double*)v + c0 * ldv, ldv, alpha, (float*)out + c0 * ldo, ldo, rows_out);
    else hipLaunchKernelGGL((cg_pc_mm_kernel<float, float>), g, dim3(256), 0, s, Mt, Mp, k, (const float*)v + c0 * ldv, ldv, alpha, (float*)out + c0 * ldo, ldo, rows_out);
  }
}

int cg_dot_blocks(int64_t N) {
  const int64_t nb = (N + 4095) / 4096;
  return int(nb < 1 ? 1 : nb > 256 ? 256 : nb);
}

void launch_cg_dot(int dtype, hipStream_t s, const void* a, int64_t lda, const void* b, int64_t ldb, int64_t N, int64_t ncols, double* partial) {
  const int nblk = cg_dot_blocks(N);
  const int64_t per = (N + nblk - 1) / nblk;
  for (int64_t c0 = 0; c0 < ncols; c0 += 32768) {   // (grid.y limit)
    const int64_t nc = ncols - c0 < 32768 ? ncols - c0 : 32768;
    const dim3 grid((unsigned)nblk, (unsigned)nc);
    if (dtype == 0) hipLaunchKernelGGL(cg_dot_kernel<double>, grid, dim3(256), 0, s, (const double*)a + c0 * lda, lda, (const double*)b + c0 * ldb, ldb, N, per, partial + c0 * nblk);
    else hipLaunchKernelGGL(cg_dot_kernel<float>, grid, dim3(256), 0, s, (const float*)a + c0 * lda, lda, (const float*)b + c0 * ldb, ldb, N, per, partial + c0 * nblk);
  }
}

void launch_cg_colsum(hipStream_t s, const double* partial, int64_t N, int64_t ncols, double* out) {
  hipLaunchKernelGGL(cg_colsum_kernel, dim3((unsigned)((ncols + 63) / 64)), dim3(64), 0, s, partial, cg_dot_blocks(N), ncols, out);
}

void launch_cg_coef(hipStream_t s, int mode, double* st, const double* partial, int64_t N, int ncols, int k, double tol2, double* hist_a, double* hist_b,
                    double* rho) {
  hipLaunchKernelGGL(cg_coef_kernel, dim3(1), dim3(64), 0, s, mode, st, partial, cg_dot_blocks(N), ncols, k, tol2, hist_a, hist_b, rho);
}

void launch_cg_update_xr(int dtype, hipStream_t s, const double* st, int64_t N, int ncols, void* x, void* r, const void* p, const void* q) {
  if (dtype == 0) hipLaunchKernelGGL(cg_update_xr_kernel<double>, grid2(N, ncols), dim3(256), 0, s, st, N, (double*)x, (double*)r, (const double*)p, (const double*)q);
  else hipLaunchKernelGGL(cg_update_xr_kernel<float>, grid2(N, ncols), dim3(256), 0, s, st, N, (float*)x, (float*)r, (const float*)p, (const float*)q);
}

void launch_cg_update_p(int dtype, hipStream_t s, const double* st, int64_t N, int ncols, const void* r, void* p) {
  if (dtype == 0) hipLaunchKernelGGL(cg_update_p_kernel<double>, grid2(N, ncols), dim3(256), 0, s, st, N, (const double*)r, (double*)p);
  else hipLaunchKernelGGL(cg_update_p_kernel<float>, grid2(N, ncols), dim3(256), 0, s, st, N, (const float*)r, (float*)p);
}

void launch_cg_affine(int dtype, hipStream_t s, const void* src, int src_f64, int64_t lds, int64_t N, int64_t ncols, double alpha, double beta, void* dst, int64_t ldd) {
  for (int64_t c0 = 0; c0 < ncols; c0 += 32768) {
    const int64_t nc = ncols - c0 < 32768 ? ncols - c0 : 32768;
    const dim3 g = grid2(N, nc);
    if (dtype == 0) hipLaunchKernelGGL((cg_affine_kernel<double, double>), g, dim3(256), 0, s, (const double*)src + c0 * lds, lds, N, alpha, beta, (double*)dst + c0 * ldd, ldd);
    else if (src_f64) hipLaunchKernelGGL((cg_affine_kernel<float, double>), g, dim3(256), 0, s, (const double*)src + c0 * lds, lds, N, alpha, beta, (float*)dst + c0 * ldd, ldd);
    else hipLaunchKernelGGL((cg_affine_kernel<float, float>), g, dim3(256), 0, s, (const float*)src + c0 * lds, lds, N, alpha, beta, (float*)dst + c0 * ldd, ldd);
  }
}

void launch_cg_kcols(int dtype, hipStream_t s, const void* x, int64_t ldx, int64_t N, const void* xt, int64_t ldt, int64_t nt, const void* invl, int d,
                     int family, double variance, void* out, int64_t ldo) {
  for (int64_t c0 = 0; c0 < nt; c0 += 32768) {
    const int64_t nc = nt - c0 < 32768 ? nt - c0 : 32768;
    const dim3 g = grid2(N, nc);
    if (dtype == 0) hipLaunchKernelGGL(cg_kcols_kernel<double>, g, dim3(256), 0, s, (const double*)x, ldx, N, (const double*)xt + c0, ldt, (const double*)invl, d, family, variance, (double*)out + c0 * ldo, ldo);
    else hipLaunchKernelGGL(cg_kcols_kernel<float>, g, dim3(256), 0, s, (const float*)x, ldx, N, (const float*)xt + c0, ldt, (const float*)invl, d, family, variance, (float*)out + c0 * ldo, ldo);
  }
}

}  // namespace svgp
