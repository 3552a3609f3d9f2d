// predict_grad.hip — predictive mean and variance of the SVGP posterior with their input gradients (svgp_predictor_*: predict_grad_api.hip
// holds the host side).  With xs = invl o x, k_i = variance kappa(r_i^2), r_i^2 = |xs - zs_i|^2, D_ic = 2 g(r_i^2) (xs_c - zs_ic),
// g = variance dkappa / d(r^2), beta = Kuu^-1 (m_u - mean(z)) and the symmetric G = Kuu^-1 (S_u - Kuu) Kuu^-1:
//   mu(x)       = mean(x) + sum_i k_i beta_i                 v(x)        = k(x, x) + k' G k + 1e-18
//   d mu / d x_c = invl_c sum_i D_ic beta_i                   d v / d x_c = 2 invl_c sum_i D_ic (G k)_i        (k(x, x) = variance is constant)
// One data pass of 2 Mp^2 flops a point gives all four.  A workgroup of 4 waves, a wave owns PG groups of 16 points.  The workgroup walks
// the rows of G in blocks of IB = 128 (64 in f64); per block it walks all Mp contraction rows in chunks of KC = 32 staged in LDS (the chunk of the
// inducing rows and the KC x IB chunk of G, read along G's rows: G is symmetric).  Every 16 x 16 Kuf tile is generated TRANSPOSED on the
// MFMA (sample.hip's generation: the expansion form, or by differences for fp32 with d <= 8), and its C/D registers are at once the B
// operand of T[ib, points] += G[ib, k] K[k, points], IB / 16 accumulator tiles a point group; nothing n x M is stored.  The chunks are
// NOT double-buffered: a register-staged prefetch of the next chunk spilled 45 .. 240 VGPRs in every instantiation at the two-wave
// bound, and the two workgroups a CU holds overlap one's loads with the other's MFMAs.  When a block's T is complete its own
// k_i and D_ic are generated again in the accumulators' layout - the coordinate difference per ENTRY, before the product, for the
// cancellation reason of sample_grad.hip - and contracted in registers into the per-point partial sums
//   sum k_i T_i,   sum D_ic T_i,   sum k_i beta_i,   sum D_ic beta_i
// that a lane keeps for the rows it holds; the four lanes of a point meet once at the end (xor 16, then xor 32).  Row blocks ascend,
// every sum has a fixed order, no atomics: a point's results depend on its own MFMA column alone, whatever window, grid or call.
// Coordinates go in blocks of 8 (4 for the widest f64 fragment), one launch per block; the first block writes the mean and the variance.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "predict_grad.hpp"

namespace svgp {

namespace {

constexpr int kPgKC = 32;    // contraction rows per LDS chunk
// rows of G per block (Mp is a multiple of 128): 8 accumulator tiles a point group, 4 of twice the width in f64
template <typename T>
constexpr int pg_row_block() {
  return sizeof(T) == 8 ? 64 : 128;
}

// coordinates per launch: sample_grad.hip's blocks
template <typename T, int DREG>
constexpr int pg_coord_block() {
  return (sizeof(T) == 8 && DREG > 32) ? 4 : 8;
}

// groups of 16 points a wave owns: as many as keep the kernel at two waves per SIMD (<= 256 VGPRs + AGPRs) without a spill.  A group
// costs IB / 16 accumulator tiles (32 registers) and 2 + 2 CB partial sums, and in the fp32 by-differences form of 8 features the 8
// unscaled coordinates of the point and the 32 differences of the tile (two groups there: 34 VGPRs spilled)
template <typename T, int DREG>
constexpr int pg_point_groups() {
  return (sizeof(T) == 8 || DREG > 16 || DREG == 8) ? 1 : 2;
}

template <typename T, int DREG>
__global__ void __launch_bounds__(256, 2) predict_grad_kernel(PredictGradArgs a) {
  constexpr int KS = DREG / 4, KC = kPgKC, IB = pg_row_block<T>(), NTI = IB / 16, NW = 4, CB = pg_coord_block<T, DREG>();
  constexpr int PG = pg_point_groups<T, DREG>();
  constexpr int ZLD = KC + 16, GLD = IB + 4;
  constexpr bool DIFF = sizeof(T) == 4 && DREG <= 8;   // sample_eval_kernel's DIFF: the rows hold z itself (sample_rows_kernel, raw)
  static_assert(!DIFF || DREG <= CB, "the by-differences form keeps every coordinate in one block");
  using acc_t = typename Mfma16<T>::acc_t;
  __shared__ T zc[DREG * ZLD];   // [f][kk]  inducing rows of the chunk
  __shared__ T gc[KC * GLD];     // [kk][i]  G[k0 + kk][ib0 + i]
  __shared__ T tc[KC];           // [kk]     bias
  __shared__ T bc[KC];           // [kk]     beta (the contraction of a finished block)
  const T* __restrict__ rows = static_cast<const T*>(a.rows);
  const T* __restrict__ bias = static_cast<const T*>(a.bias);
  const T* __restrict__ Gm = static_cast<const T*>(a.G);
  const T* __restrict__ beta = static_cast<const T*>(a.beta);
  const T* __restrict__ invl = static_cast<const T*>(a.invl);
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
  const int d = a.d, family = a.family, e0 = a.e0;
  const bool grad = a.mgrad != nullptr || a.vgrad != nullptr;
  const int ne = !grad ? 0 : d - e0 < CB ? d - e0 : CB;   // coordinates of this launch
  const int64_t len = a.len, Mp = a.Mp;
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
  // the lane's partial sums over the rows it holds
  T sv[PG], sm[PG], gv[PG][CB], gm[PG][CB];
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    sv[g] = sm[g] = T(0);
#pragma unroll
    for (int e = 0; e < CB; ++e) gv[g][e] = gm[g][e] = T(0);
  }

  // r^2 of the 16 x 16 tile h of the chunk in LDS for point group g, transposed: register r = row kr[r], point c
  auto tile_r2 = [&](int h, int g, const T (&za)[KS], const T (&tb)[4], const T (&zr)[DIFF ? 4 : 1][DIFF ? DREG : 1],
                     T (&dfr)[DIFF ? 4 : 1][DIFF ? DREG : 1]) -> acc_t {
    acc_t t;
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
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = t[r] < T(0) ? T(0) : t[r];
    (void)h;
    return t;
  };
  // the tile's operands from LDS: the generation's A fragment, the bias and (DIFF) every feature of the lane's four rows
  auto tile_operands = [&](int h, T (&za)[KS], int (&kr)[4], T (&tb)[4], T (&zr)[DIFF ? 4 : 1][DIFF ? DREG : 1]) {
#pragma unroll
    for (int q = 0; q < KS; ++q) za[q] = zc[(4 * q + kq) * ZLD + h * 16 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      kr[r] = h * 16 + Mfma16<T>::row(lane, r);
      tb[r] = tc[kr[r]];
    }
    if constexpr (DIFF) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int f = 0; f < DREG; ++f) zr[r][f] = zc[f * ZLD + kr[r]];
    }
  };

  for (int64_t ib0 = 0; ib0 < Mp; ib0 += IB) {
    acc_t acc[PG][NTI];
#pragma unroll
    for (int g = 0; g < PG; ++g)
#pragma unroll
      for (int t = 0; t < NTI; ++t) acc[g][t] = acc_t{0, 0, 0, 0};
    for (int64_t k0 = 0; k0 < Mp; k0 += KC) {
      __syncthreads();   // the previous chunk has been read
      for (int idx = tid; idx < KC * IB; idx += 256) {
        const int kk = idx / IB, ii = idx % IB;
        gc[kk * GLD + ii] = Gm[(k0 + kk) * Mp + ib0 + ii];
      }
      for (int idx = tid; idx < DREG * KC; idx += 256) {
        const int f = idx / KC, kk = idx % KC;
        zc[f * ZLD + kk] = (f < d) ? rows[int64_t(f) * Mp + k0 + kk] : T(0);
      }
      if (tid < KC) tc[tid] = bias[k0 + tid];
      __syncthreads();
#pragma unroll
      for (int h = 0; h < KC / 16; ++h) {
        T za[KS], tb[4];
        int kr[4];
        T zr[DIFF ? 4 : 1][DIFF ? DREG : 1], dfr[DIFF ? 4 : 1][DIFF ? DREG : 1];
        tile_operands(h, za, kr, tb, zr);
        acc_t kt[PG];
#pragma unroll
        for (int g = 0; g < PG; ++g) {
          kt[g] = acc_t{0, 0, 0, 0};
          if (p0 + g * 16 >= len) continue;   // wave-uniform
          const acc_t t = tile_r2(h, g, za, tb, zr, dfr);
#pragma unroll
          for (int r = 0; r < 4; ++r) kt[g][r] = kappa<T>(family, t[r], variance);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int t = 0; t < NTI; ++t) {
            const T ga = gc[kr[r] * GLD + t * 16 + c];   // G[ib0 + 16 t + c][k0 + kr]
#pragma unroll
            for (int g = 0; g < PG; ++g)
              if (p0 + g * 16 < len) acc[g][t] = Mfma16<T>::mma(ga, kt[g][r], acc[g][t]);
          }
      }
    }
    // the block's T is complete: its own k_i and D_ic again, 32 rows (two accumulator tiles) a chunk
#pragma unroll
    for (int ch = 0; ch < IB / KC; ++ch) {
      __syncthreads();
      for (int idx = tid; idx < DREG * KC; idx += 256) {
        const int f = idx / KC, kk = idx % KC;
        zc[f * ZLD + kk] = (f < d) ? rows[int64_t(f) * Mp + ib0 + ch * KC + kk] : T(0);
      }
      if (tid < KC) {
        tc[tid] = bias[ib0 + ch * KC + tid];
        bc[tid] = beta[ib0 + ch * KC + tid];
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < KC / 16; ++h) {
        T za[KS], tb[4], bt[4];
        int kr[4];
        T zr[DIFF ? 4 : 1][DIFF ? DREG : 1], dfr[DIFF ? 4 : 1][DIFF ? DREG : 1];
        tile_operands(h, za, kr, tb, zr);
#pragma unroll
        for (int r = 0; r < 4; ++r) bt[r] = bc[kr[r]];
#pragma unroll
        for (int g = 0; g < PG; ++g) {
          if (p0 + g * 16 >= len) continue;   // wave-uniform
          const acc_t t = tile_r2(h, g, za, tb, zr, dfr);
          const acc_t Tt = acc[g][ch * (KC / 16) + h];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const T kv = kappa<T>(family, t[r], variance);
            const T dv = kappa_2g<T>(family, t[r], variance, kv);
            sv[g] = fma(kv, Tt[r], sv[g]);
            sm[g] = fma(kv, bt[r], sm[g]);
#pragma unroll
            for (int e = 0; e < CB; ++e) {
              if (e >= ne) break;   // wave-uniform
              T df;
              if constexpr (DIFF) df = dfr[r][e < DREG ? e : 0];
              else df = fma(T(0.5), zc[(e0 + e) * ZLD + kr[r]], xsb[g][e]);   // xs_c - zs_ic from the row -2 zs_ic, rounded once
              const T D = dv * df;
              gv[g][e] = fma(D, Tt[r], gv[g][e]);
              gm[g][e] = fma(D, bt[r], gm[g][e]);
            }
          }
        }
      }
    }
  }

  const T* __restrict__ mux = static_cast<const T*>(a.mux);
  T* __restrict__ mean = static_cast<T*>(a.mean);
  T* __restrict__ var = static_cast<T*>(a.var);
  T* __restrict__ mgrad = static_cast<T*>(a.mgrad);
  T* __restrict__ vgrad = static_cast<T*>(a.vgrad);
  const T mc = T(a.mean_const);
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    // the four lanes of a point, in a fixed order
    sv[g] += __shfl_xor(sv[g], 16);
    sv[g] += __shfl_xor(sv[g], 32);
    sm[g] += __shfl_xor(sm[g], 16);
    sm[g] += __shfl_xor(sm[g], 32);
#pragma unroll
    for (int e = 0; e < CB; ++e) {
      gv[g][e] += __shfl_xor(gv[g][e], 16);
      gv[g][e] += __shfl_xor(gv[g][e], 32);
      gm[g][e] += __shfl_xor(gm[g][e], 16);
      gm[g][e] += __shfl_xor(gm[g][e], 32);
    }
    const int64_t pt = p0 + g * 16 + c;
    if (pt >= len || kq != 0) continue;
    if (e0 == 0) {
      if (mean) mean[pt] = (mux ? mc + mux[pt] : mc) + sm[g];
      if (var) var[pt] = (variance + sv[g]) + T(1e-18);
    }
#pragma unroll
    for (int e = 0; e < CB; ++e) {
      if (e >= ne) break;
      const T ile = invl[e0 + e];
      if (mgrad) mgrad[int64_t(e0 + e) * a.ldg + pt] = ile * gm[g][e];
      if (vgrad) vgrad[int64_t(e0 + e) * a.ldg + pt] = T(2) * ile * gv[g][e];
    }
  }
}

template <typename T, int DREG>
void launch_pg_d(hipStream_t s, const PredictGradArgs& a0) {
  PredictGradArgs a = a0;
  const int64_t per = 4 * 16 * pg_point_groups<T, DREG>();   // points per workgroup
  const dim3 grid((unsigned)((a.len + per - 1) / per));
  const bool grad = a.mgrad != nullptr || a.vgrad != nullptr;
  for (int e0 = 0; e0 < (grad ? a.d : 1); e0 += pg_coord_block<T, DREG>()) {   // one block of coordinates per launch
    a.e0 = e0;
    hipLaunchKernelGGL((predict_grad_kernel<T, DREG>), grid, dim3(256), 0, s, a);
  }
}

template <typename T>
void launch_pg_t(hipStream_t s, const PredictGradArgs& a) {   // the DREG of sample.hip's launch_eval_t: the rows' layout follows it
  if (a.d <= 4) launch_pg_d<T, 4>(s, a);
  else if (a.d <= 8) launch_pg_d<T, 8>(s, a);
  else if (a.d <= 16) launch_pg_d<T, 16>(s, a);
  else if (a.d <= 32) launch_pg_d<T, 32>(s, a);
  else launch_pg_d<T, 64>(s, a);
}

// ---- the M-sized stage (fp64) -------------------------------------------------------------------------------------------------

template <typename T>
__global__ void __launch_bounds__(k256) pg_widen_q_kernel(const T* __restrict__ Lq, const T* __restrict__ m, const T* __restrict__ muz, int64_t M,
                                                          int64_t Mp, int centered, double mean_const, double* __restrict__ Lq64,
                                                          double* __restrict__ mv) {
  const int64_t i = int64_t(blockIdx.x) * k256 + threadIdx.x, j = blockIdx.y;
  if (i >= Mp) return;
  Lq64[i + j * Mp] = (i < M && j <= i) ? double(Lq[i + j * M]) : 0.0;
  if (j == 0) {
    double v = 0.0;
    if (i < M) v = centered ? (double(m[i]) - mean_const) - (muz ? double(muz[i]) : 0.0) : double(m[i]);
    mv[i] = v;
  }
}

// C[i + j Mp] = sum_k A[k + i Mp] B[k + j Mp] - W[i + j Mp], k ascending in one chain; 16 x 16 entries a workgroup
__global__ void __launch_bounds__(k256) pg_atb_kernel(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ W,
                                                      int64_t Mp, int64_t Mvalid, int alow, int blow, double* __restrict__ C) {
  __shared__ double As[16][17], Bs[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t i = int64_t(blockIdx.x) * 16 + tx, j = int64_t(blockIdx.y) * 16 + ty;
  const int64_t ia = int64_t(blockIdx.x) * 16 + ty, jb = j;
  double acc = 0.0;
  for (int64_t k0 = 0; k0 < Mp; k0 += 16) {
    const int64_t k = k0 + tx;
    As[tx][ty] = (alow && k < ia) ? 0.0 : A[k + ia * Mp];
    Bs[tx][ty] = (blow && k < jb) ? 0.0 : B[k + jb * Mp];
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = fma(As[kk][tx], Bs[kk][ty], acc);
    __syncthreads();
  }
  if (W) acc -= W[i + j * Mp];
  if (Mvalid >= 0 && (i >= Mvalid || j >= Mvalid)) acc = 0.0;
  C[i + j * Mp] = acc;
}

template <typename T>
__global__ void __launch_bounds__(k256) pg_round_kernel(const double* __restrict__ G64, const double* __restrict__ beta64, int64_t Mp,
                                                        T* __restrict__ G, T* __restrict__ beta) {
  const int64_t i = int64_t(blockIdx.x) * k256 + threadIdx.x, j = blockIdx.y;
  if (i >= Mp) return;
  G[i + j * Mp] = T(G64[i + j * Mp]);
  if (j == 0) beta[i] = T(beta64[i]);
}

}  // namespace

void launch_predict_grad(int dtype, hipStream_t s, const PredictGradArgs& a) {
  if (dtype == 0) launch_pg_t<double>(s, a); else launch_pg_t<float>(s, a);
}

void launch_pg_widen_q(int dtype, hipStream_t s, const void* Lq, const void* m, const void* muz, int64_t M, int64_t Mp, int centered,
                       double mean_const, double* Lq64, double* mv) {
  const dim3 grid((unsigned)((Mp + k256 - 1) / k256), (unsigned)Mp);
  if (dtype == 0) hipLaunchKernelGGL(pg_widen_q_kernel<double>, grid, dim3(k256), 0, s, (const double*)Lq, (const double*)m, (const double*)muz, M, Mp, centered, mean_const, Lq64, mv);
  else hipLaunchKernelGGL(pg_widen_q_kernel<float>, grid, dim3(k256), 0, s, (const float*)Lq, (const float*)m, (const float*)muz, M, Mp, centered, mean_const, Lq64, mv);
}

void launch_pg_atb(hipStream_t s, const double* A, const double* B, const double* W, int64_t Mp, int64_t Mvalid, int alow, int blow, double* C) {
  const dim3 grid((unsigned)(Mp / 16), (unsigned)(Mp / 16));
  hipLaunchKernelGGL(pg_atb_kernel, grid, dim3(k256), 0, s, A, B, W, Mp, Mvalid, alow, blow, C);
}

void launch_pg_round(int dtype, hipStream_t s, const double* G64, const double* beta64, int64_t Mp, void* G, void* beta) {
  const dim3 grid((unsigned)((Mp + k256 - 1) / k256), (unsigned)Mp);
  if (dtype == 0) hipLaunchKernelGGL(pg_round_kernel<double>, grid, dim3(k256), 0, s, G64, beta64, Mp, (double*)G, (double*)beta);
  else hipLaunchKernelGGL(pg_round_kernel<float>, grid, dim3(k256), 0, s, G64, beta64, Mp, (float*)G, (float*)beta);
}

}  // namespace svgp
