// sample.hip — pathwise posterior function samples (svgp_sampler_*: sample_api.hip holds the host side).
//   f_s(x) = mean(x) + sum_l phi_l(x) w_sl + sum_i k(x, z_i) V_is,     phi_l(x) = sqrt(2 variance / L) cos(omega_l . (invl o x) + tau_l)
// The data-sized kernel (sample_eval_kernel) walks ONE contraction index k over the L features, then the Mp inducing points: for
// every 16 x 16 tile (16 rows k, 16 points) it generates the tile with the MFMA - rows[f][k] . xs[f][point] + bias[k], which is the
// phase of a feature row and r^2 of an inducing row (the expansion form of the Kuf kernels: bias = |zs|^2, rows = -2 zs, + |xs|^2) -
// applies cos or kappa<T>, and feeds the result straight back to the MFMA against the panel [amp W; V] ((Lp + Mp) x Sp).  The tile is
// generated TRANSPOSED (row index = MFMA row, point = MFMA column): its C/D registers are then exactly the B operand of the second
// product out'[s][point] += panel[k][s] tile[k][point], so no tile ever passes through LDS or memory.  Every sum has a fixed order
// (k ascending in steps of 4 inside one accumulator chain), no atomics; a point's value depends on its own MFMA column alone, so it
// does not depend on the window, the grid or the call it is evaluated in.
// The M-sized stage (u, Phi(z) w, the right-hand sides of V) is a handful of small fp64 kernels, whatever the model's dtype.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {

namespace {

__device__ __forceinline__ double kcos(double v) { return cos(v); }
__device__ __forceinline__ float kcos(float v) { return cosf(v); }

constexpr int kSampleKC = 32;   // contraction rows per LDS chunk (Lp and Mp are multiples of it)

// groups of 16 points a wave owns: as many as keep the kernel at two waves per SIMD (<= 256 VGPRs + AGPRs) - the x fragments grow with
// DREG, the accumulators with NSB, both twice as wide in f64
template <typename T, int DREG, int NSB>
constexpr int sample_point_groups() {
  return (sizeof(T) == 8 && DREG > 32 && NSB > 1) ? 1 : (DREG > 16 || NSB > 1) ? 2 : 4;
}

// One workgroup = 4 waves; a wave owns PG groups of 16 points and, per launch, NSB 16-column blocks of the panel (<= 64 samples).
// The chunk of rows / bias / panel is staged in LDS once per workgroup and read by its 4 x PG point groups.
// fp32: the phase sum_f omega_lf xs_f + tau_l is accumulated by the fp32 MFMA, so it carries an absolute error of about
// eps32 |phase| (|phase| grows with |omega| |x| / lengthscale) before cosf reduces it; the fp64 build has the same form at eps64.
// The phase is not reduced or widened: tests/test_gpu_pathwise.py measures the fp32 data stage against the fp64 one per case
// (profiles/sample/accuracy.md) and the numpy fp32 chain loses the same digits.
template <typename T, int DREG, int NSB>
__global__ void __launch_bounds__(256) sample_eval_kernel(SampleEvalArgs a) {
  constexpr int KS = DREG / 4, KC = kSampleKC, NW = 4;
  constexpr int PG = sample_point_groups<T, DREG, NSB>();
  constexpr int ZLD = KC + 16, PLD = NSB * 16 + 4;
  // fp32, d <= 8: r^2 of the inducing rows by differences on the VALU, not by the expansion on the MFMA.  The expansion loses
  // eps32 (|xs|^2 + |zs|^2) absolutely, and a short lengthscale on a long domain (d = 1, M = 37 on [-3, 3]: |xs| <= 30) makes that 1e-4
  // of r^2, which Kuu^-1 (max|V| of tens) turns into more than the fp32 contract of the sample; 2 d instructions per entry cost less
  // than kappa at these d.  Wider inputs have scaled coordinates of order one and keep the MFMA form, as the Kuf kernels do.
  // The difference is taken of the UNSCALED coordinates and scaled afterwards, (x_f - z_f) invl_f: x_f invl_f - z_f invl_f loses
  // eps32 |xs| absolutely (|xs| reaches 300 at d = 1, M = 300: 1.3e-4 of the sample, tests/fuzz_pathwise.py REPLAYS), the unscaled
  // difference only eps32 |x_f - z_f|.  The inducing rows of such a sampler hold z itself (sample_rows_kernel, raw).
  constexpr bool DIFF = sizeof(T) == 4 && DREG <= 8;
  using acc_t = typename Mfma16<T>::acc_t;
  __shared__ T zc[DREG * ZLD];   // [f][kk]  rows of the chunk (MFMA A operand of the generation)
  __shared__ T pc[KC * PLD];     // [kk][j]  panel rows of the chunk, the launch's column block
  __shared__ T tc[KC];           // [kk]     bias
  const T* __restrict__ rows = static_cast<const T*>(a.rows);
  const T* __restrict__ bias = static_cast<const T*>(a.bias);
  const T* __restrict__ panel = static_cast<const T*>(a.panel);
  const T* __restrict__ invl = static_cast<const T*>(a.invl);
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ mux = static_cast<const T*>(a.mux);
  T* __restrict__ out = static_cast<T*>(a.out);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
  const int d = a.d, family = a.family;
  const int64_t len = a.len, Kp = a.Lp + a.Mp;
  const T variance = T(a.variance);
  const int64_t p0 = (int64_t(blockIdx.x) * NW + wave) * (PG * 16);
  // the wave's points: feature 4 q + kq of point c of group g, scaled (B operand of the generation), and |xs|^2 of point c
  T xb[PG][KS], xn[PG];
  T xall[DIFF ? PG : 1][DIFF ? DREG : 1];   // DIFF: every feature of point c, unscaled
  T il[DIFF ? DREG : 1];
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
  acc_t acc[PG][NSB];
#pragma unroll
  for (int g = 0; g < PG; ++g)
#pragma unroll
    for (int b = 0; b < NSB; ++b) acc[g][b] = acc_t{0, 0, 0, 0};

  for (int64_t k0 = 0; k0 < Kp; k0 += KC) {
    const bool feat = k0 < a.Lp;   // a chunk holds features or inducing rows, never both
    __syncthreads();               // the previous chunk has been read
    for (int idx = tid; idx < DREG * KC; idx += 256) {
      const int f = idx / KC, kk = idx % KC;
      zc[f * ZLD + kk] = (f < d) ? rows[int64_t(f) * Kp + k0 + kk] : T(0);
    }
    for (int idx = tid; idx < KC * NSB * 16; idx += 256) {
      const int kk = idx / (NSB * 16), j = idx % (NSB * 16);
      pc[kk * PLD + j] = (a.s0 + j < a.Sp) ? panel[(k0 + kk) * a.Sp + a.s0 + j] : T(0);
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
        const int kk = h * 16 + Mfma16<T>::row(lane, r);   // the row this lane's register r holds after the generation
        tb[r] = tc[kk];
#pragma unroll
        for (int b = 0; b < NSB; ++b) pa[r][b] = pc[kk * PLD + b * 16 + c];
      }
      T zr[DIFF ? 4 : 1][DIFF ? DREG : 1];   // DIFF: every feature of the lane's four rows (the chunk holds z itself)
      if constexpr (DIFF) {
        if (!feat) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int f = 0; f < DREG; ++f) zr[r][f] = zc[f * ZLD + h * 16 + Mfma16<T>::row(lane, r)];
        }
      }
#pragma unroll
      for (int g = 0; g < PG; ++g) {
        if (p0 + g * 16 >= len) break;   // wave-uniform
        acc_t t;
        if (DIFF && !feat) {
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
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = feat ? tb[r] : tb[r] + xn[g];
#pragma unroll
          for (int q = 0; q < KS; ++q) t = Mfma16<T>::mma(za[q], xb[g][q], t);
        }
        if (feat) {
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = kcos(t[r]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = kappa<T>(family, t[r] < T(0) ? T(0) : t[r], variance);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int b = 0; b < NSB; ++b) acc[g][b] = Mfma16<T>::mma(pa[r][b], t[r], acc[g][b]);
      }
    }
  }
  const T mc = T(a.mean_const);
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    const int64_t pt = p0 + g * 16 + c;
    if (pt >= len) continue;
    const T mean = mux ? mc + mux[pt] : mc;
#pragma unroll
    for (int b = 0; b < NSB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t s = a.s0 + b * 16 + Mfma16<T>::row(lane, r);
        if (s < a.S) out[s * a.ldo + pt] = mean + acc[g][b][r];
      }
  }
}

template <typename T, int DREG>
void launch_eval_d(hipStream_t s, const SampleEvalArgs& a0) {
  SampleEvalArgs a = a0;
  for (int64_t s0 = 0; s0 < a.Sp; s0 += 64) {   // column blocks of at most 64 samples, one launch each
    a.s0 = s0;
    const bool one = a.Sp - s0 <= 16;
    const int64_t per = 4 * 16 * (one ? sample_point_groups<T, DREG, 1>() : sample_point_groups<T, DREG, 4>());   // points per workgroup
    const dim3 grid((unsigned)((a.len + per - 1) / per));
    if (one) hipLaunchKernelGGL((sample_eval_kernel<T, DREG, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((sample_eval_kernel<T, DREG, 4>), grid, dim3(256), 0, s, a);
  }
}

template <typename T>
void launch_eval_t(hipStream_t s, const SampleEvalArgs& a) {
  if (a.d <= 4) launch_eval_d<T, 4>(s, a);
  else if (a.d <= 8) launch_eval_d<T, 8>(s, a);
  else if (a.d <= 16) launch_eval_d<T, 16>(s, a);
  else if (a.d <= 32) launch_eval_d<T, 32>(s, a);
  else launch_eval_d<T, 64>(s, a);
}

// ---- the M-sized stage (fp64) -------------------------------------------------------------------------------------------------

// zs64[f][i] = z_i,f * invl64[f] (i < M), 0 on the padding; z in the model's dtype and layout
template <typename T>
__global__ void sample_widen_z_kernel(const T* __restrict__ z, int layout, int d, int64_t M, int64_t Mp, const double* __restrict__ invl64,
                                      double* __restrict__ zs64) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int f = blockIdx.y;
  if (i >= Mp) return;
  double v = 0.0;
  if (i < M) v = double(layout == 1 ? z[int64_t(f) * M + i] : z[i * d + f]) * invl64[f];
  zs64[int64_t(f) * Mp + i] = v;
}

// the generation operands of the data stage in the model's dtype: rows[f][k] = omega_k,f (k < L), 0 (L <= k < Lp), -2 zs_f,i (k = Lp + i);
// bias[k] = tau_k, 0, |zs_i|^2 (from the ROUNDED zs, as the Kuf kernels form it).  raw (the by-differences kernels): the inducing rows
// hold z_f,i itself (i < M; 0 on the padding, whose panel rows are zero) and their bias is not read
template <typename T>
__global__ void sample_rows_kernel(const double* __restrict__ zs64, const T* __restrict__ z, int layout, int64_t M, int raw,
                                   const T* __restrict__ omega, const T* __restrict__ tau, int d, int64_t L,
                                   int64_t Lp, int64_t Mp, T* __restrict__ rows, T* __restrict__ bias) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t Kp = Lp + Mp;
  if (k >= Kp) return;
  T s = T(0);
  for (int f = 0; f < d; ++f) {
    T r;
    if (k < Lp) {
      r = (k < L) ? omega[k * d + f] : T(0);
    } else {
      const int64_t i = k - Lp;
      const T v = T(zs64[int64_t(f) * Mp + i]);
      r = raw ? (i < M ? (layout == 1 ? z[int64_t(f) * M + i] : z[i * d + f]) : T(0)) : T(-2) * v;
      s = fma(v, v, s);
    }
    rows[int64_t(f) * Kp + k] = r;
  }
  bias[k] = (k < Lp) ? ((k < L) ? tau[k] : T(0)) : s;
}

// one block per sample s: rhs[s][i] = (u_s - mean(z))_i, u[s][i] = u_s,i (fp64; rhs zero on the padding)
//   NonCentered: u - mean(z) = Lk (m + Lq eps_s);   Centered: u - mean(z) = (m - mean_const - muz) + Lq eps_s
// sums over j ascending, one thread per row: a fixed order
template <typename T>
__global__ void __launch_bounds__(256) sample_u_kernel(const T* __restrict__ m, const T* __restrict__ Lq, const T* __restrict__ eps,
                                                       const T* __restrict__ muz, const double* __restrict__ Lk, int64_t M, int64_t Mp,
                                                       int centered, double mean_const, double* __restrict__ tmp,
                                                       double* __restrict__ rhs, double* __restrict__ u) {
  const int64_t s = blockIdx.x;
  const T* __restrict__ e = eps + s * M;
  double* __restrict__ t = tmp + s * Mp;
  for (int64_t i = threadIdx.x; i < Mp; i += blockDim.x) {
    double v = 0.0;
    if (i < M) {
      for (int64_t j = 0; j <= i; ++j) v = fma(double(Lq[i + j * M]), double(e[j]), v);
      const double mi = double(m[i]);
      v = centered ? ((mi - mean_const) - (muz ? double(muz[i]) : 0.0)) + v : mi + v;
    }
    if (centered) rhs[s * Mp + i] = v; else t[i] = v;
    if (centered && i < M) u[s * M + i] = v + (mean_const + (muz ? double(muz[i]) : 0.0));
  }
  if (centered) return;
  __threadfence_block();
  __syncthreads();   // t was written by this block (global memory, block scope)
  for (int64_t i = threadIdx.x; i < Mp; i += blockDim.x) {
    double v = 0.0;
    if (i < M) {
      for (int64_t j = 0; j <= i; ++j) v = fma(Lk[i + j * Mp], t[j], v);
      u[s * M + i] = v + (mean_const + (muz ? double(muz[i]) : 0.0));
    }
    rhs[s * Mp + i] = v;
  }
}

// rhs[s][i] -= sum_l amp cos(sum_f omega_l,f zs64_f,i + tau_l) w_s,l  (fp64, l ascending).  One block per inducing point i and 256 samples:
// per chunk of 256 features every thread evaluates one cosine, then thread s adds the chunk to its own sum
template <typename T>
__global__ void __launch_bounds__(256) sample_phiz_kernel(const double* __restrict__ zs64, const T* __restrict__ omega, const T* __restrict__ tau,
                                                          const T* __restrict__ w, int d, int64_t L, int64_t S, int64_t Mp, double amp,
                                                          double* __restrict__ rhs) {
  __shared__ double cs[256];
  __shared__ double zi[64];
  const int64_t i = blockIdx.x;
  const int64_t s = int64_t(blockIdx.y) * 256 + threadIdx.x;
  if (threadIdx.x < d) zi[threadIdx.x] = zs64[int64_t(threadIdx.x) * Mp + i];
  double sum = 0.0;
  for (int64_t l0 = 0; l0 < L; l0 += 256) {
    __syncthreads();
    const int64_t l = l0 + threadIdx.x;
    if (l < L) {
      double ph = 0.0;
      for (int f = 0; f < d; ++f) ph = fma(double(omega[l * d + f]), zi[f], ph);
      cs[threadIdx.x] = cos(ph + double(tau[l]));
    }
    __syncthreads();
    if (s < S) {
      const int64_t nl = (L - l0 < 256) ? L - l0 : 256;
      for (int64_t q = 0; q < nl; ++q) sum = fma(cs[q], double(w[s * L + l0 + q]), sum);
    }
  }
  if (s < S) rhs[s * Mp + i] -= amp * sum;
}

// panel[k][s] in the model's dtype, each entry rounded once: amp w_s,k (k < L), V_s,i (k = Lp + i, i < M), 0 on every padding row / column
template <typename T>
__global__ void sample_panel_kernel(const T* __restrict__ w, const double* __restrict__ V, int64_t L, int64_t Lp, int64_t M, int64_t Mp, int64_t S,
                                    int64_t Sp, double amp, T* __restrict__ panel) {
  const int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= (Lp + Mp) * Sp) return;
  const int64_t k = idx / Sp, s = idx % Sp;
  double v = 0.0;
  if (s < S) {
    if (k < L) v = amp * double(w[s * L + k]);
    else if (k >= Lp && k - Lp < M) v = V[s * Mp + (k - Lp)];
  }
  panel[idx] = T(v);
}

}  // namespace

void launch_sample_eval(int dtype, hipStream_t s, const SampleEvalArgs& a) {
  if (dtype == 0) launch_eval_t<double>(s, a); else launch_eval_t<float>(s, a);
}

void launch_sample_widen_z(int dtype, hipStream_t s, const void* z, int layout, int d, int64_t M, int64_t Mp, const double* invl64, double* zs64) {
  const dim3 grid((unsigned)((Mp + 255) / 256), (unsigned)d);
  if (dtype == 0) hipLaunchKernelGGL(sample_widen_z_kernel<double>, grid, dim3(256), 0, s, (const double*)z, layout, d, M, Mp, invl64, zs64);
  else hipLaunchKernelGGL(sample_widen_z_kernel<float>, grid, dim3(256), 0, s, (const float*)z, layout, d, M, Mp, invl64, zs64);
}

void launch_sample_rows(int dtype, hipStream_t s, const double* zs64, const void* z, int layout, int64_t M, const void* omega, const void* tau, int d,
                        int64_t L, int64_t Lp, int64_t Mp, void* rows, void* bias) {
  const dim3 grid((unsigned)((Lp + Mp + 255) / 256));
  const int raw = (dtype != 0 && d <= 8) ? 1 : 0;   // DIFF of the sample_eval_kernel this d is dispatched to (launch_eval_t)
  if (dtype == 0) hipLaunchKernelGGL(sample_rows_kernel<double>, grid, dim3(256), 0, s, zs64, (const double*)z, layout, M, raw, (const double*)omega, (const double*)tau, d, L, Lp, Mp, (double*)rows, (double*)bias);
  else hipLaunchKernelGGL(sample_rows_kernel<float>, grid, dim3(256), 0, s, zs64, (const float*)z, layout, M, raw, (const float*)omega, (const float*)tau, d, L, Lp, Mp, (float*)rows, (float*)bias);
}

void launch_sample_u(int dtype, hipStream_t s, const void* m, const void* Lq, const void* eps, const void* muz, const double* Lk, int64_t M,
                     int64_t Mp, int64_t S, int centered, double mean_const, double* tmp, double* rhs, double* u) {
  if (dtype == 0) hipLaunchKernelGGL(sample_u_kernel<double>, dim3((unsigned)S), dim3(256), 0, s, (const double*)m, (const double*)Lq, (const double*)eps, (const double*)muz, Lk, M, Mp, centered, mean_const, tmp, rhs, u);
  else hipLaunchKernelGGL(sample_u_kernel<float>, dim3((unsigned)S), dim3(256), 0, s, (const float*)m, (const float*)Lq, (const float*)eps, (const float*)muz, Lk, M, Mp, centered, mean_const, tmp, rhs, u);
}

void launch_sample_phiz(int dtype, hipStream_t s, const double* zs64, const void* omega, const void* tau, const void* w, int d, int64_t M, int64_t L,
                        int64_t S, int64_t Mp, double amp, double* rhs) {
  if (L < 1) return;
  const dim3 grid((unsigned)M, (unsigned)((S + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(sample_phiz_kernel<double>, grid, dim3(256), 0, s, zs64, (const double*)omega, (const double*)tau, (const double*)w, d, L, S, Mp, amp, rhs);
  else hipLaunchKernelGGL(sample_phiz_kernel<float>, grid, dim3(256), 0, s, zs64, (const float*)omega, (const float*)tau, (const float*)w, d, L, S, Mp, amp, rhs);
}

void launch_sample_panel(int dtype, hipStream_t s, const void* w, const double* V, int64_t L, int64_t Lp, int64_t M, int64_t Mp, int64_t S, int64_t Sp,
                         double amp, void* panel) {
  const dim3 grid((unsigned)(((Lp + Mp) * Sp + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(sample_panel_kernel<double>, grid, dim3(256), 0, s, (const double*)w, V, L, Lp, M, Mp, S, Sp, amp, (double*)panel);
  else hipLaunchKernelGGL(sample_panel_kernel<float>, grid, dim3(256), 0, s, (const float*)w, V, L, Lp, M, Mp, S, Sp, amp, (float*)panel);
}

}  // namespace svgp
