// nn_points.hip — the NearestNeighbors point kernels with per-point noise variances and prior-mean offsets
// (svgp_nn_set_noise / svgp_nn_set_mean) and the per-point gradient of svgp_nn_lml_grad_points.
//   sigma_j^2 = T(diag) + s_j (data dtype T, one rounding),   delta_j = y_j - mean_const - mu_j
//   C = k(ns, ns) + diag(sigma^2_ns),  c = k(ns, x_i),  kd = variance + sigma_i^2;  b, w, F, r, gF as in nn.hip
//   s_bar_j    = d lml / d sigma_j^2 = gF_j + sum_{(i, t): ns(i)_t = j} (gF_i b_it^2 - (r_i / F_i) w_it b_it)     (the diagonal of C_bar)
//   mean_bar_j = d lml / d mu_j      = alpha_j                                                                 (the alpha of the fit)
// nn_point_body_v is nn.hip's nn_point_body line for line, with one more load per lane per vector: a sibling, not a template flag
// on the body, for the reason written above nn_block in nn.hip (the existing instantiations keep their registers only untouched),
// and a translation unit of its own so that those instantiations are compiled from the text they were.  Either vector may be
// null: zeros, and then every expression reduces to nn_point_body's own, bit for bit (T(diag) + 0, delta - 0.0, the same floor and
// the same closed forms), which is what makes the scalars of svgp_nn_lml_grad_points those of svgp_nn_lml_grad.
#include <hip/hip_runtime.h>

#include "nn_points.hpp"

namespace svgp {
namespace {

// MODE 0: the lml slots.  MODE 1: + b_i, F_i, r_i / F_i (fit).  MODE 2: + the gradient slots.  MODE 3: MODE 2 with MODE 1's stores,
// gF_i and the per-pair terms Qd (laid out like Bd).
template <typename T, int KB, int MODE, bool G>
__device__ __forceinline__ void nn_point_body_v(const NnParams& P, const T* __restrict__ x, const T* __restrict__ y,
                                                const T* __restrict__ sv, const T* __restrict__ mu, double* __restrict__ terms, int S,
                                                int* __restrict__ bad, T* __restrict__ Bd, double* __restrict__ Fd,
                                                double* __restrict__ rFd, T* __restrict__ Qd, double* __restrict__ gFd,
                                                const int* __restrict__ nbr) {
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  if (i >= P.n) return;
  int m;
  int64_t base, src = 0;
  if constexpr (G) {
    const int e = lane < P.k ? nbr[i + int64_t(lane) * P.n] : -1;
    m = __builtin_amdgcn_readfirstlane(__popcll(__ballot(e >= 0)));
    base = 0;
    src = e;
  } else {
    m = i < P.k ? int(i) : P.k;
    base = i - m;
  }
  const bool act = lane < m;
  const T variance = T(P.variance);
  // the two vectors at the lane's neighbour and at point i
  const T sig = T(P.diag) + ((sv && act) ? sv[G ? src : base + lane] : T(0));   // sigma_j^2
  const double sigi = sv ? double(T(P.diag) + sv[i]) : P.diag;                  // sigma_i^2
  double smax = sigi;                                                           // the largest of the block, point i included
  if (sv) {
    double sl = act ? double(sig) : sigi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sl = fmax(sl, __shfl_xor(sl, o));
    smax = fmax(sl, sigi);
  }
  T A[KB], c;
  nn_dist2<T, KB, G>(P, x, base, i, lane, m, A, c, src);
  // the block: C on the m x m corner, identity on the padding
#pragma unroll
  for (int g = 0; g < KB / 8; ++g) {
    if (g * 8 < m) {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) {
        const T kv = kappa(P.family, A[q], variance) + (q == lane ? sig : T(0));
        A[q] = (act && q < m) ? kv : (q == lane ? T(1) : T(0));
      }
    } else {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = q == lane ? T(1) : T(0);
    }
  }
  c = act ? kappa(P.family, c, variance) : T(0);
  T dd = act ? T(double(y[G ? src : base + lane]) - P.mean_const - (mu ? double(mu[G ? src : base + lane]) : 0.0)) : T(0);
  double F = P.variance + sigi, r = double(y[i]) - P.mean_const - (mu ? double(mu[i]) : 0.0);
  // "not positive": at or below the rounding noise of its own computation, 4 eps (m + 1) (variance + the largest sigma^2 of the block)
  const double floor_ = 4.0 * (sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07) * double(m + 1) * (P.variance + smax);
  bool isbad = false;
  T myrs = T(1), lme = T(0), zme = T(0);   // lane p keeps 1 / L[p][p], l_p, z_p
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
  if (!(F > floor_)) isbad = true;
  if (lane == 0) {
    double* t = terms + i * S;
    t[0] = isbad ? 0.0 : log(F);
    t[1] = isbad ? 0.0 : r * r / F;
    t[2] = (F <= 0.0) ? 1.0 : 0.0;
    if (isbad) atomicMin(bad, int(i + 1 < kNnNone ? i + 1 : kNnNone - 1));
  }
  if (MODE == 0) return;
  // b = L^-T l, w = L^-T z: L[p][j], j < p, is lane j's frozen register p times its own 1 / L[j][j]
  T tb = lme, tw = zme, bme = T(0), wme = T(0);
  nn_static_for<0, KB>([&](auto pc) __attribute__((always_inline)) {
    constexpr int p = KB - 1 - decltype(pc)::value;
    if (p < m) {
      const T rsp = nn_rl(myrs, p);
      const T bp = nn_rl(tb, p) * rsp, wp = nn_rl(tw, p) * rsp;
      if (lane == p) { bme = bp; wme = wp; }
      const T lpj = lane < p ? A[p] * myrs : T(0);
      tb = fma(-lpj, bp, tb);
      tw = fma(-lpj, wp, tw);
    }
  });
  const double rF = r / F;
  if (MODE == 1 || MODE == 3) {
    if (act) Bd[i + int64_t(G ? lane : P.k - m + lane) * P.n] = bme;
    if (lane == 0) { Fd[i] = F; rFd[i] = rF; }
    if (MODE == 1) return;
  }
  // ---- gradient ----
  const double gF = -0.5 / F + 0.5 * r * r / (F * F);
  const double btb = nn_wave_sum(double(bme) * double(bme)), wtb = nn_wave_sum(double(wme) * double(bme));
  const T qv = T(gF * double(bme) - rF * double(wme));               // C_bar[q][j] = qv_q b_j
  const T cb = T(-2.0 * gF * double(bme) + rF * double(wme));        // c_bar_j
  // the diagonal of C_bar: d lml / d sigma_j^2 of this block, and its contraction with the block's variances for d / d variance
  const double qd = (gF * double(bme) - rF * double(wme)) * double(bme);
  const double sq = sv ? nn_wave_sum(act ? double(sig) * qd : 0.0) : 0.0;
  if (MODE == 3) {
    if (act) Qd[i + int64_t(G ? lane : P.k - m + lane) * P.n] = T(qd);
    if (lane == 0) gFd[i] = gF;
  }
  T cr2;
  nn_dist2<T, KB, G>(P, x, base, i, lane, m, A, cr2, src);
  const T v2 = T(2) * variance;
#pragma unroll
  for (int g = 0; g < KB / 8; ++g) {
    if (g * 8 < m) {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = (act && q < m) ? v2 * nn_dkappa(P.family, A[q]) * nn_rl(qv, q) * bme : T(0);
    } else {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = T(0);
    }
  }
  const T gc = act ? v2 * nn_dkappa(P.family, cr2) * cb : T(0);
  double* t = terms + i * S;
  for (int f = 0; f < P.d; ++f) {
    const T il = T(P.invl[f]);
    const T xj = act ? x[int64_t(f) * P.ldx + (G ? src : base + lane)] * il : T(0);
    const T dc = xj - x[int64_t(f) * P.ldx + i] * il;
    T acc = gc * dc * dc;
#pragma unroll
    for (int g = 0; g < KB / 8; ++g)
      if (g * 8 < m) {
#pragma unroll
        for (int q = g * 8; q < g * 8 + 8; ++q) {
          const T df = nn_rl(xj, q) - xj;
          acc = fma(A[q], df * df, acc);
        }
      }
    const double sum = nn_wave_sum(double(acc));   // sum P_ab dk 2 variance (ds_f)^2 = invl_f * d / d invl_f
    if (lane == 0) t[kNnGradSlots + f] = (isbad || P.invl[f] == 0.0) ? 0.0 : sum / P.invl[f];
  }
  if (lane == 0) {
    const double tr = gF * btb - rF * wtb;   // trace of C_bar
    // variance d / d variance + sum_j sigma_j^2 d / d sigma_j^2 = gF F over the block (scaling both scales F, r stays)
    if (sv) t[3] = isbad ? 0.0 : (gF * (F - sigi) - sq) / P.variance;
    else t[3] = isbad ? 0.0 : (gF * (F - P.diag) - P.diag * tr) / P.variance;
    t[4] = isbad ? 0.0 : gF + tr;
  }
}

template <typename T, int KB, int MODE, bool G>
__global__ void __launch_bounds__(k256) nn_point_v_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ y,
                                                          const T* __restrict__ sv, const T* __restrict__ mu, double* __restrict__ terms,
                                                          int S, int* __restrict__ bad, T* __restrict__ Bd, double* __restrict__ Fd,
                                                          double* __restrict__ rFd, T* __restrict__ Qd, double* __restrict__ gFd,
                                                          const int* __restrict__ nbr) {
  nn_point_body_v<T, KB, MODE, G>(P, x, y, sv, mu, terms, S, bad, Bd, Fd, rFd, Qd, gFd, nbr);
}

// nn.hip's nn_block with the lane's own sigma^2 on the diagonal
template <typename T, int KB>
__device__ __forceinline__ void nn_block_v(const NnParams& P, int lane, int m, T sig, T (&A)[KB], T& c) {
  const bool act = lane < m;
  const T variance = T(P.variance);
#pragma unroll
  for (int g = 0; g < KB / 8; ++g) {
    if (g * 8 < m) {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) {
        const T kv = kappa(P.family, A[q], variance) + (q == lane ? sig : T(0));
        A[q] = (act && q < m) ? kv : (q == lane ? T(1) : T(0));
      }
    } else {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = q == lane ? T(1) : T(0);
    }
  }
  c = act ? kappa(P.family, c, variance) : T(0);
}

// nn.hip's nn_local_kernel conditioned on the two vectors: C = k(ns*, ns*) + diag(sigma^2_ns*), delta_ns* = y - mean_const - mu.
// The pivot floor is 4 eps (m + 1) (variance + the largest sigma^2 of the block).
template <typename T, int KB>
__global__ void __launch_bounds__(k256) nn_local_v_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ y,
                                                          const T* __restrict__ sv, const T* __restrict__ mu, const T* __restrict__ xq,
                                                          int64_t ldq, int64_t nq, int64_t q0, const int* __restrict__ nbr,
                                                          int* __restrict__ bad, T* __restrict__ mean, T* __restrict__ var) {
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  if (i >= nq) return;
  bool qnan = false;
  for (int f = lane; f < P.d; f += 64) qnan = qnan || !isfinite(double(xq[int64_t(f) * ldq + i]));
  if (__ballot(qnan) != 0) {
    if (lane == 0) {
      if (mean) mean[i] = T(NAN);
      if (var) var[i] = T(NAN);
    }
    return;
  }
  const int e = lane < P.k ? nbr[i + int64_t(lane) * nq] : -1;
  const int m = __builtin_amdgcn_readfirstlane(__popcll(__ballot(e >= 0)));
  const bool act = lane < m;
  const T sig = T(P.diag) + ((sv && act) ? sv[e] : T(0));
  double smax = act ? double(sig) : P.diag;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) smax = fmax(smax, __shfl_xor(smax, o));
  T A[KB], c;
  nn_dist2_query<T, KB>(P, x, xq, ldq, i, lane, m, A, c, e);
  nn_block_v<T, KB>(P, lane, m, sig, A, c);
  T dd = act ? T(double(y[e]) - P.mean_const - (mu ? double(mu[e]) : 0.0)) : T(0);
  double F = P.variance, r = 0.0;
  const double floor_ = 4.0 * (sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07) * double(m + 1) * (P.variance + smax);
  T myrs = T(1), lme = T(0), zme = T(0);
  const bool isbad = nn_factor<T, KB>(lane, m, floor_, A, c, dd, F, r, myrs, lme, zme);
  if (lane == 0) {
    if (mean) mean[i] = isbad ? T(NAN) : T(P.mean_const - r);
    if (var) var[i] = isbad ? T(NAN) : T(F);
    if (isbad) atomicMin(bad, int(q0 + i + 1 < kNnNone ? q0 + i + 1 : kNnNone - 1));
  }
}

// s_bar_j = gF_j + sum_{s = 1 .. kb, j + s < n} Q(j + s, kb - s): the window, nn_alpha_kernel's gather
template <typename T>
__global__ void nn_sbar_kernel(const T* __restrict__ Qd, const double* __restrict__ gF, int64_t n, int kb, double* __restrict__ sbar) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double a = gF[j];
  for (int s = 1; s <= kb && j + s < n; ++s) a += double(Qd[(j + s) + int64_t(kb - s) * n]);
  sbar[j] = a;
}
// ... over the reverse list of j: one wavefront per j, the lanes stride the list and a fixed tree adds them (nn_alpha_tab_kernel's)
template <typename T>
__global__ void __launch_bounds__(k256) nn_sbar_tab_kernel(const T* __restrict__ Qd, const double* __restrict__ gF, int64_t n,
                                                           const int64_t* __restrict__ off, const int64_t* __restrict__ rv,
                                                           double* __restrict__ sbar) {
  const int lane = threadIdx.x & 63;
  const int64_t j = int64_t(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  if (j >= n) return;
  double a = 0.0;
  for (int64_t p = off[j] + lane; p < off[j + 1]; p += 64) a += double(Qd[rv[p]]);
  a = nn_wave_sum(a);
  if (lane == 0) sbar[j] = gF[j] + a;
}

template <typename T, int MODE>
void nn_launch_point_v(hipStream_t s, const NnParams& P, const NnPointArgs& a) {
  const dim3 grid(unsigned((P.n + 3) / 4)), block(k256);
  const T *x = (const T*)a.x, *y = (const T*)a.y, *sv = (const T*)a.sv, *mu = (const T*)a.mu;
  T *Bd = (T*)a.Bd, *Qd = (T*)a.Qd;
#define NN_PV(KB, G) \
  hipLaunchKernelGGL((nn_point_v_kernel<T, KB, MODE, G>), grid, block, 0, s, P, x, y, sv, mu, a.terms, a.S, a.bad, Bd, a.Fd, a.rF, Qd, a.gF, a.nbr)
  if (a.nbr) {
    if (P.k <= 16) NN_PV(16, true);
    else if (P.k <= 32) NN_PV(32, true);
    else NN_PV(64, true);
  } else {
    if (P.k <= 16) NN_PV(16, false);
    else if (P.k <= 32) NN_PV(32, false);
    else NN_PV(64, false);
  }
#undef NN_PV
}

template <typename T>
void nn_launch_point_v_mode(int mode, hipStream_t s, const NnParams& P, const NnPointArgs& a) {
  if (mode == 0) nn_launch_point_v<T, 0>(s, P, a);
  else if (mode == 1) nn_launch_point_v<T, 1>(s, P, a);
  else if (mode == 2) nn_launch_point_v<T, 2>(s, P, a);
  else nn_launch_point_v<T, 3>(s, P, a);
}

template <typename T>
void nn_launch_local_v(hipStream_t s, const NnParams& P, const void* x, const void* y, const void* sv, const void* mu, const void* xq,
                       int64_t ldq, int64_t nq, int64_t q0, const int* nbr, int* bad, void* mean, void* var) {
  const dim3 grid(unsigned((nq + 3) / 4)), block(k256);
#define NN_LV(KB)                                                                                                                       \
  hipLaunchKernelGGL((nn_local_v_kernel<T, KB>), grid, block, 0, s, P, (const T*)x, (const T*)y, (const T*)sv, (const T*)mu, (const T*)xq, \
                     ldq, nq, q0, nbr, bad, (T*)mean, (T*)var)
  if (P.k <= 16) NN_LV(16);
  else if (P.k <= 32) NN_LV(32);
  else NN_LV(64);
#undef NN_LV
}

template <typename T>
void nn_launch_sbar(hipStream_t s, const void* Qd, const double* gF, int64_t n, int kb, const int64_t* off, const int64_t* rv, double* sbar) {
  if (off) hipLaunchKernelGGL(nn_sbar_tab_kernel<T>, dim3(unsigned((n + 3) / 4)), dim3(k256), 0, s, (const T*)Qd, gF, n, off, rv, sbar);
  else hipLaunchKernelGGL(nn_sbar_kernel<T>, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, (const T*)Qd, gF, n, kb, sbar);
}

}  // namespace

void launch_nn_point_v(int dtype, int mode, hipStream_t s, const NnParams& P, const NnPointArgs& a) {
  if (dtype == 0) nn_launch_point_v_mode<double>(mode, s, P, a);
  else nn_launch_point_v_mode<float>(mode, s, P, a);
}

void launch_nn_local_v(int dtype, hipStream_t s, const NnParams& P, const void* x, const void* y, const void* sv, const void* mu,
                       const void* xq, int64_t ldq, int64_t nq, int64_t q0, const int* nbr, int* bad, void* mean, void* var) {
  if (dtype == 0) nn_launch_local_v<double>(s, P, x, y, sv, mu, xq, ldq, nq, q0, nbr, bad, mean, var);
  else nn_launch_local_v<float>(s, P, x, y, sv, mu, xq, ldq, nq, q0, nbr, bad, mean, var);
}

void launch_nn_sbar(int dtype, hipStream_t s, const void* Qd, const double* gF, int64_t n, int kb, const int64_t* off, const int64_t* rv,
                    double* sbar) {
  if (dtype == 0) nn_launch_sbar<double>(s, Qd, gF, n, kb, off, rv, sbar);
  else nn_launch_sbar<float>(s, Qd, gF, n, kb, off, rv, sbar);
}

}  // namespace svgp
