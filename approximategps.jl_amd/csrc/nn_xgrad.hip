// nn_xgrad.hip — the NearestNeighbors gradient of the log marginal likelihood with respect to the data inputs x
// (svgp_nn_lml_grad_inputs), at the fixed conditioning sets.  With s = invl .* x, L_i = -1/2 (log F_i + r_i^2 / F_i), g = d kappa / d r2 of
// the unit-variance kernel and b, w, F, r, gF, qv = gF b - (r / F) w, c_bar = -2 gF b + (r / F) w as in nn_points.hip:
//   W_ab = 2 variance g(r2_ab) (qv_a b_b + qv_b b_a)   a, b in ns(i)   (C_bar = qv b' symmetrised: it meets a symmetric d K)
//   W_ai = 2 variance g(r2_ai) c_bar_a
//   d L_i / d s_{a, f} =  sum_b W_ab (s_a - s_b)_f + W_ai (s_a - s_i)_f      a in ns(i)    -> Xd[f][t][i], ns(i)_t = a
//   d L_i / d s_{i, f} = -sum_a W_ai (s_a - s_i)_f                                         -> Hd[f][i]
//   x_bar[f, j] = invl_f (Hd[f][j] + the sum of Xd[f] over the pairs (i, t) that name j)
// Summed over j, x_bar[f, :] is 0 (translation) and x[f, :] . x_bar[f, :] is invl_f d lml / d invl_f (scaling), block by block.
//   point kernel   nn_point_body_v's mode 3 line for line up to the second nn_dist2: the same slots, Bd, Fd, rF, Qd, gF, floor and bad
//                  word, so the scalars, mean_bar and s_bar of the call are those of svgp_nn_lml_grad_points bit for bit.  A sibling in
//                  a unit of its own, for the reason written at the top of nn_points.hip.  After the second nn_dist2 the register array
//                  keeps G[q] = 2 variance g(r2_qj) alone; the two weights of a pair are formed where they are used, from readlanes of
//                  qv and b: P = (G qv_q) b_j, the product mode 3 stores (the inverse-lengthscale slots stay its bits), and
//                  W = P + (G b_q) qv_j.  No second register array.  In fp32 two coordinates go through the block together and share P and W.
//                  The coordinate differences are taken per entry before any product, as everywhere in this tree.
//   gathers        one thread per (j, f) over the <= kb later rows of the window, or one wavefront per (j, f) over the reverse list of a
//                  table with a fixed tree: fp64, a fixed order, no atomics, one rounding to the data dtype into the caller's memory.
#include <hip/hip_runtime.h>

#include "nn_xgrad.hpp"

namespace svgp {
namespace {

// kappa() of device_common.hpp.  This unit is built without packed fp32 arithmetic, and without it the compiler contracts the fp32
// Matern-5/2 polynomial 1 + s + 5/3 r2 into two fmas where nn_points.hip's build multiplies (one packed multiply of r2 and r) and
// then adds.  The block must be mode 3's bit for bit, so that one polynomial is written here as the products and sums it is there
template <typename T>
__device__ __forceinline__ T nn_kappa_x(int family, T r2, T variance) {
  if (sizeof(T) == 8 || family != KM52) return kappa(family, r2, variance);
  float s = float(T(2.2360679774997896964) * ksqrt(r2)), t = float(T(5.0 / 3.0) * r2);
  asm volatile("" : "+v"(s), "+v"(t));   // the two rounded products in registers: nothing to contract with the sums
  return variance * ((T(1) + T(s)) + T(t)) * kexp(-T(s));
}

template <typename T, int KB, bool G>
__global__ void __launch_bounds__(k256) nn_point_x_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ y,
                                                          const T* __restrict__ sv, const T* __restrict__ mu, double* __restrict__ terms,
                                                          int S, int* __restrict__ bad, T* __restrict__ Bd, double* __restrict__ Fd,
                                                          double* __restrict__ rFd, T* __restrict__ Qd, double* __restrict__ gFd,
                                                          const int* __restrict__ nbr, T* __restrict__ Xd, double* __restrict__ Hd) {
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
        const T kv = nn_kappa_x(P.family, A[q], variance) + (q == lane ? sig : T(0));
        A[q] = (act && q < m) ? kv : (q == lane ? T(1) : T(0));
      }
    } else {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = q == lane ? T(1) : T(0);
    }
  }
  c = act ? nn_kappa_x(P.family, c, variance) : T(0);
  T dd = act ? T(double(y[G ? src : base + lane]) - P.mean_const - (mu ? double(mu[G ? src : base + lane]) : 0.0)) : T(0);
  double F = P.variance + sigi, r = double(y[i]) - P.mean_const - (mu ? double(mu[i]) : 0.0);
  // "not positive": at or below the rounding noise of its own computation, 4 eps (m + 1) (variance + the largest sigma^2 of the block)
  const double floor_ = 4.0 * (sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07) * double(m + 1) * (P.variance + smax);
  T myrs = T(1), lme = T(0), zme = T(0);   // lane p keeps 1 / L[p][p], l_p, z_p
  bool isbad = nn_factor<T, KB>(lane, m, floor_, A, c, dd, F, r, myrs, lme, zme);
  if (!(F > floor_)) isbad = true;
  double* t = terms + i * S;
  if (lane == 0) {
    t[0] = isbad ? 0.0 : log(F);
    t[1] = isbad ? 0.0 : r * r / F;
    t[2] = (F <= 0.0) ? 1.0 : 0.0;
    if (isbad) atomicMin(bad, int(i + 1 < kNnNone ? i + 1 : kNnNone - 1));
  }
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
  const int64_t slot = G ? lane : P.k - m + lane;   // the pair's column of Bd, Qd and of every coordinate of Xd
  if (act) Bd[i + slot * P.n] = bme;
  if (lane == 0) { Fd[i] = F; rFd[i] = rF; }
  // ---- gradient ----
  const double gF = -0.5 / F + 0.5 * r * r / (F * F);
  const double btb = nn_wave_sum(double(bme) * double(bme)), wtb = nn_wave_sum(double(wme) * double(bme));
  const T qv = T(gF * double(bme) - rF * double(wme));               // C_bar[q][j] = qv_q b_j
  const T cb = T(-2.0 * gF * double(bme) + rF * double(wme));        // c_bar_j
  // the diagonal of C_bar: d lml / d sigma_j^2 of this block, and its contraction with the block's variances for d / d variance
  const double qd = (gF * double(bme) - rF * double(wme)) * double(bme);
  const double sq = sv ? nn_wave_sum(act ? double(sig) * qd : 0.0) : 0.0;
  if (act) Qd[i + slot * P.n] = T(qd);
  if (lane == 0) gFd[i] = gF;
  T cr2;
  nn_dist2<T, KB, G>(P, x, base, i, lane, m, A, cr2, src);
  const T v2 = T(2) * variance;
#pragma unroll
  for (int g = 0; g < KB / 8; ++g) {
    if (g * 8 < m) {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = (act && q < m) ? v2 * nn_dkappa(P.family, A[q]) : T(0);   // G[q]
    } else {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = T(0);
    }
  }
  const T gc = act ? v2 * nn_dkappa(P.family, cr2) * cb : T(0);   // W_ji
  const int64_t cs = int64_t(P.k) * P.n;                          // one coordinate of Xd
  constexpr int FB = sizeof(T) == 8 ? 1 : 2;                      // coordinates that go through the block together
  for (int f0 = 0; f0 < P.d; f0 += FB) {
    T xj[FB], hc[FB], acc[FB], xa[FB];
#pragma unroll
    for (int u = 0; u < FB; ++u) {
      const int f = f0 + u < P.d ? f0 + u : P.d - 1;   // (past the last coordinate: the last once more, not stored)
      const T il = T(P.invl[f]);
      xj[u] = act ? x[int64_t(f) * P.ldx + (G ? src : base + lane)] * il : T(0);
      const T dc = xj[u] - x[int64_t(f) * P.ldx + i] * il;
      hc[u] = gc * dc;   // W_ji (s_j - s_i)_f
      acc[u] = hc[u] * dc;
      xa[u] = T(0);      // sum_q W_qj (s_q - s_j)_f
    }
#pragma unroll
    for (int g = 0; g < KB / 8; ++g)
      if (g * 8 < m) {
#pragma unroll
        for (int q = g * 8; q < g * 8 + 8; ++q) {
          const T pq = A[q] * nn_rl(qv, q) * bme;
          const T wq = fma(A[q] * nn_rl(bme, q), qv, pq);
#pragma unroll
          for (int u = 0; u < FB; ++u) {
            const T df = nn_rl(xj[u], q) - xj[u];
            acc[u] = fma(pq, df * df, acc[u]);
            xa[u] = fma(wq, df, xa[u]);
          }
        }
      }
#pragma unroll
    for (int u = 0; u < FB; ++u) {
      const int f = f0 + u;
      if (f < P.d) {
        const double sum = nn_wave_sum(double(acc[u]));   // sum P_ab dk 2 variance (ds_f)^2 = invl_f * d / d invl_f
        const double own = nn_wave_sum(double(hc[u]));
        if (act) Xd[int64_t(f) * cs + i + slot * P.n] = hc[u] - xa[u];
        if (lane == 0) {
          t[kNnGradSlots + f] = (isbad || P.invl[f] == 0.0) ? 0.0 : sum / P.invl[f];
          Hd[int64_t(f) * P.n + i] = -own;
        }
      }
    }
  }
  if (lane == 0) {
    const double tr = gF * btb - rF * wtb;   // trace of C_bar
    // variance d / d variance + sum_j sigma_j^2 d / d sigma_j^2 = gF F over the block (scaling both scales F, r stays)
    if (sv) t[3] = isbad ? 0.0 : (gF * (F - sigi) - sq) / P.variance;
    else t[3] = isbad ? 0.0 : (gF * (F - P.diag) - P.diag * tr) / P.variance;
    t[4] = isbad ? 0.0 : gF + tr;
  }
}

// x_bar[f, j] = invl_f (Hd[f][j] + sum_{s = 1 .. kb, j + s < n} Xd[f](j + s, kb - s)): the window, nn_sbar_kernel's gather per coordinate
template <typename T>
__global__ void nn_xbar_kernel(const NnParams P, const T* __restrict__ Xd, const double* __restrict__ Hd, T* __restrict__ out, int64_t ldo) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int f = blockIdx.y;
  if (j >= P.n) return;
  const T* X = Xd + int64_t(f) * P.k * P.n;
  double a = 0.0;
  for (int s = 1; s <= P.k && j + s < P.n; ++s) a += double(X[(j + s) + int64_t(P.k - s) * P.n]);
  out[int64_t(f) * ldo + j] = T(P.invl[f] * (Hd[int64_t(f) * P.n + j] + a));
}
// ... over the reverse list of j: one wavefront per (j, f), the lanes stride the list and a fixed tree adds them (nn_sbar_tab_kernel's)
template <typename T>
__global__ void __launch_bounds__(k256) nn_xbar_tab_kernel(const NnParams P, const T* __restrict__ Xd, const double* __restrict__ Hd,
                                                           const int64_t* __restrict__ off, const int64_t* __restrict__ rv,
                                                           T* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63;
  const int64_t j = int64_t(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int f = blockIdx.y;
  if (j >= P.n) return;
  const T* X = Xd + int64_t(f) * P.k * P.n;
  double a = 0.0;
  for (int64_t p = off[j] + lane; p < off[j + 1]; p += 64) a += double(X[rv[p]]);
  a = nn_wave_sum(a);
  if (lane == 0) out[int64_t(f) * ldo + j] = T(P.invl[f] * (Hd[int64_t(f) * P.n + j] + a));
}

template <typename T>
__global__ void nn_xfill_kernel(int64_t n, T v, T* __restrict__ out, int64_t ldo) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < n) out[int64_t(blockIdx.y) * ldo + j] = v;
}

template <typename T>
void nn_launch_point_x(hipStream_t s, const NnParams& P, const NnPointArgs& a, void* Xd, double* Hd) {
  const dim3 grid(unsigned((P.n + 3) / 4)), block(k256);
  const T *x = (const T*)a.x, *y = (const T*)a.y, *sv = (const T*)a.sv, *mu = (const T*)a.mu;
#define NN_PX(KB, G)                                                                                                                        \
  hipLaunchKernelGGL((nn_point_x_kernel<T, KB, G>), grid, block, 0, s, P, x, y, sv, mu, a.terms, a.S, a.bad, (T*)a.Bd, a.Fd, a.rF, (T*)a.Qd, \
                     a.gF, a.nbr, (T*)Xd, Hd)
  if (a.nbr) {
    if (P.k <= 16) NN_PX(16, true);
    else if (P.k <= 32) NN_PX(32, true);
    else NN_PX(64, true);
  } else {
    if (P.k <= 16) NN_PX(16, false);
    else if (P.k <= 32) NN_PX(32, false);
    else NN_PX(64, false);
  }
#undef NN_PX
}

template <typename T>
void nn_launch_xbar(hipStream_t s, const NnParams& P, const void* Xd, const double* Hd, const int64_t* off, const int64_t* rv, void* out,
                    int64_t ldo) {
  if (off)
    hipLaunchKernelGGL(nn_xbar_tab_kernel<T>, dim3(unsigned((P.n + 3) / 4), unsigned(P.d)), dim3(k256), 0, s, P, (const T*)Xd, Hd, off, rv,
                       (T*)out, ldo);
  else
    hipLaunchKernelGGL(nn_xbar_kernel<T>, dim3(unsigned((P.n + 255) / 256), unsigned(P.d)), dim3(256), 0, s, P, (const T*)Xd, Hd, (T*)out, ldo);
}

}  // namespace

void launch_nn_point_x(int dtype, hipStream_t s, const NnParams& P, const NnPointArgs& a, void* Xd, double* Hd) {
  if (dtype == 0) nn_launch_point_x<double>(s, P, a, Xd, Hd);
  else nn_launch_point_x<float>(s, P, a, Xd, Hd);
}

void launch_nn_xbar(int dtype, hipStream_t s, const NnParams& P, const void* Xd, const double* Hd, const int64_t* off, const int64_t* rv,
                    void* out, int64_t ldo) {
  if (dtype == 0) nn_launch_xbar<double>(s, P, Xd, Hd, off, rv, out, ldo);
  else nn_launch_xbar<float>(s, P, Xd, Hd, off, rv, out, ldo);
}

void launch_nn_xfill(int dtype, hipStream_t s, int64_t n, int d, double v, void* out, int64_t ldo) {
  const dim3 grid(unsigned((n + 255) / 256), unsigned(d));
  if (dtype == 0) hipLaunchKernelGGL(nn_xfill_kernel<double>, grid, dim3(256), 0, s, n, v, (double*)out, ldo);
  else hipLaunchKernelGGL(nn_xfill_kernel<float>, grid, dim3(256), 0, s, n, float(v), (float*)out, ldo);
}

}  // namespace svgp
