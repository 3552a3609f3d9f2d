// nn.hip — the NearestNeighbors (Vecchia) approximation (reference src/NearestNeighborsModule.jl):
//   posterior(nn, fx, y) :97-106      approx_lml(nn, fx, y) :108-113      make_row :27-29      make_F :46-61
// The prior factors as p(f) = prod_i p(f_i | f_ns(i)), ns(i) = the m = min(i, k) points before i in the given order.  Per point:
//   C = k(ns, ns) + diag I,  c = k(ns, x_i),  kd = k(x_i, x_i) + diag,  b_i = C \ c,  F_i = kd - c' b_i,  r_i = delta_i - b_i' delta_ns
//   approx_lml = -1/2 sum_i (log 2 pi + log F_i + r_i^2 / F_i)
// The reference packs the b_i into a sparse B and U = (I - B)' F^-1/2; nothing here is sparse or sequential: one dense solve of
// order <= k per point, N of them independent.
//   point kernel     one wavefront per point, lane j owns COLUMN j of the <= 64 x 64 block in registers (A[q] = C[q][j]).  The block
//                    is symmetric, so at step p of the right-looking factorisation lane j finds C[j][p] in its own register p,
//                    and the other factor of the update, L[q][p], is lane q's value: a v_readlane into scalar registers, uniform
//                    over the wave.  No LDS, no barrier.  c and delta_ns ride along as two more rows of the block (one register
//                    each), so l = L^-1 c, z = L^-1 delta_ns, F = kd - l'l and r = delta_i - l'z come out of the same sweep (F and r
//                    in fp64 for both dtypes: kd - l'l cancels).  Lanes below the pivot keep their column of the Schur complement
//                    frozen: scaled by their pivot it is the column of L the back-substitutions b = L^-T l, w = L^-T z read.
//                    Templated on the k bucket (16 / 32 / 64 registers) and the mode (value / fit / gradient).          nn_point_kernel
//   reduction        per-point slots -> per-block partials -> one block per slot, fixed order, no atomics             nn_reduce*_kernel
//   gradient         gF = -1/(2F) + r^2/(2F^2), qv = gF b - (r/F) w:  C_bar = qv b' (the unsymmetrised form: it only meets symmetric
//                    dK), c_bar = -2 gF b + (r/F) w; the inverse lengthscales contract them with dk/dr2 * 2 (ds_f)^2 / invl_f over a
//                    regenerated block; d/d variance and d/d diag have closed forms in (F, b'b, w'b) (nn_point_kernel, MODE 2)
//   fit              the same sweep stores b_i (banded N x kb column-major, data dtype), F_i and r_i / F_i; alpha = U (U' delta) is
//                    a gather over the <= k later rows                                                                  nn_alpha_kernel
//   predictions      V = U' k(x, x*) streamed in row tiles of at most 2048 points, never N x n*: k(x, x*) tile (nn_kx_kernel),
//                    V tile with the column sums of the mean and of V.^2 (nn_v_kernel), V'V on the MFMA product kernel of the
//                    gradient path (launch_gemm_pm) accumulated tile after tile in stream order
//   local predictions   nearest-neighbour kriging: per test point the min(k, N) nearest training points (nn_query_search_kernel: one
//                    wavefront per query, 16 per workgroup, double-buffered 64-wide LDS tiles), then the point kernel's sweep over the
//                    gathered block with the query read from the test array (nn_local_kernel); rounds of 32768 test points
//   per-point vectors   svgp_nn_set_noise / svgp_nn_set_mean keep N noise variances s and N mean offsets mu on the handle: C carries
//                    diag(T(diag) + s), delta = y - mean_const - mu.  With either set, and in svgp_nn_lml_grad_points (s_bar, mean_bar =
//                    alpha), the point and local kernels are the siblings of nn_points.hip; without, the ones below, untouched
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "ctx.hpp"
#include "device_common.hpp"
#include "kernels.hpp"
#include "nn_common.hpp"
#include "nn_points.hpp"

namespace svgp {
namespace {

#define NN_DISPATCH(dtype, T, ...)      \
  do {                                  \
    if ((dtype) == 0) {                 \
      using T = double;                 \
      __VA_ARGS__;                      \
    } else {                            \
      using T = float;                  \
      __VA_ARGS__;                      \
    }                                   \
  } while (0)

constexpr int kNnMaxK = 64;        // one lane per neighbour
constexpr int kNnSlots = 3;        // per point: log F, r^2 / F, (F <= 0)
constexpr int kNnRows = 2048;      // most rows of one V tile
constexpr int64_t kNnTileElems = int64_t(1) << 23;   // elements of one V tile (rows x padded columns): the workspace rule
constexpr int64_t kNnMaxCov = 4096;                  // most test points of cov / cross-cov
constexpr int64_t kNnMaxPred = int64_t(1) << 17;     // most test points of one mean / var call (64-row tiles at the workspace rule)
constexpr int64_t kNnLocalChunk = int64_t(1) << 15;  // test points of one round of svgp_nn_predict_local: its whole workspace

// MODE 0: the lml slots.  MODE 1: + b_i, F_i, r_i / F_i (fit).  MODE 2: + the gradient slots.
// G (gathered): lane t conditions on point nbr(i, t) of the neighbour table (N x P.k column-major, the valid entries first, -1 after
// them) instead of point i - m + t of the window; everything after the loads is the same arithmetic in the same order.
template <typename T, int KB, int MODE, bool G>
__device__ __forceinline__ void nn_point_body(const NnParams& P, const T* __restrict__ x, const T* __restrict__ y,
                                              double* __restrict__ terms, int S, int* __restrict__ bad, T* __restrict__ Bd,
                                              double* __restrict__ Fd, double* __restrict__ rFd, const int* __restrict__ nbr) {
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
  T A[KB], c;
  nn_dist2<T, KB, G>(P, x, base, i, lane, m, A, c, src);
  // the block: C on the m x m corner, identity on the padding
#pragma unroll
  for (int g = 0; g < KB / 8; ++g) {
    if (g * 8 < m) {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) {
        const T kv = kappa(P.family, A[q], variance) + (q == lane ? T(P.diag) : T(0));
        A[q] = (act && q < m) ? kv : (q == lane ? T(1) : T(0));
      }
    } else {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = q == lane ? T(1) : T(0);
    }
  }
  c = act ? kappa(P.family, c, variance) : T(0);
  T dd = act ? T(double(y[G ? src : base + lane]) - P.mean_const) : T(0);
  double F = P.variance + P.diag, r = double(y[i]) - P.mean_const;
  // "not positive": at or below the rounding noise of its own computation, 4 eps (m + 1) kd - a pivot or an F down there is a
  // difference of equal numbers (an exactly repeated point with diag = 0 leaves +-1e-16, either sign)
  const double floor_ = 4.0 * (sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07) * double(m + 1) * F;
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
  if (MODE == 1) {
    if (act) Bd[i + int64_t(G ? lane : P.k - m + lane) * P.n] = bme;
    if (lane == 0) { Fd[i] = F; rFd[i] = rF; }
    return;
  }
  // ---- gradient ----
  const double gF = -0.5 / F + 0.5 * r * r / (F * F);
  const double btb = nn_wave_sum(double(bme) * double(bme)), wtb = nn_wave_sum(double(wme) * double(bme));
  const T qv = T(gF * double(bme) - rF * double(wme));               // C_bar[q][j] = qv_q b_j
  const T cb = T(-2.0 * gF * double(bme) + rF * double(wme));        // c_bar_j
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
    t[3] = isbad ? 0.0 : (gF * (F - P.diag) - P.diag * tr) / P.variance;
    t[4] = isbad ? 0.0 : gF + tr;
  }
}
// ---- the sweep of a local prediction: nn_point_body's distances, block and factorisation with the query read from a second array.
// A sibling, not a shared body: with the three pieces below factored out of nn_point_body its instantiations did not keep their
// register counts (f64 KB = 16 value 74 -> 84 VGPRs, 6 -> 5 waves per SIMD; the fp32 ones moved by up to 110), so nn_point_body stays
// as it was, and the arithmetic and its order are repeated line for line (nn_dist2_query and nn_factor in nn_common.hpp, nn_block here).
// The same rule made the point kernels with per-point noise variances and mean offsets a second sibling, in nn_points.hip.
// The block from its squared distances: C = k(ns, ns) + diag I on the m x m corner, identity on the padding; c = k(ns, x_i)
template <typename T, int KB>
__device__ __forceinline__ void nn_block(const NnParams& P, int lane, int m, T (&A)[KB], T& c) {
  const bool act = lane < m;
  const T variance = T(P.variance);
#pragma unroll
  for (int g = 0; g < KB / 8; ++g) {
    if (g * 8 < m) {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) {
        const T kv = kappa(P.family, A[q], variance) + (q == lane ? T(P.diag) : T(0));
        A[q] = (act && q < m) ? kv : (q == lane ? T(1) : T(0));
      }
    } else {
#pragma unroll
      for (int q = g * 8; q < g * 8 + 8; ++q) A[q] = q == lane ? T(1) : T(0);
    }
  }
  c = act ? kappa(P.family, c, variance) : T(0);
}

template <typename T, int KB, int MODE>
__global__ void __launch_bounds__(k256) nn_point_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ y,
                                                        double* __restrict__ terms, int S, int* __restrict__ bad, T* __restrict__ Bd,
                                                        double* __restrict__ Fd, double* __restrict__ rFd) {
  nn_point_body<T, KB, MODE, false>(P, x, y, terms, S, bad, Bd, Fd, rFd, nullptr);
}
template <typename T, int KB, int MODE>
__global__ void __launch_bounds__(k256) nn_point_tab_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ y,
                                                            double* __restrict__ terms, int S, int* __restrict__ bad, T* __restrict__ Bd,
                                                            double* __restrict__ Fd, double* __restrict__ rFd,
                                                            const int* __restrict__ nbr) {
  nn_point_body<T, KB, MODE, true>(P, x, y, terms, S, bad, Bd, Fd, rFd, nbr);
}

// Local (nearest-neighbour kriging) prediction: query q (column q of xq, ld ldq) is conditioned on the points of row q of its own table
// (nq x P.k column-major, P.k = min(k, N), -1 after the valid entries); the block, its factorisation and the two riding rows are
// nn_point_body's (the sibling pieces above).  kd = k(x*, x*) carries no diag (the latent variance), so F starts from the variance and r from 0:
//   var = F = variance - l'l,   mean = mean_const + l'z = mean_const - r.
// Only a pivot is "not positive" here (floor: 4 eps (m + 1) of the block's diagonal, variance + diag); F is returned as computed.
// A query with a coordinate that is not finite gives NaN, and is no error.
template <typename T, int KB>
__global__ void __launch_bounds__(k256) nn_local_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ y,
                                                        const T* __restrict__ xq, int64_t ldq, int64_t nq, int64_t q0,
                                                        const int* __restrict__ nbr, int* __restrict__ bad, T* __restrict__ mean,
                                                        T* __restrict__ var) {
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
  T A[KB], c;
  nn_dist2_query<T, KB>(P, x, xq, ldq, i, lane, m, A, c, e);
  nn_block<T, KB>(P, lane, m, A, c);
  T dd = act ? T(double(y[e]) - P.mean_const) : T(0);
  double F = P.variance, r = 0.0;
  const double floor_ = 4.0 * (sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07) * double(m + 1) * (P.variance + P.diag);
  T myrs = T(1), lme = T(0), zme = T(0);
  const bool isbad = nn_factor<T, KB>(lane, m, floor_, A, c, dd, F, r, myrs, lme, zme);
  if (lane == 0) {
    if (mean) mean[i] = isbad ? T(NAN) : T(P.mean_const - r);
    if (var) var[i] = isbad ? T(NAN) : T(F);
    if (isbad) atomicMin(bad, int(q0 + i + 1 < kNnNone ? q0 + i + 1 : kNnNone - 1));
  }
}

// part[s][b] = sum of slot s over the points of block b (contiguous ranges of `chunk` points), fixed order
__global__ void __launch_bounds__(k256) nn_reduce1_kernel(const double* __restrict__ terms, int64_t n, int S, int64_t chunk,
                                                          double* __restrict__ part) {
  __shared__ double sh[k256];
  const int t = threadIdx.x, s = blockIdx.y;
  const int64_t i0 = int64_t(blockIdx.x) * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
  double acc = 0.0;
  for (int64_t i = i0 + t; i < i1; i += k256) acc += terms[i * S + s];
  sh[t] = acc;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  if (t == 0) part[int64_t(s) * gridDim.x + blockIdx.x] = sh[0];
}
__global__ void __launch_bounds__(k256) nn_reduce2_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double sh[k256];
  const int t = threadIdx.x, s = blockIdx.x;
  double acc = 0.0;
  for (int b = t; b < nb; b += k256) acc += part[int64_t(s) * nb + b];
  sh[t] = acc;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  if (t == 0) out[s] = sh[0];
}

// alpha = U (U' delta):  alpha_j = r_j / F_j - sum_{s = 1 .. kb, j + s < n} B(j + s, kb - s) r_{j+s} / F_{j+s}   (:103)
template <typename T>
__global__ void nn_alpha_kernel(const T* __restrict__ Bd, const double* __restrict__ rF, int64_t n, int kb, double* __restrict__ alpha) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double a = rF[j];
  for (int s = 1; s <= kb && j + s < n; ++s) a = fma(-double(Bd[(j + s) + int64_t(kb - s) * n]), rF[j + s], a);
  alpha[j] = a;
}

// ---- the neighbour table ---------------------------------------------------------------------------------------
// nbr is N x kb int32 column-major: row i lists the conditioning set of point i, its m_i <= min(i, kb) valid entries first (each in
// [0, i), distinct), -1 after them.

// One wavefront per row: flag = min(flag, i + 1) over the rows that break the rule above
__global__ void __launch_bounds__(k256) nn_check_tab_kernel(const int* __restrict__ nbr, int64_t n, int kb, int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  if (i >= n) return;
  const int e = lane < kb ? nbr[i + int64_t(lane) * n] : -1;
  const unsigned long long valid = __ballot(e >= 0);
  bool badl = e < -1 || int64_t(e) >= i;
  if ((valid & (valid + 1)) != 0) badl = true;   // a -1 before a valid entry
  for (int q = 0; q < kb; ++q) {
    const int v = __shfl(e, q);
    if (lane > q && e >= 0 && e == v) badl = true;
  }
  if (__ballot(badl) != 0 && lane == 0) atomicMin(flag, int(i + 1 < kNnNone ? i + 1 : kNnNone - 1));
}

// The current best of a search are kept one per lane (lane l < K: the l-th best so far), sorted by (distance, index).  Candidates
// arrive in ascending index (lane c of this tile is point j0 + c, `ok`: it is a candidate), so one beats the worst only with a
// strictly smaller distance, and it goes in behind every entry at most as far (a wave shift).  A distance that is not finite is
// never chosen.
template <typename T>
__device__ __forceinline__ void nn_best_insert(T r2, bool ok, int64_t j0, int K, int lane, T& bd, int& bi) {
  T worst = nn_rl(bd, K - 1);
  unsigned long long mask = __ballot(ok && r2 < worst);
  while (mask) {
    const int c = __builtin_ctzll(mask);
    mask &= mask - 1;
    const T dc = nn_rl(r2, c);
    if (!(dc < worst)) continue;   // the worst moved since the ballot
    const int pos = __popcll(__ballot(lane < K && bd <= dc));
    const T ud = __shfl_up(bd, 1);
    const int ui = __shfl_up(bi, 1);
    if (lane > pos) { bd = ud; bi = ui; }
    if (lane == pos) { bd = dc; bi = int(j0 + c); }
    worst = nn_rl(bd, K - 1);
  }
}
// Row i of a table (ld rows, kb columns) from the best K: ascending index - the rank of an entry is the number of smaller ones (the
// unfilled places hold INT_MAX and come last) - and -1 after them
__device__ __forceinline__ void nn_store_row(int* __restrict__ nbr, int64_t i, int64_t ld, int K, int kb, int lane, int bi) {
  const bool have = lane < K && bi != INT_MAX;
  int rank = 0;
  for (int q = 0; q < K; ++q) {
    const int v = __shfl(bi, q);
    rank += v < bi ? 1 : 0;
  }
  const int nv = __popcll(__ballot(have));
  if (have) nbr[i + int64_t(rank) * ld] = bi;
  if (lane >= nv && lane < kb) nbr[i + int64_t(lane) * ld] = -1;
}

// The exact k nearest predecessors: for query i the min(i, kb) points j < i with the smallest sum_f ((x_j,f - x_i,f) il_f)^2 (data
// dtype), ties to the lower index, stored in ascending index.  One wavefront per query, four queries per workgroup in descending i
// (block 0 holds the longest), candidates in 64-wide tiles shared through LDS.  A distance that is not finite is never chosen: that
// row comes out short.
template <typename T>
__global__ void __launch_bounds__(k256) nn_search_kernel(const NnParams P, const T* __restrict__ x, int* __restrict__ nbr) {
  extern __shared__ double nn_search_lds[];
  T* tile = reinterpret_cast<T*>(nn_search_lds);   // [d][64] candidates, then [4][d] queries
  T* qs = tile + int64_t(P.d) * 64;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t top = P.n - 1 - int64_t(blockIdx.x) * 4;   // the block's largest query
  const int64_t i = top - w;                               // may be negative in the last block
  const int K = i < P.k ? int(i < 0 ? 0 : i) : P.k;
  for (int e = threadIdx.x; e < 4 * P.d; e += k256) {
    const int qw = e / P.d, f = e - qw * P.d;
    qs[e] = top - qw >= 0 ? x[int64_t(f) * P.ldx + (top - qw)] : T(0);
  }
  T bd = T(INFINITY);   // lane l < K: the l-th best so far
  int bi = INT_MAX;
  for (int64_t j0 = 0; j0 < top; j0 += 64) {
    __syncthreads();   // the previous tile is consumed (first round: qs is written)
    for (int e = threadIdx.x; e < 64 * P.d; e += k256) {
      const int f = e >> 6, c = e & 63;
      tile[e] = j0 + c < top ? x[int64_t(f) * P.ldx + j0 + c] : T(0);
    }
    __syncthreads();
    if (j0 >= i) continue;   // wave-uniform: no candidate of this tile precedes the query
    T r2 = T(0);
    for (int f = 0; f < P.d; ++f) {
      const T df = (tile[f * 64 + lane] - qs[w * P.d + f]) * T(P.invl[f]);
      r2 = fma(df, df, r2);
    }
    nn_best_insert<T>(r2, j0 + lane < i, j0, K, lane, bd, bi);
  }
  if (i < 0) return;
  nn_store_row(nbr, i, P.n, K, P.k, lane, bi);
}

// The k nearest training points of a test point: for query q (column q of xq, ld ldq) the P.k = min(k, N) points j with the smallest
// sum_f ((x_j,f - x*_f) il_f)^2, by the rules above, as row q of an nq x P.k table.  Every query scans all N candidates, so the scans
// of a workgroup have one length and a tile serves every wavefront for all of its life: kNnQw = 16 queries per workgroup (one
// wavefront each), four times the reuse of a tile and a quarter of the barriers per query of the predecessor search.  The tiles are
// double buffered - the next one is fetched into registers before the distances of the current one and stored behind them, one
// barrier per tile - because at one workgroup per compute unit nothing else hides the fetch.  The query's d <= 64 coordinates sit
// one per lane and are read through scalar registers.
constexpr int kNnQw = 16;
template <typename T>
__global__ void __launch_bounds__(kNnQw * 64) nn_query_search_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ xq,
                                                                     int64_t ldq, int64_t nq, int* __restrict__ nbr) {
  extern __shared__ double nn_search_lds[];
  T* tile = reinterpret_cast<T*>(nn_search_lds);   // [2][d][64] candidates
  constexpr int kPre = 64 * SVGP_MAX_D / (kNnQw * 64);   // elements of a tile per thread
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t i = int64_t(blockIdx.x) * kNnQw + w;   // may be beyond nq in the last block: that wavefront only moves tiles
  const int te = 64 * P.d;
  const T qx = (i < nq && lane < P.d) ? xq[int64_t(lane) * ldq + i] : T(0);
  T pre[kPre];
  auto fetch = [&](int64_t j0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
      const int e = int(threadIdx.x) + u * kNnQw * 64, f = e >> 6, c = e & 63;
      pre[u] = (e < te && j0 + c < P.n) ? x[int64_t(f) * P.ldx + j0 + c] : T(0);
    }
  };
  auto stash = [&](T* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
      const int e = int(threadIdx.x) + u * kNnQw * 64;
      if (e < te) buf[e] = pre[u];
    }
  };
  fetch(0);
  stash(tile);
  __syncthreads();
  T bd = T(INFINITY);
  int bi = INT_MAX, cur = 0;
  for (int64_t j0 = 0; j0 < P.n; j0 += 64) {
    const bool more = j0 + 64 < P.n;
    if (more) fetch(j0 + 64);
    if (i < nq) {   // wave-uniform
      const T* tb = tile + cur * te;
      T r2 = T(0);
      for (int f = 0; f < P.d; ++f) {
        const T df = (tb[f * 64 + lane] - nn_rl(qx, f)) * T(P.invl[f]);
        r2 = fma(df, df, r2);
      }
      nn_best_insert<T>(r2, j0 + lane < P.n, j0, P.k, lane, bd, bi);
    }
    cur ^= 1;
    if (more) stash(tile + cur * te);
    __syncthreads();   // the next tile is whole, and this one is consumed before the round after next overwrites it
  }
  if (i >= nq) return;
  nn_store_row(nbr, i, nq, P.k, P.k, lane, bi);
}

// The reverse lists: the pairs (i, t) with nbr(i, t) = j, for every j, in ascending i.  The pairs are listed row by row (p = i kb + t),
// keyed by j (n for the -1 entries) and put through a stable radix sort; val = i + t n is the pair's place in B.
__global__ void nn_pairs_kernel(const int* __restrict__ nbr, int64_t n, int kb, unsigned* __restrict__ key, int64_t* __restrict__ val) {
  const int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= n * kb) return;
  const int64_t i = p / kb;
  const int t = int(p - i * kb);
  const int e = nbr[i + int64_t(t) * n];
  key[p] = e >= 0 ? unsigned(e) : unsigned(n);
  val[p] = i + int64_t(t) * n;
}
// off[j] = the first place of the sorted keys that holds a key >= j, j = 0 .. n
__global__ void nn_offsets_kernel(const unsigned* __restrict__ key, int64_t total, int64_t n, int64_t* __restrict__ off) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j > n) return;
  int64_t lo = 0, hi = total;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (int64_t(key[mid]) < j) lo = mid + 1; else hi = mid;
  }
  off[j] = lo;
}
// alpha_j = r_j / F_j - sum over the reverse list of j of B(i, t) r_i / F_i: one wavefront per j, the lanes stride the list and a
// fixed tree adds them (a hub's list has up to n - 1 pairs)
template <typename T>
__global__ void __launch_bounds__(k256) nn_alpha_tab_kernel(const T* __restrict__ Bd, const double* __restrict__ rF, int64_t n,
                                                            const int64_t* __restrict__ off, const int64_t* __restrict__ rv,
                                                            double* __restrict__ alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t j = int64_t(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  if (j >= n) return;
  double a = 0.0;
  for (int64_t p = off[j] + lane; p < off[j + 1]; p += 64) {
    const int64_t v = rv[p];
    a = fma(double(Bd[v]), rF[v % n], a);
  }
  a = nn_wave_sum(a);
  if (lane == 0) alpha[j] = rF[j] - a;
}

template <typename T>
__global__ void nn_cast_kernel(const double* __restrict__ in, int64_t n, double shift, double scale, T* __restrict__ out) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < n) out[j] = T(shift + scale * in[j]);
}

// ---- predictions ---------------------------------------------------------------------------------------------
// Kx[rr][j] = k(x_g, x*_j), g = i0 - 64 + rr, for rr < rows, j < np; 0 where g is outside [0, n) or j >= nt (row-major, ld np)
template <typename T>
__global__ void __launch_bounds__(k256) nn_kx_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ xt, int64_t ldt,
                                                     int64_t nt, int64_t np, int64_t i0, int rows, T* __restrict__ Kx) {
  const int64_t j = int64_t(blockIdx.x) * k256 + threadIdx.x;
  if (j >= np) return;
  for (int rr = blockIdx.y; rr < rows; rr += gridDim.y) {
    const int64_t g = i0 - kNnMaxK + rr;
    T v = T(0);
    if (g >= 0 && g < P.n && j < nt) {
      T r2 = T(0);
      for (int f = 0; f < P.d; ++f) {
        const T df = (x[int64_t(f) * P.ldx + g] - xt[int64_t(f) * ldt + j]) * T(P.invl[f]);
        r2 = fma(df, df, r2);
      }
      v = kappa(P.family, r2, T(P.variance));
    }
    Kx[int64_t(rr) * np + j] = v;
  }
}

// Row i of V = U' k(x, x*): (k(x_i, x*) - sum_t B(i, t) k(x_{i - kb + t}, x*)) / sqrt(F_i), for the rows [i0, i0 + 64 gridDim.y) of one
// tile (zero beyond n); per 64-row group the column sums of V.^2 and of k(x_i, x*) alpha_i (fp64).  256 threads = 64 columns x 4 rows.
template <typename T>
__global__ void __launch_bounds__(k256) nn_v_kernel(const T* __restrict__ Kx, int64_t np, int64_t i0, int64_t n, int kb,
                                                    const T* __restrict__ Bd, const double* __restrict__ Fd, const double* __restrict__ alpha,
                                                    int want_v, T* __restrict__ V, double* __restrict__ pm, double* __restrict__ pv) {
  __shared__ double sm[4][64], sv[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t j = int64_t(blockIdx.x) * 64 + tx;
  double am = 0.0, av = 0.0;
  for (int s = 0; s < 16; ++s) {
    const int rr = blockIdx.y * 64 + ty + 4 * s;
    const int64_t i = i0 + rr;
    double v = 0.0;
    if (i < n) {
      const double kx = double(Kx[int64_t(rr + kNnMaxK) * np + j]);
      am = fma(kx, alpha[i], am);
      if (want_v) {
        double acc = 0.0;
        for (int t = 0; t < kb; ++t) acc = fma(double(Bd[i + int64_t(t) * n]), double(Kx[int64_t(rr + kNnMaxK - kb + t) * np + j]), acc);
        v = (kx - acc) / sqrt(Fd[i]);
        av = fma(v, v, av);
      }
    }
    if (want_v) V[int64_t(rr) * np + j] = T(v);
  }
  sm[ty][tx] = am;
  sv[ty][tx] = av;
  __syncthreads();
  if (ty == 0) {
    pm[int64_t(blockIdx.y) * np + j] = ((sm[0][tx] + sm[1][tx]) + sm[2][tx]) + sm[3][tx];
    pv[int64_t(blockIdx.y) * np + j] = ((sv[0][tx] + sv[1][tx]) + sv[2][tx]) + sv[3][tx];
  }
}
// The same rows with a neighbour table: (k(x_i, x*) - sum_t B(i, t) k(x_nbr(i, t), x*)) / sqrt(F_i).  The neighbours of a row are
// anywhere before it, so their kernel values are evaluated here (kb + 1 evaluations per entry); same tiles and column sums.
template <typename T>
__device__ __forceinline__ T nn_kval(const NnParams& P, const T* __restrict__ x, int64_t g, const T* __restrict__ xt, int64_t ldt, int64_t j) {
  T r2 = T(0);
  for (int f = 0; f < P.d; ++f) {
    const T df = (x[int64_t(f) * P.ldx + g] - xt[int64_t(f) * ldt + j]) * T(P.invl[f]);
    r2 = fma(df, df, r2);
  }
  return kappa(P.family, r2, T(P.variance));
}
template <typename T>
__global__ void __launch_bounds__(k256) nn_vtab_kernel(const NnParams P, const T* __restrict__ x, const T* __restrict__ xt, int64_t ldt,
                                                       int64_t nt, int64_t np, int64_t i0, const int* __restrict__ nbr,
                                                       const T* __restrict__ Bd, const double* __restrict__ Fd,
                                                       const double* __restrict__ alpha, int want_v, T* __restrict__ V,
                                                       double* __restrict__ pm, double* __restrict__ pv) {
  __shared__ double sm[4][64], sv[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t j = int64_t(blockIdx.x) * 64 + tx, n = P.n;
  double am = 0.0, av = 0.0;
  for (int s = 0; s < 16; ++s) {
    const int rr = blockIdx.y * 64 + ty + 4 * s;
    const int64_t i = i0 + rr;
    double v = 0.0;
    if (i < n && j < nt) {
      const double kx = double(nn_kval<T>(P, x, i, xt, ldt, j));
      am = fma(kx, alpha[i], am);
      if (want_v) {
        double acc = 0.0;
        for (int t = 0; t < P.k; ++t) {
          const int e = nbr[i + int64_t(t) * n];   // uniform over the wavefront
          if (e < 0) break;
          acc = fma(double(Bd[i + int64_t(t) * n]), double(nn_kval<T>(P, x, e, xt, ldt, j)), acc);
        }
        v = (kx - acc) / sqrt(Fd[i]);
        av = fma(v, v, av);
      }
    }
    if (want_v) V[int64_t(rr) * np + j] = T(v);
  }
  sm[ty][tx] = am;
  sv[ty][tx] = av;
  __syncthreads();
  if (ty == 0) {
    pm[int64_t(blockIdx.y) * np + j] = ((sm[0][tx] + sm[1][tx]) + sm[2][tx]) + sm[3][tx];
    pv[int64_t(blockIdx.y) * np + j] = ((sv[0][tx] + sv[1][tx]) + sv[2][tx]) + sv[3][tx];
  }
}
// acc[j] += the tile's row-group partials, in order
__global__ void nn_colacc_kernel(const double* __restrict__ pm, const double* __restrict__ pv, int groups, int64_t np,
                                 double* __restrict__ macc, double* __restrict__ vacc) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= np) return;
  double a = macc[j], b = vacc[j];
  for (int g = 0; g < groups; ++g) {
    a += pm[int64_t(g) * np + j];
    b += pv[int64_t(g) * np + j];
  }
  macc[j] = a;
  vacc[j] = b;
}
// out[a + b na] = k(xa_a, xb_b) - acc[a][b]   (acc row-major, ld np)
template <typename T>
__global__ void nn_cov_finish_kernel(const NnParams P, const T* __restrict__ xa, int64_t lda, int64_t na, const T* __restrict__ xb,
                                     int64_t ldb, int64_t nb, const T* __restrict__ acc, int64_t np, T* __restrict__ out) {
  const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (a >= na || b >= nb) return;
  T r2 = T(0);
  for (int f = 0; f < P.d; ++f) {
    const T df = (xa[int64_t(f) * lda + a] - xb[int64_t(f) * ldb + b]) * T(P.invl[f]);
    r2 = fma(df, df, r2);
  }
  out[a + b * na] = T(double(kappa(P.family, r2, T(P.variance))) - double(acc[a * np + b]));
}

inline unsigned nblk(int64_t n, int b = 256) { return unsigned((n + b - 1) / b); }

}  // namespace
}  // namespace svgp

// ================================================================================================
using namespace svgp;

struct svgp_nn {
  const svgp_data* data = nullptr;
  int dtype = 0, d = 0;
  int64_t N = 0;
  size_t es = 8;
  DevBuf terms;   // [N][slots] fp64 per-point terms, grown on demand
  DevBuf part;    // [slots][blocks] fp64 block partials
  DevBuf res;     // [kNnGradSlots + SVGP_MAX_D] fp64 sums
  DevBuf bad;     // (int) 1-based index of the first bad point, kNnNone: none
  DevBuf Bd, Fd, rF, alpha;   // the last fit: b_i (N x kb column-major, data dtype), F_i, r_i / F_i, alpha (fp64)
  bool have_fit = false;
  NnParams P{};   // ... and its parameters
  // the neighbour table (svgp_nn_set_neighbors / svgp_nn_build_neighbors); tab_kb < 0: none, the window of the previous k points
  int tab_kb = -1;
  DevBuf nbr;        // (int) N x tab_kb column-major
  DevBuf roff, rv;   // (int64) the reverse lists: offsets [N + 1], and the places i + t N in B of the pairs with nbr(i, t) = j
  // per-point noise variances and prior-mean offsets (svgp_nn_set_noise / svgp_nn_set_mean): snapshots in the data dtype, and the
  // NaN-propagating minimum of s, reduced on the device at set time.  With either set the point kernels are those of nn_points.hip
  DevBuf sv, mu;
  bool have_s = false, have_mu = false;
  double s_min = 0;
  DevBuf Qd, gF, sbar, gout;   // svgp_nn_lml_grad_points: the per-pair terms (N x kb, data dtype), gF_i and s_bar (fp64), the cast outputs
};

namespace {

int nn_check_desc(svgp_ctx* ctx, const svgp_nn* nn, const svgp_nn_desc* ds) {
  if (!ds) return fail(ctx, SVGP_INVALID_ARG, "null NearestNeighbors descriptor");
  if (ds->dtype != nn->dtype) return fail(ctx, SVGP_INVALID_ARG, "descriptor dtype differs from the data's");
  if (ds->d != nn->d) return fail(ctx, SVGP_INVALID_ARG, "descriptor d differs from the data's");
  if (ds->kernel < SVGP_KERNEL_SE || ds->kernel > SVGP_KERNEL_MATERN52) return fail(ctx, SVGP_INVALID_ARG, "bad kernel");
  if (ds->k < 1) return fail(ctx, SVGP_INVALID_ARG, "k must be >= 1");
  if (ds->reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved field must be 0");
  if (!ds->inv_lengthscale) return fail(ctx, SVGP_INVALID_ARG, "null inv_lengthscale");
  if (!(ds->variance > 0.0)) return fail(ctx, SVGP_INVALID_ARG, "variance must be > 0");
  if (!(ds->diag >= 0.0)) return fail(ctx, SVGP_INVALID_ARG, "diag must be >= 0");
  if (std::min<int64_t>(ds->k, nn->N - 1) > kNnMaxK) return fail(ctx, SVGP_UNSUPPORTED, "more than 64 neighbours: one lane per neighbour");   // k >= N is k = N - 1
  if (nn->tab_kb >= 0 && std::min<int64_t>(ds->k, nn->N - 1) != nn->tab_kb)
    return fail(ctx, SVGP_INVALID_ARG, "descriptor k gives " + std::to_string(std::min<int64_t>(ds->k, nn->N - 1)) +
                                           " neighbours, the handle's neighbour table has " + std::to_string(nn->tab_kb));
  return SVGP_OK;
}

NnParams nn_params(const svgp_nn* nn, const svgp_nn_desc* ds) {
  NnParams P{};
  P.family = ds->kernel;
  P.d = nn->d;
  P.k = int(std::min<int64_t>(ds->k, nn->N - 1));   // k >= N is k = N - 1
  P.n = nn->N;
  P.ldx = nn->data->ldx;
  P.variance = ds->variance;
  P.diag = ds->diag;
  P.mean_const = ds->mean_const;
  for (int f = 0; f < nn->d; ++f) P.invl[f] = ds->inv_lengthscale[f];
  return P;
}

template <typename T, int MODE>
void nn_launch_point(hipStream_t s, const NnParams& P, const svgp_nn* nn, int S) {
  const dim3 grid(nblk(P.n, 4)), block(k256);
  const T *x = (const T*)nn->data->x.p, *y = (const T*)nn->data->y.p;
  double* terms = nn->terms.as<double>();
  int* bad = nn->bad.as<int>();
  T* Bd = (T*)nn->Bd.p;
  double *Fd = nn->Fd.as<double>(), *rF = nn->rF.as<double>();
  if (nn->tab_kb >= 0) {
    const int* nbr = nn->nbr.as<int>();
    if (P.k <= 16) hipLaunchKernelGGL((nn_point_tab_kernel<T, 16, MODE>), grid, block, 0, s, P, x, y, terms, S, bad, Bd, Fd, rF, nbr);
    else if (P.k <= 32) hipLaunchKernelGGL((nn_point_tab_kernel<T, 32, MODE>), grid, block, 0, s, P, x, y, terms, S, bad, Bd, Fd, rF, nbr);
    else hipLaunchKernelGGL((nn_point_tab_kernel<T, 64, MODE>), grid, block, 0, s, P, x, y, terms, S, bad, Bd, Fd, rF, nbr);
    return;
  }
  if (P.k <= 16) hipLaunchKernelGGL((nn_point_kernel<T, 16, MODE>), grid, block, 0, s, P, x, y, terms, S, bad, Bd, Fd, rF);
  else if (P.k <= 32) hipLaunchKernelGGL((nn_point_kernel<T, 32, MODE>), grid, block, 0, s, P, x, y, terms, S, bad, Bd, Fd, rF);
  else hipLaunchKernelGGL((nn_point_kernel<T, 64, MODE>), grid, block, 0, s, P, x, y, terms, S, bad, Bd, Fd, rF);
}

// a noise vector is set: the smallest variance T(diag) + min s of the call's descriptor, before any data pass (svgp_cg_set_noise's rule)
int nn_noise_check(svgp_ctx* ctx, const svgp_nn* nn, const svgp_nn_desc* ds) {
  if (!nn->have_s) return SVGP_OK;
  const double lo = nn->dtype == SVGP_F64 ? ds->diag + nn->s_min : double(float(ds->diag) + float(nn->s_min));
  if (lo != lo) return fail(ctx, SVGP_NOT_POSDEF, "NearestNeighbors per-point noise: a variance diag + s_i is NaN");
  if (lo < 0) return fail(ctx, SVGP_NOT_POSDEF, "NearestNeighbors per-point noise: a variance diag + s_i is negative");
  return SVGP_OK;
}

// mode 0: lml; 1: fit; 2: lml and gradient; 3: lml, gradient, fit, s_bar and the sum of alpha (svgp_nn_lml_grad_points).
// out[S] = the reduced slots (mode 3: out[S] = sum_j alpha_j after them)
int nn_eval(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* ds, int mode, double* lml_out, svgp_nn_info* info, double* out) {
  int rc = nn_check_desc(ctx, nn, ds);
  if (rc) return rc;
  if (!lml_out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  const bool fits = mode == 1 || mode == 3;
  if ((rc = nn_noise_check(ctx, nn, ds)) != SVGP_OK) {   // before the data pass
    if (fits) nn->have_fit = false;
    *lml_out = NAN;
    if (info) {
      std::memset(info, 0, sizeof(*info));
      info->lml = NAN;
    }
    return rc;
  }
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const NnParams P = nn_params(nn, ds);
  const int64_t N = nn->N;
  const int S = mode >= 2 ? kNnGradSlots + nn->d : kNnSlots;
  const int nb = int(std::min<int64_t>(1024, (N + 1023) / 1024));
  const int64_t chunk = (N + nb - 1) / nb;
  const bool vec = nn->have_s || nn->have_mu || mode == 3;   // the kernels of nn_points.hip
  rc = nn->terms.reserve(ctx, size_t(N) * S * 8, "the NearestNeighbors per-point terms");
  if (rc == SVGP_OK) rc = nn->part.reserve(ctx, size_t(nb) * S * 8, "the NearestNeighbors block partials");
  if (rc == SVGP_OK && fits) {
    nn->have_fit = false;
    rc = nn->Bd.reserve(ctx, std::max<size_t>(size_t(N) * P.k * nn->es, 8), "the NearestNeighbors rows b_i");
    if (rc == SVGP_OK) rc = nn->Fd.reserve(ctx, size_t(N) * 8, "F");
    if (rc == SVGP_OK) rc = nn->rF.reserve(ctx, size_t(N) * 8, "r / F");
    if (rc == SVGP_OK) rc = nn->alpha.reserve(ctx, size_t(N) * 8, "alpha");
    if (rc == SVGP_OK && P.k > 0) HIPC(ctx, hipMemsetAsync(nn->Bd.p, 0, size_t(N) * P.k * nn->es, s));   // the ramp-up rows i < k are shorter
  }
  if (rc == SVGP_OK && mode == 3) {
    rc = nn->Qd.reserve(ctx, std::max<size_t>(size_t(N) * P.k * nn->es, 8), "the NearestNeighbors per-pair gradient terms");
    if (rc == SVGP_OK) rc = nn->gF.reserve(ctx, size_t(N) * 8, "gF");
    if (rc == SVGP_OK) rc = nn->sbar.reserve(ctx, size_t(N) * 8, "s_bar");
    if (rc == SVGP_OK && P.k > 0) HIPC(ctx, hipMemsetAsync(nn->Qd.p, 0, size_t(N) * P.k * nn->es, s));
  }
  if (rc) return rc;
  HIPC(ctx, hipMemsetAsync(nn->bad.p, 0x7f, sizeof(int), s));   // kNnNone
  if (vec) {
    const NnPointArgs a{nn->data->x.p, nn->data->y.p, nn->have_s ? nn->sv.p : nullptr, nn->have_mu ? nn->mu.p : nullptr,
                        nn->terms.as<double>(), S, nn->bad.as<int>(), nn->Bd.p, nn->Fd.as<double>(), nn->rF.as<double>(), nn->Qd.p,
                        nn->gF.as<double>(), nn->tab_kb >= 0 ? nn->nbr.as<int>() : nullptr};
    launch_nn_point_v(nn->dtype, mode, s, P, a);
  } else {
    NN_DISPATCH(nn->dtype, T, {
      if (mode == 0) nn_launch_point<T, 0>(s, P, nn, S);
      else if (mode == 1) nn_launch_point<T, 1>(s, P, nn, S);
      else nn_launch_point<T, 2>(s, P, nn, S);
    });
  }
  KCHECK(ctx, "nn_point");
  hipLaunchKernelGGL(nn_reduce1_kernel, dim3((unsigned)nb, (unsigned)S), dim3(k256), 0, s, (const double*)nn->terms.as<double>(), N, S, chunk,
                     nn->part.as<double>());
  hipLaunchKernelGGL(nn_reduce2_kernel, dim3((unsigned)S), dim3(k256), 0, s, (const double*)nn->part.as<double>(), nb, nn->res.as<double>());
  if (fits)
    NN_DISPATCH(nn->dtype, T, {
      if (nn->tab_kb >= 0)
        hipLaunchKernelGGL(nn_alpha_tab_kernel<T>, dim3(nblk(N, 4)), dim3(k256), 0, s, (const T*)nn->Bd.p, (const double*)nn->rF.as<double>(), N,
                           (const int64_t*)nn->roff.as<int64_t>(), (const int64_t*)nn->rv.as<int64_t>(), nn->alpha.as<double>());
      else
        hipLaunchKernelGGL(nn_alpha_kernel<T>, dim3(nblk(N)), dim3(256), 0, s, (const T*)nn->Bd.p, (const double*)nn->rF.as<double>(), N, P.k,
                           nn->alpha.as<double>());
    });
  if (mode == 3) {   // s_bar by the same gathers, and the sum of alpha in the fixed order of the slots (the partials are free again)
    const bool tab = nn->tab_kb >= 0;
    launch_nn_sbar(nn->dtype, s, nn->Qd.p, nn->gF.as<double>(), N, P.k, tab ? nn->roff.as<int64_t>() : nullptr,
                   tab ? nn->rv.as<int64_t>() : nullptr, nn->sbar.as<double>());
    hipLaunchKernelGGL(nn_reduce1_kernel, dim3((unsigned)nb, 1u), dim3(k256), 0, s, (const double*)nn->alpha.as<double>(), N, 1, chunk,
                       nn->part.as<double>());
    hipLaunchKernelGGL(nn_reduce2_kernel, dim3(1u), dim3(k256), 0, s, (const double*)nn->part.as<double>(), nb, nn->res.as<double>() + S);
  }
  KCHECK(ctx, "nn_reduce");
  int badv = 0;
  HIPC(ctx, hipMemcpyAsync(out, nn->res.p, size_t(S + (mode == 3 ? 1 : 0)) * 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipMemcpyAsync(&badv, nn->bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  const bool isbad = badv != kNnNone;
  const double lml = isbad ? NAN : -0.5 * (double(N) * 1.8378770664093454836 + out[0] + out[1]);
  *lml_out = lml;
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->first_bad = isbad ? badv : 0;
    info->n_neg_f = int64_t(out[2]);
    info->lml = lml;
  }
  if (isbad)
    return fail(ctx, SVGP_NOT_POSDEF, "NearestNeighbors: the block or F of point " + std::to_string(badv) + " is not positive");
  if (fits) {
    nn->P = P;
    nn->have_fit = true;
  }
  return SVGP_OK;
}

// a snapshot of N values of the data dtype from host or device memory into buf; src null: the vector is removed.  Either way the
// fit is discarded, as a table call does
int nn_set_vector(svgp_ctx* ctx, svgp_nn* nn, const void* src, bool given, int32_t on_device, int32_t reserved, DevBuf& buf, bool& have,
                  const char* what) {
  if (given && !src) return fail(ctx, SVGP_INVALID_ARG, std::string("null ") + what);
  if (given && on_device != 0 && on_device != 1) return fail(ctx, SVGP_INVALID_ARG, "on_device must be 0 or 1");
  if (given && reserved != 0) return fail(ctx, SVGP_INVALID_ARG, "reserved must be 0");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  nn->have_fit = false;
  have = false;   // (a failure below leaves the handle without the vector)
  if (!given) return SVGP_OK;
  const size_t nb = size_t(nn->N) * nn->es;
  const int rc = buf.reserve(ctx, nb, what);
  if (rc) return rc;
  HIPC(ctx, hipMemcpyAsync(buf.p, src, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  HIPC(ctx, hipStreamSynchronize(s));   // the caller's memory is the caller's again
  have = true;
  return SVGP_OK;
}

int check_point_out(svgp_ctx* ctx, const void* p, int32_t on_device, int32_t reserved, const char* what) {
  if (!p) return fail(ctx, SVGP_INVALID_ARG, std::string("null ") + what);
  if ((on_device != 0 && on_device != 1) || reserved != 0)
    return fail(ctx, SVGP_INVALID_ARG, std::string(what) + ": on_device must be 0 or 1 and reserved 0");
  return SVGP_OK;
}

struct NnHold {   // test inputs uploaded for one call
  svgp_ctx* ctx;
  svgp_data* D = nullptr;
  ~NnHold() { if (D) svgp_data_free(ctx, D); }
};

// mean / var / cov of the column set A, or cov(A, B) when Bset is given (then only cov_out)
int nn_predict_impl(svgp_ctx* ctx, svgp_nn* nn, const svgp_data* Aset, const svgp_data* Bset, void* mean_out, void* var_out, void* cov_out) {
  hipStream_t s = ctx->stream;
  const NnParams& P = nn->P;
  const int64_t N = nn->N, na = Aset->n, nbp = Bset ? Bset->n : 0;
  const int64_t np = (std::max(na, nbp) + kNB - 1) / kNB * kNB;
  const bool want_v = var_out || cov_out;
  const int rows_max = int(std::max<int64_t>(64, std::min<int64_t>(kNnRows, kNnTileElems / np / 64 * 64)));
  const int groups_max = rows_max / 64;
  const size_t es = nn->es;
  DevBuf Kx, Va, Vb, pm, pv, macc, vacc, Cacc, outb;
  const bool tab = nn->tab_kb >= 0;
  if (!tab) HIPC(ctx, Kx.alloc(size_t(rows_max + kNnMaxK) * np * es));
  if (want_v) HIPC(ctx, Va.alloc(size_t(rows_max) * np * es));
  if (Bset) HIPC(ctx, Vb.alloc(size_t(rows_max) * np * es));
  HIPC(ctx, pm.alloc(size_t(groups_max) * np * 8));
  HIPC(ctx, pv.alloc(size_t(groups_max) * np * 8));
  HIPC(ctx, macc.alloc(size_t(np) * 8));
  HIPC(ctx, vacc.alloc(size_t(np) * 8));
  HIPC(ctx, hipMemsetAsync(macc.p, 0, size_t(np) * 8, s));
  HIPC(ctx, hipMemsetAsync(vacc.p, 0, size_t(np) * 8, s));
  if (cov_out) HIPC(ctx, Cacc.alloc(size_t(np) * np * es));
  bool first = true;
  for (int64_t i0 = 0; i0 < N; i0 += rows_max) {
    const int rows = int(std::min<int64_t>(rows_max, N - i0));
    const int groups = (rows + 63) / 64;
    NN_DISPATCH(nn->dtype, T, {
      for (int side = 0; side < (Bset ? 2 : 1); ++side) {
        const svgp_data* D = side ? Bset : Aset;
        if (tab) {
          hipLaunchKernelGGL(nn_vtab_kernel<T>, dim3(unsigned(np / 64), unsigned(groups)), dim3(k256), 0, s, P, (const T*)nn->data->x.p,
                             (const T*)D->x.p, D->ldx, D->n, np, i0, (const int*)nn->nbr.as<int>(), (const T*)nn->Bd.p,
                             (const double*)nn->Fd.as<double>(), (const double*)nn->alpha.as<double>(), want_v ? 1 : 0,
                             (T*)(side ? Vb.p : Va.p), pm.as<double>(), pv.as<double>());
        } else {
          hipLaunchKernelGGL(nn_kx_kernel<T>, dim3(nblk(np), 256), dim3(k256), 0, s, P, (const T*)nn->data->x.p, (const T*)D->x.p, D->ldx, D->n,
                             np, i0, groups * 64 + kNnMaxK, (T*)Kx.p);
          hipLaunchKernelGGL(nn_v_kernel<T>, dim3(unsigned(np / 64), unsigned(groups)), dim3(k256), 0, s, (const T*)Kx.p, np, i0, N, P.k,
                             (const T*)nn->Bd.p, (const double*)nn->Fd.as<double>(), (const double*)nn->alpha.as<double>(), want_v ? 1 : 0,
                             (T*)(side ? Vb.p : Va.p), pm.as<double>(), pv.as<double>());
        }
        if (!side)
          hipLaunchKernelGGL(nn_colacc_kernel, dim3(nblk(np)), dim3(256), 0, s, (const double*)pm.as<double>(), (const double*)pv.as<double>(),
                             groups, np, macc.as<double>(), vacc.as<double>());
      }
    });
    KCHECK(ctx, "nn predict tile");
    if (cov_out) {
      launch_gemm_pm(nn->dtype, s, Va.p, Bset ? Vb.p : Va.p, nullptr, 1.0, np, int64_t(groups) * 64, int64_t(groups) * 64, 1, Cacc.p,
                     first ? 1 : 0, kMmFull);
      KCHECK(ctx, "gemm_pm (V'V)");
    }
    first = false;
  }
  const size_t ob = std::max(size_t(na) * (cov_out ? std::max<int64_t>(Bset ? nbp : na, 1) : 1), size_t(1)) * es;
  HIPC(ctx, outb.alloc(ob));
  NN_DISPATCH(nn->dtype, T, {
    if (mean_out) {
      hipLaunchKernelGGL(nn_cast_kernel<T>, dim3(nblk(na)), dim3(256), 0, s, (const double*)macc.as<double>(), na, P.mean_const, 1.0, (T*)outb.p);
      HIPC(ctx, hipMemcpyAsync(mean_out, outb.p, size_t(na) * es, hipMemcpyDeviceToHost, s));
    }
    if (var_out) {
      hipLaunchKernelGGL(nn_cast_kernel<T>, dim3(nblk(na)), dim3(256), 0, s, (const double*)vacc.as<double>(), na, P.variance, -1.0, (T*)outb.p);
      HIPC(ctx, hipMemcpyAsync(var_out, outb.p, size_t(na) * es, hipMemcpyDeviceToHost, s));
    }
    if (cov_out) {
      const svgp_data* D2 = Bset ? Bset : Aset;
      hipLaunchKernelGGL(nn_cov_finish_kernel<T>, dim3(nblk(na), (unsigned)D2->n), dim3(256), 0, s, P, (const T*)Aset->x.p, Aset->ldx, na,
                         (const T*)D2->x.p, D2->ldx, D2->n, (const T*)Cacc.p, np, (T*)outb.p);
      HIPC(ctx, hipMemcpyAsync(cov_out, outb.p, size_t(na) * D2->n * es, hipMemcpyDeviceToHost, s));
    }
  });
  KCHECK(ctx, "nn predict finish");
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

void nn_drop_table(svgp_nn* nn) {
  nn->tab_kb = -1;
  nn->have_fit = false;
}

// k of a set / build call -> kb = min(k, N - 1), or a status
int nn_table_kb(svgp_ctx* ctx, const svgp_nn* nn, int32_t k, int* kb) {
  if (k < 1) return fail(ctx, SVGP_INVALID_ARG, "k must be >= 1");
  if (nn->N > int64_t(INT_MAX)) return fail(ctx, SVGP_UNSUPPORTED, "a neighbour table holds int32 indices: N does not fit");
  if (std::min<int64_t>(k, nn->N - 1) > kNnMaxK) return fail(ctx, SVGP_UNSUPPORTED, "more than 64 neighbours: one lane per neighbour");
  *kb = int(std::min<int64_t>(k, nn->N - 1));
  return SVGP_OK;
}

// the reverse lists of nn->nbr (N x kb): a stable radix sort of the pairs by the point they name, then the offsets
int nn_reverse_lists(svgp_ctx* ctx, svgp_nn* nn, int kb) {
  hipStream_t s = ctx->stream;
  const int64_t N = nn->N, total = N * kb;
  int rc = nn->roff.reserve(ctx, size_t(N + 1) * 8, "the reverse-list offsets");
  if (rc == SVGP_OK) rc = nn->rv.reserve(ctx, std::max<size_t>(size_t(total) * 8, 8), "the reverse lists");
  if (rc) return rc;
  DevBuf key, key2, val, tmp;
  if (total > 0) {
    HIPC(ctx, key.alloc(size_t(total) * 4));
    HIPC(ctx, key2.alloc(size_t(total) * 4));
    HIPC(ctx, val.alloc(size_t(total) * 8));
    hipLaunchKernelGGL(nn_pairs_kernel, dim3(nblk(total)), dim3(256), 0, s, (const int*)nn->nbr.as<int>(), N, kb, key.as<unsigned>(),
                       val.as<int64_t>());
    KCHECK(ctx, "nn_pairs");
    unsigned bits = 1;
    while (bits < 32 && (uint64_t(1) << bits) <= uint64_t(N)) ++bits;   // the keys are 0 .. N
    size_t tb = 0;
    HIPC(ctx, rocprim::radix_sort_pairs(nullptr, tb, key.as<unsigned>(), key2.as<unsigned>(), val.as<int64_t>(), nn->rv.as<int64_t>(),
                                        size_t(total), 0u, bits, s));
    HIPC(ctx, tmp.alloc(std::max<size_t>(tb, 8)));
    HIPC(ctx, rocprim::radix_sort_pairs(tmp.p, tb, key.as<unsigned>(), key2.as<unsigned>(), val.as<int64_t>(), nn->rv.as<int64_t>(),
                                        size_t(total), 0u, bits, s));
  }
  hipLaunchKernelGGL(nn_offsets_kernel, dim3(nblk(N + 1)), dim3(256), 0, s, (const unsigned*)key2.as<unsigned>(), total, N,
                     nn->roff.as<int64_t>());
  KCHECK(ctx, "nn_offsets");
  HIPC(ctx, hipStreamSynchronize(s));   // the sort's buffers are released on return
  return SVGP_OK;
}

}  // namespace

extern "C" {

int32_t svgp_nn_set_neighbors(svgp_ctx* ctx, svgp_nn* nn, int32_t k, const int32_t* nbr_host) {
  if (!ctx || !nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  nn_drop_table(nn);
  int kb = 0;
  int rc = nn_table_kb(ctx, nn, k, &kb);
  if (rc) return rc;
  if (!nbr_host && kb > 0) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = nn->N;
  rc = nn->nbr.reserve(ctx, std::max<size_t>(size_t(N) * kb * 4, 8), "the neighbour table");
  if (rc) return rc;
  if (kb > 0) {
    HIPC(ctx, hipMemcpyAsync(nn->nbr.p, nbr_host, size_t(N) * kb * 4, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemsetAsync(nn->bad.p, 0x7f, sizeof(int), s));   // kNnNone
    hipLaunchKernelGGL(nn_check_tab_kernel, dim3(nblk(N, 4)), dim3(k256), 0, s, (const int*)nn->nbr.as<int>(), N, kb, nn->bad.as<int>());
    KCHECK(ctx, "nn_check_tab");
    int badv = 0;
    HIPC(ctx, hipMemcpyAsync(&badv, nn->bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));   // also: nbr_host is the caller's again
    if (badv != kNnNone)
      return fail(ctx, SVGP_INVALID_ARG, "neighbour table: row " + std::to_string(badv) + " (1-based) is not a set of distinct earlier points, the valid entries first and -1 after them");
  }
  rc = nn_reverse_lists(ctx, nn, kb);
  if (rc) return rc;
  nn->tab_kb = kb;
  return SVGP_OK;
}

int32_t svgp_nn_build_neighbors(svgp_ctx* ctx, svgp_nn* nn, int32_t k, const double* inv_lengthscale) {
  if (!ctx || !nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  nn_drop_table(nn);
  int kb = 0;
  int rc = nn_table_kb(ctx, nn, k, &kb);
  if (rc) return rc;
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = nn->N;
  rc = nn->nbr.reserve(ctx, std::max<size_t>(size_t(N) * kb * 4, 8), "the neighbour table");
  if (rc) return rc;
  if (kb > 0) {
    NnParams P{};
    P.d = nn->d;
    P.k = kb;
    P.n = N;
    P.ldx = nn->data->ldx;
    for (int f = 0; f < nn->d; ++f) P.invl[f] = inv_lengthscale ? inv_lengthscale[f] : 1.0;
    NN_DISPATCH(nn->dtype, T, {
      hipLaunchKernelGGL(nn_search_kernel<T>, dim3(nblk(N, 4)), dim3(k256), size_t(68) * nn->d * sizeof(T), s, P, (const T*)nn->data->x.p,
                         nn->nbr.as<int>());
    });
    KCHECK(ctx, "nn_search");
  }
  rc = nn_reverse_lists(ctx, nn, kb);
  if (rc) return rc;
  nn->tab_kb = kb;
  return SVGP_OK;
}

int32_t svgp_nn_get_neighbors(svgp_ctx* ctx, svgp_nn* nn, int32_t* k_out, int32_t* nbr_out) {
  if (!ctx || !nn || !k_out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  *k_out = nn->tab_kb;
  if (nn->tab_kb <= 0 || !nbr_out) return SVGP_OK;
  HIPC(ctx, hipSetDevice(ctx->device));
  HIPC(ctx, hipMemcpyAsync(nbr_out, nn->nbr.p, size_t(nn->N) * nn->tab_kb * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(ctx, hipStreamSynchronize(ctx->stream));
  return SVGP_OK;
}

int32_t svgp_nn_clear_neighbors(svgp_ctx* ctx, svgp_nn* nn) {
  if (!ctx || !nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  nn_drop_table(nn);
  return SVGP_OK;
}

int32_t svgp_nn_create(svgp_ctx* ctx, const svgp_data* data, svgp_nn** out) {
  if (!ctx || !data || !out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!data->y.p) return fail(ctx, SVGP_INVALID_ARG, "the NearestNeighbors approximation needs y");
  if (data->n < 1) return fail(ctx, SVGP_INVALID_ARG, "empty data");
  HIPC(ctx, hipSetDevice(ctx->device));
  auto* nn = new (std::nothrow) svgp_nn();
  if (!nn) return SVGP_OOM;
  nn->data = data;
  nn->dtype = data->dtype;
  nn->d = data->d;
  nn->N = data->n;
  nn->es = data->dtype == SVGP_F64 ? 8 : 4;
  hipError_t e = nn->res.alloc((kNnGradSlots + SVGP_MAX_D + 1) * 8);   // the slots' sums, then the sum of alpha
  if (e == hipSuccess) e = nn->bad.alloc(256);
  if (e != hipSuccess) {
    delete nn;
    return fail(ctx, e == hipErrorOutOfMemory ? SVGP_OOM : SVGP_HIP_ERROR, std::string("svgp_nn_create: ") + hipGetErrorString(e));
  }
  *out = nn;
  return SVGP_OK;
}

int32_t svgp_nn_free(svgp_ctx* ctx, svgp_nn* nn) {
  if (!nn) return SVGP_OK;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  delete nn;
  return SVGP_OK;
}

int32_t svgp_nn_lml(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info) {
  if (!ctx || !nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  double out[kNnGradSlots + SVGP_MAX_D];
  return nn_eval(ctx, nn, desc, 0, lml_out, info, out);
}

int32_t svgp_nn_lml_grad(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info, double* d_variance,
                         double* d_inv_lengthscale, double* d_diag) {
  if (!ctx || !nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!d_variance || !d_inv_lengthscale) {
    const int rc = nn_check_desc(ctx, nn, desc);
    return rc ? rc : fail(ctx, SVGP_INVALID_ARG, "null argument");
  }
  double out[kNnGradSlots + SVGP_MAX_D];
  const int rc = nn_eval(ctx, nn, desc, 2, lml_out, info, out);
  if (rc) return rc;
  *d_variance = out[3];
  if (d_diag) *d_diag = out[4];
  for (int f = 0; f < nn->d; ++f) d_inv_lengthscale[f] = out[kNnGradSlots + f];
  return SVGP_OK;
}

int32_t svgp_nn_set_noise(svgp_ctx* ctx, svgp_nn* nn, const svgp_point_noise* pn) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  int rc = nn_set_vector(ctx, nn, pn ? pn->s : nullptr, pn != nullptr, pn ? pn->on_device : 0, pn ? pn->reserved : 0, nn->sv, nn->have_s,
                         "noise vector");
  if (rc || !pn) return rc;
  nn->have_s = false;
  hipStream_t s = ctx->stream;
  launch_cg_noise_min(nn->dtype, s, nn->sv.p, nn->N, nn->res.as<double>());   // NaN-propagating, one workgroup, a fixed tree
  KCHECK(ctx, "nn (noise minimum)");
  double lo = 0;
  HIPC(ctx, hipMemcpyAsync(&lo, nn->res.p, 8, hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));
  nn->s_min = lo;
  nn->have_s = true;
  return SVGP_OK;
}

int32_t svgp_nn_set_mean(svgp_ctx* ctx, svgp_nn* nn, const svgp_point_mean* pm) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  return nn_set_vector(ctx, nn, pm ? pm->mu : nullptr, pm != nullptr, pm ? pm->on_device : 0, pm ? pm->reserved : 0, nn->mu, nn->have_mu,
                       "mean offsets");
}

int32_t svgp_nn_lml_grad_points(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info,
                                double* d_variance, double* d_inv_lengthscale, double* d_diag, double* d_mean_const,
                                svgp_point_mean_grad* gpm, svgp_point_noise_grad* gpn) {
  if (!ctx) return SVGP_INVALID_ARG;
  if (!nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  int rc = nn_check_desc(ctx, nn, desc);
  if (rc) return rc;
  if (!d_variance || !d_inv_lengthscale) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (gpm && (rc = check_point_out(ctx, gpm->mu_bar, gpm->on_device, gpm->reserved, "mean gradient output")) != SVGP_OK) return rc;
  if (gpn && (rc = check_point_out(ctx, gpn->s_bar, gpn->on_device, gpn->reserved, "noise gradient output")) != SVGP_OK) return rc;
  double out[kNnGradSlots + SVGP_MAX_D + 1];
  rc = nn_eval(ctx, nn, desc, 3, lml_out, info, out);
  if (rc) return rc;
  *d_variance = out[3];
  if (d_diag) *d_diag = out[4];
  for (int f = 0; f < nn->d; ++f) d_inv_lengthscale[f] = out[kNnGradSlots + f];
  if (d_mean_const) *d_mean_const = out[kNnGradSlots + nn->d];
  if (!gpm && !gpn) return SVGP_OK;
  hipStream_t s = ctx->stream;
  const int64_t N = nn->N;
  const size_t nb = size_t(N) * nn->es;
  rc = nn->gout.reserve(ctx, nb, "the per-point gradient in the data dtype");
  if (rc) return rc;
  for (int q = 0; q < 2; ++q) {   // fp64 sums, rounded once to the data dtype: into the caller's device memory, or staged for the host's
    void* dst = q ? (gpn ? gpn->s_bar : nullptr) : (gpm ? gpm->mu_bar : nullptr);
    if (!dst) continue;
    const bool dev = q ? gpn->on_device != 0 : gpm->on_device != 0;
    NN_DISPATCH(nn->dtype, T, {
      hipLaunchKernelGGL(nn_cast_kernel<T>, dim3(nblk(N)), dim3(256), 0, s, (const double*)(q ? nn->sbar : nn->alpha).as<double>(), N, 0.0, 1.0,
                         (T*)(dev ? dst : nn->gout.p));
    });
    KCHECK(ctx, "nn_cast");
    if (!dev) {
      HIPC(ctx, hipMemcpyAsync(dst, nn->gout.p, nb, hipMemcpyDeviceToHost, s));
      HIPC(ctx, hipStreamSynchronize(s));   // gout is reused by the second vector
    }
  }
  return SVGP_OK;
}

int32_t svgp_nn_fit(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info) {
  if (!ctx || !nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  double out[kNnGradSlots + SVGP_MAX_D];
  return nn_eval(ctx, nn, desc, 1, lml_out, info, out);
}

int32_t svgp_nn_factors(svgp_ctx* ctx, svgp_nn* nn, void* B_out, void* F_out, void* alpha_out) {
  if (!ctx || !nn) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!nn->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_nn_fit on this handle yet");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t N = nn->N;
  if (B_out && nn->P.k > 0) HIPC(ctx, hipMemcpyAsync(B_out, nn->Bd.p, size_t(N) * nn->P.k * nn->es, hipMemcpyDeviceToHost, s));
  DevBuf tmp;
  HIPC(ctx, tmp.alloc(size_t(N) * nn->es));
  for (int q = 0; q < 2; ++q) {
    void* dst = q ? alpha_out : F_out;
    if (!dst) continue;
    NN_DISPATCH(nn->dtype, T, {
      hipLaunchKernelGGL(nn_cast_kernel<T>, dim3(nblk(N)), dim3(256), 0, s, (const double*)(q ? nn->alpha : nn->Fd).as<double>(), N, 0.0, 1.0,
                         (T*)tmp.p);
    });
    KCHECK(ctx, "nn_cast");
    HIPC(ctx, hipMemcpyAsync(dst, tmp.p, size_t(N) * nn->es, hipMemcpyDeviceToHost, s));
  }
  HIPC(ctx, hipStreamSynchronize(s));
  return SVGP_OK;
}

int32_t svgp_nn_predict(svgp_ctx* ctx, svgp_nn* nn, int32_t layout, int64_t n, const void* x_host, void* mean_out, void* var_out,
                        void* cov_out) {
  if (!ctx || !nn || !x_host) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!nn->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_nn_fit on this handle yet");
  if (n < 1) return fail(ctx, SVGP_INVALID_ARG, "no test points");
  if (cov_out && n > kNnMaxCov) return fail(ctx, SVGP_UNSUPPORTED, "cov of more than 4096 test points");
  if (n > kNnMaxPred) return fail(ctx, SVGP_UNSUPPORTED, "more than 131072 test points in one call");
  NnHold h{ctx};
  const int rc = svgp_data_upload(ctx, nn->dtype, layout, nn->d, n, x_host, nullptr, &h.D);
  if (rc) return rc;
  return nn_predict_impl(ctx, nn, h.D, nullptr, mean_out, var_out, cov_out);
}

int32_t svgp_nn_predict_cross_cov(svgp_ctx* ctx, svgp_nn* nn, int32_t layout, int64_t nx, const void* x_host, int64_t ny,
                                  const void* y_host, void* cov_out) {
  if (!ctx || !nn || !x_host || !y_host || !cov_out) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!nn->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_nn_fit on this handle yet");
  if (nx < 1 || ny < 1) return fail(ctx, SVGP_INVALID_ARG, "no test points");
  if (nx > kNnMaxCov || ny > kNnMaxCov) return fail(ctx, SVGP_UNSUPPORTED, "cov of more than 4096 test points");
  NnHold hx{ctx}, hy{ctx};
  int rc = svgp_data_upload(ctx, nn->dtype, layout, nn->d, nx, x_host, nullptr, &hx.D);
  if (!rc) rc = svgp_data_upload(ctx, nn->dtype, layout, nn->d, ny, y_host, nullptr, &hy.D);
  if (rc) return rc;
  return nn_predict_impl(ctx, nn, hx.D, hy.D, nullptr, nullptr, cov_out);
}

int32_t svgp_nn_predict_local(svgp_ctx* ctx, svgp_nn* nn, int32_t layout, int64_t n, const void* x_host, int32_t k, void* mean_out,
                              void* var_out, int32_t* nbr_out) {
  if (!ctx || !nn || !x_host) return fail(ctx, SVGP_INVALID_ARG, "null argument");
  if (!nn->have_fit) return fail(ctx, SVGP_INVALID_ARG, "no successful svgp_nn_fit on this handle yet");
  if (n < 1) return fail(ctx, SVGP_INVALID_ARG, "no test points");
  if (k < 1) return fail(ctx, SVGP_INVALID_ARG, "k must be >= 1");
  if (layout < 0 || layout > SVGP_VEC || (layout == SVGP_VEC && nn->d != 1)) return fail(ctx, SVGP_INVALID_ARG, "bad layout");
  if (std::min<int64_t>(k, nn->N) > kNnMaxK) return fail(ctx, SVGP_UNSUPPORTED, "more than 64 neighbours: one lane per neighbour");
  if (nn->N > int64_t(INT_MAX)) return fail(ctx, SVGP_UNSUPPORTED, "a neighbour table holds int32 indices: N does not fit");
  HIPC(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  NnParams P = nn->P;
  P.k = int(std::min<int64_t>(k, nn->N));   // k > N is N
  const int d = nn->d, kq = P.k;
  const size_t es = nn->es;
  const int64_t cmax = std::min(n, kNnLocalChunk);
  const bool colvecs = layout == SVGP_COLVECS && d > 1;
  DevBuf xq, xt, tab, mo, vo;
  HIPC(ctx, xq.alloc(size_t(cmax) * d * es));
  if (colvecs) HIPC(ctx, xt.alloc(size_t(cmax) * d * es));
  HIPC(ctx, tab.alloc(size_t(cmax) * kq * 4));
  if (mean_out) HIPC(ctx, mo.alloc(size_t(cmax) * es));
  if (var_out) HIPC(ctx, vo.alloc(size_t(cmax) * es));
  HIPC(ctx, hipMemsetAsync(nn->bad.p, 0x7f, sizeof(int), s));   // kNnNone
  const char* xh = static_cast<const char*>(x_host);
  for (int64_t q0 = 0; q0 < n; q0 += kNnLocalChunk) {
    const int64_t c = std::min(kNnLocalChunk, n - q0);   // this round's queries: feature-major [d][c] in xq
    if (colvecs) {
      HIPC(ctx, hipMemcpyAsync(xt.p, xh + size_t(q0) * d * es, size_t(c) * d * es, hipMemcpyHostToDevice, s));
      launch_transpose_colvecs(nn->dtype, s, xt.p, d, c, c, xq.p);
      KCHECK(ctx, "transpose_colvecs");
    } else {
      for (int f = 0; f < d; ++f)   // n x d column-major: a round's rows are strided
        HIPC(ctx, hipMemcpyAsync(static_cast<char*>(xq.p) + size_t(f) * c * es, xh + (size_t(f) * n + q0) * es, size_t(c) * es,
                                 hipMemcpyHostToDevice, s));
    }
    NN_DISPATCH(nn->dtype, T, {
      const T *x = (const T*)nn->data->x.p, *y = (const T*)nn->data->y.p, *q = (const T*)xq.p;
      hipLaunchKernelGGL(nn_query_search_kernel<T>, dim3(nblk(c, kNnQw)), dim3(kNnQw * 64), size_t(2) * 64 * d * sizeof(T), s, P, x, q, c, c,
                         tab.as<int>());
      const dim3 grid(nblk(c, 4)), block(k256);
      const int* nbr = tab.as<int>();
      int* bad = nn->bad.as<int>();
      if (nn->have_s || nn->have_mu)   // the fit's vectors: setting one discards the fit, so these are the ones it was made with
        launch_nn_local_v(nn->dtype, s, P, x, y, nn->have_s ? nn->sv.p : nullptr, nn->have_mu ? nn->mu.p : nullptr, q, c, c, q0, nbr, bad,
                          mo.p, vo.p);
      else if (kq <= 16) hipLaunchKernelGGL((nn_local_kernel<T, 16>), grid, block, 0, s, P, x, y, q, c, c, q0, nbr, bad, (T*)mo.p, (T*)vo.p);
      else if (kq <= 32) hipLaunchKernelGGL((nn_local_kernel<T, 32>), grid, block, 0, s, P, x, y, q, c, c, q0, nbr, bad, (T*)mo.p, (T*)vo.p);
      else hipLaunchKernelGGL((nn_local_kernel<T, 64>), grid, block, 0, s, P, x, y, q, c, c, q0, nbr, bad, (T*)mo.p, (T*)vo.p);
    });
    KCHECK(ctx, "nn_local");
    if (mean_out) HIPC(ctx, hipMemcpyAsync(static_cast<char*>(mean_out) + size_t(q0) * es, mo.p, size_t(c) * es, hipMemcpyDeviceToHost, s));
    if (var_out) HIPC(ctx, hipMemcpyAsync(static_cast<char*>(var_out) + size_t(q0) * es, vo.p, size_t(c) * es, hipMemcpyDeviceToHost, s));
    if (nbr_out)
      for (int t = 0; t < kq; ++t)
        HIPC(ctx, hipMemcpyAsync(nbr_out + size_t(t) * n + q0, tab.as<int>() + size_t(t) * c, size_t(c) * 4, hipMemcpyDeviceToHost, s));
  }
  int badv = 0;
  HIPC(ctx, hipMemcpyAsync(&badv, nn->bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPC(ctx, hipStreamSynchronize(s));   // also: the round buffers are released on return
  if (badv != kNnNone)
    return fail(ctx, SVGP_NOT_POSDEF, "NearestNeighbors: the block of test point " + std::to_string(badv) + " is not positive");
  return SVGP_OK;
}

}  // extern "C"
