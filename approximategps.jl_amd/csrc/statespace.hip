// statespace.hip — the kernels of the exact one-dimensional Matern GP in O(N) (svgp_ss_*): a Kalman filter and a Rauch-Tung-Striebel
// smoother as two associative scans over small dense elements (Sarkka & Garcia-Fernandez 2021; statespace.hpp: the algebra).
// A scan over n elements is three launches:
//   reduce     every workgroup builds (level 1: from the points; above: loads) the <= 64 elements of its tile, one per lane, combines
//              them across the wavefront with 6 shuffle steps and writes the tile's aggregate
//   aggregates the same scan over the ceil(n / 64) aggregates, in place: one workgroup when they fit its tile, otherwise recursively
//              reduce / aggregates / downsweep one level up
//   downsweep  every workgroup rebuilds and scans its tile as before, prepends the aggregate of all tiles before it and writes results
// No workgroup waits for another inside a launch.  The tile is 64 elements at every level and the tiling a function of n alone, every
// combination happens in a fixed order: results are bitwise repeatable.  Elements live in registers (up to 27 doubles, the triangles of the
// symmetric blocks only) and are kept component-major in memory, so a wavefront's loads and stores of one component are contiguous.
// The tile is one wavefront so that the recursive level is reached from ~4000 points on, where a dense reference can still check it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.hpp"
#include "statespace.hpp"

namespace svgp {
namespace {
using namespace ss;

template <class E> __device__ __forceinline__ E load_elem(const double* __restrict__ buf, int64_t ld, int64_t i) {
  E e;
#pragma unroll
  for (int c = 0; c < E::NV; ++c) e.v[c] = buf[c * ld + i];
  return e;
}
template <class E> __device__ __forceinline__ void store_elem(double* __restrict__ buf, int64_t ld, int64_t i, const E& e) {
#pragma unroll
  for (int c = 0; c < E::NV; ++c) buf[c * ld + i] = e.v[c];
}

// inclusive scan over the wavefront's 64 lanes, lane order = scan order.  Every lane takes part in every shuffle
template <class E> __device__ __forceinline__ E wave_scan(E e, int lane) {
#pragma unroll 1
  for (int off = 1; off < kTile; off <<= 1) {
    E o;
#pragma unroll
    for (int c = 0; c < E::NV; ++c) o.v[c] = __shfl_up(e.v[c], (unsigned)off, kTile);
    if (lane >= off) e = E::combine(o, e);
  }
  return e;
}

// what a tile does with its scanned elements.  REDUCE: the last lane holds the aggregate.  DOWN: prepend the aggregate of the tiles before
enum { REDUCE = 0, DOWN = 1 };

template <class E, int MODE>
__device__ __forceinline__ E tile_finish(E e, int lane, int64_t tile, double* __restrict__ agg, int64_t nagg) {
  e = wave_scan(e, lane);
  if (MODE == REDUCE) {
    if (lane == kTile - 1) store_elem<E>(agg, nagg, tile, e);
  } else if (agg != nullptr && tile > 0) {
    e = E::combine(load_elem<E>(agg, nagg, tile - 1), e);
  }
  return e;
}

// level 1 of the filter's scan over points [0, n): fm (DOWN) gets the filtered mean (D rows) and covariance triangle per point
template <int D, int MODE>
__global__ void __launch_bounds__(kTile) ss_filter_kernel(Model m, const double* __restrict__ t, const double* __restrict__ dl,
                                                          const double* __restrict__ r, int64_t n, double* __restrict__ agg, int64_t nagg,
                                                          double* __restrict__ fm, int64_t ld) {
  using E = FiltElem<D>;
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x, k = tile * kTile + lane;
  E e = E::identity();
  if (k < n) e = E::build(m, k == 0, k == 0 ? 0.0 : t[k] - t[k - 1], dl[k], r[k]);
  e = tile_finish<E, MODE>(e, lane, tile, agg, nagg);
  if (MODE == DOWN && k < n) {
#pragma unroll
    for (int c = 0; c < D + E::TRI; ++c) fm[c * ld + k] = e.v[E::ob + c];   // b then C: contiguous in the element
  }
}

// level 1 of the smoother's scan, position p = point n - 1 - p.  DOWN writes the first entry of the smoothed mean (+ mean_const) and of
// the smoothed covariance where slot[k] >= 0, at that index, in the data dtype
template <int D, int MODE>
__global__ void __launch_bounds__(kTile) ss_smooth_kernel(Model m, const double* __restrict__ t, int64_t n, const double* __restrict__ fm, int64_t ld,
                                                          double* __restrict__ agg, int64_t nagg, const int* __restrict__ slot, double mean_const,
                                                          int f32, void* __restrict__ mean_out, void* __restrict__ var_out) {
  using E = SmoothElem<D>;
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x, p = tile * kTile + lane, k = n - 1 - p;
  E e = E::identity();
  if (p < n) {
    double mk[D], Pk[E::TRI];
#pragma unroll
    for (int c = 0; c < D; ++c) mk[c] = fm[c * ld + k];
#pragma unroll
    for (int c = 0; c < E::TRI; ++c) Pk[c] = fm[(D + c) * ld + k];
    e = E::build(m, k == n - 1, k == n - 1 ? 0.0 : t[k + 1] - t[k], mk, Pk);
  }
  e = tile_finish<E, MODE>(e, lane, tile, agg, nagg);
  if (MODE == DOWN && p < n) {
    const int j = slot[k];
    if (j >= 0) {
      const double mu = e.v[E::og] + mean_const, var = e.v[E::oL];
      if (f32) {
        if (mean_out) static_cast<float*>(mean_out)[j] = float(mu);
        if (var_out) static_cast<float*>(var_out)[j] = float(var);
      } else {
        if (mean_out) static_cast<double*>(mean_out)[j] = mu;
        if (var_out) static_cast<double*>(var_out)[j] = var;
      }
    }
  }
}

// the levels above: stored elements buf [NV][n].  DOWN scans in place (agg NULL: a single tile, nothing to prepend)
template <class E, int MODE>
__global__ void __launch_bounds__(kTile) ss_elem_kernel(double* __restrict__ buf, int64_t n, double* __restrict__ agg, int64_t nagg) {
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x, i = tile * kTile + lane;
  E e = E::identity();
  if (i < n) e = load_elem<E>(buf, n, i);
  e = tile_finish<E, MODE>(e, lane, tile, agg, nagg);
  if (MODE == DOWN && i < n) store_elem<E>(buf, n, i, e);
}

// the log marginal likelihood's point pass: -1/2 (log 2 pi S_k + e_k^2 / S_k) from the one-step prediction at every observed point, a fixed
// number of workgroups of fixed stride, each a fixed tree; ss_sum_kernel adds the partials in a fixed order
constexpr int kLmlThreads = 256, kLmlBlocks = 1024;

__device__ __forceinline__ double block_sum(double s, double* sm) {
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int w = kLmlThreads / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  return sm[0];
}

template <int D>
__global__ void __launch_bounds__(kLmlThreads) ss_lml_kernel(Model m, const double* __restrict__ t, const double* __restrict__ dl,
                                                             const double* __restrict__ r, int64_t n, const double* __restrict__ fm, int64_t ld,
                                                             double* __restrict__ partial) {
  __shared__ double sm[kLmlThreads];
  constexpr int TRI = Dim<D>::TRI;
  double s = 0.0;
  for (int64_t k = int64_t(blockIdx.x) * kLmlThreads + threadIdx.x; k < n; k += int64_t(gridDim.x) * kLmlThreads) {
    const double rk = r[k];
    if (!(rk >= 0.0)) continue;
    double mp[D], Pp[TRI], mu, var;
    if (k > 0) {
#pragma unroll
      for (int c = 0; c < D; ++c) mp[c] = fm[c * ld + k - 1];
#pragma unroll
      for (int c = 0; c < TRI; ++c) Pp[c] = fm[(D + c) * ld + k - 1];
    }
    predict_obs<D>(m, k == 0, k == 0 ? 0.0 : t[k] - t[k - 1], mp, Pp, &mu, &var);
    const double S = var + rk, e = dl[k] - mu;
    s -= 0.5 * (log(6.283185307179586476925 * S) + e * e / S);
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kLmlThreads) ss_sum_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
  __shared__ double sm[kLmlThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += kLmlThreads) s += partial[i];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) out[0] = s;
}

// flag |= 1: a time that is not finite; |= 2: a time below its predecessor
template <typename T> __global__ void ss_check_sorted_kernel(const T* __restrict__ x, int64_t n, int* __restrict__ flag) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = double(x[i]);
  int f = isfinite(v) ? 0 : 1;
  if (i > 0 && v < double(x[i - 1])) f |= 2;
  if (f) atomicOr(flag, f);
}

// the call's points in fp64: t = x, dl = y - mean_const (or the caller's delta), r = diag, or T(diag) + s_i with one rounding in the
// data dtype.  flag |= 4: a noise variance that is not > 0
template <typename T>
__global__ void ss_stage_kernel(const T* __restrict__ x, const T* __restrict__ y, const double* __restrict__ delta, const T* __restrict__ sv,
                                int64_t n, double diag, double mean_const, double* __restrict__ t, double* __restrict__ dl,
                                double* __restrict__ r, int* __restrict__ flag) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  t[i] = double(x[i]);
  dl[i] = delta ? delta[i] : double(y[i]) - mean_const;
  const double rv = sv ? double(T(T(diag) + sv[i])) : diag;
  r[i] = rv;
  if (!(rv > 0.0)) atomicOr(flag, 4);
}

// the union of the N data points and the n sorted test times (unobserved: r = -1), test points behind equal data times; slot: the test
// point's index, -1 for a datum.  Both ranks come from a binary search in the other sorted sequence: a permutation of [0, N + n)
template <typename T>
__global__ void ss_merge_kernel(const double* __restrict__ t, const double* __restrict__ dl, const double* __restrict__ r, int64_t N,
                                const T* __restrict__ ts, int64_t n, double* __restrict__ tm, double* __restrict__ dm, double* __restrict__ rm,
                                int* __restrict__ slot) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= N + n) return;
  if (i < N) {
    const double v = t[i];
    int64_t lo = 0, hi = n;   // the number of test times < v
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (double(ts[mid]) < v) lo = mid + 1; else hi = mid;
    }
    const int64_t pos = i + lo;
    tm[pos] = v; dm[pos] = dl[i]; rm[pos] = r[i]; slot[pos] = -1;
  } else {
    const int64_t j = i - N;
    const double v = double(ts[j]);
    int64_t lo = 0, hi = N;   // the number of data times <= v
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (t[mid] <= v) lo = mid + 1; else hi = mid;
    }
    const int64_t pos = j + lo;
    tm[pos] = v; dm[pos] = 0.0; rm[pos] = -1.0; slot[pos] = int(j);
  }
}

inline unsigned tiles_of(int64_t n) { return (unsigned)((n + kTile - 1) / kTile); }

// the in-place inclusive scan of n stored elements; work: room for the levels above (ss_scan_work_doubles)
template <class E> void scan_stored(hipStream_t s, double* buf, int64_t n, double* work) {
  if (n <= kTile) {
    hipLaunchKernelGGL((ss_elem_kernel<E, DOWN>), dim3(1), dim3(kTile), 0, s, buf, n, (double*)nullptr, int64_t(0));
    return;
  }
  const int64_t m = tiles_of(n);
  hipLaunchKernelGGL((ss_elem_kernel<E, REDUCE>), dim3((unsigned)m), dim3(kTile), 0, s, buf, n, work, m);
  scan_stored<E>(s, work, m, work + m * E::NV);
  hipLaunchKernelGGL((ss_elem_kernel<E, DOWN>), dim3((unsigned)m), dim3(kTile), 0, s, buf, n, work, m);
}

template <int D> void filter_scan(hipStream_t s, const Model& m, const double* t, const double* dl, const double* r, int64_t n, double* work,
                                  double* fm, int64_t ld) {
  using E = FiltElem<D>;
  const int64_t nt = tiles_of(n);
  double* agg = nt > 1 ? work : nullptr;
  if (agg) {
    hipLaunchKernelGGL((ss_filter_kernel<D, REDUCE>), dim3((unsigned)nt), dim3(kTile), 0, s, m, t, dl, r, n, agg, nt, fm, ld);
    scan_stored<E>(s, agg, nt, agg + nt * E::NV);
  }
  hipLaunchKernelGGL((ss_filter_kernel<D, DOWN>), dim3((unsigned)nt), dim3(kTile), 0, s, m, t, dl, r, n, agg, nt, fm, ld);
}

template <int D> void smooth_scan(hipStream_t s, const Model& m, const double* t, int64_t n, const double* fm, int64_t ld, double* work,
                                  const int* slot, double mean_const, int f32, void* mean_out, void* var_out) {
  using E = SmoothElem<D>;
  const int64_t nt = tiles_of(n);
  double* agg = nt > 1 ? work : nullptr;
  if (agg) {
    hipLaunchKernelGGL((ss_smooth_kernel<D, REDUCE>), dim3((unsigned)nt), dim3(kTile), 0, s, m, t, n, fm, ld, agg, nt, slot, mean_const, f32, mean_out, var_out);
    scan_stored<E>(s, agg, nt, agg + nt * E::NV);
  }
  hipLaunchKernelGGL((ss_smooth_kernel<D, DOWN>), dim3((unsigned)nt), dim3(kTile), 0, s, m, t, n, fm, ld, agg, nt, slot, mean_const, f32, mean_out, var_out);
}

inline Model model_of(int family, double variance, double inv_lengthscale) {
  return Model{variance, std::sqrt(family == 1 ? 3.0 : 5.0) * inv_lengthscale};
}

// ---- the sampler (svgp_ss_sample): three scans over AffineElem<D, kSampleChunk> ----------------------------------------------------------
// Grid: x = the tile, y = the chunk of kSampleChunk samples.  Every chunk rebuilds the shared D x D part of its elements (an exp and ~150
// flops a point) instead of reading it, so no chunk depends on another; aggregates of chunk y live at y * stride in the work buffer,
// component-major like the other scans'.  Draws: z [ns][n][D] by point identity (ident[k]: the datum's index, N + the test point's),
// eps [ns][N].  Intermediates: ft [ns][n] (the prior path's first entry), mf [ns][D][n] (the filtered means of the residual).
// kSampleChunk = 4 (profiles/statespace/kernel_resources.txt): the D = 3 element is 9 + 12 doubles and its kernels stay at the
// smoother's register count, without scratch; 8 samples (33 doubles) cost a third of the waves per SIMD for a quarter less shared work,
// in kernels that wait on memory, not on the VALU.
constexpr int kSampleChunk = 4;

// the identity of the union's point at pos: a test point's slot j -> N + j; a datum sits at its index + the number of test times below it
template <typename T>
__global__ void ss_ident_kernel(const double* __restrict__ tm, const int* __restrict__ slot, const T* __restrict__ ts, int64_t n, int64_t N,
                                int* __restrict__ ident) {
  const int64_t pos = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (pos >= N + n) return;
  const int j = slot[pos];
  if (j >= 0) { ident[pos] = int(N + j); return; }
  const double v = tm[pos];
  int64_t lo = 0, hi = n;   // the number of test times < v, as in ss_merge_kernel
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (double(ts[mid]) < v) lo = mid + 1; else hi = mid;
  }
  ident[pos] = int(pos - lo);
}

// level 1 of the prior path's scan.  DOWN writes ft
template <int D, int SC, int MODE>
__global__ void __launch_bounds__(kTile) ss_prior_kernel(Model m, SsSample a, double* __restrict__ agg, int64_t nagg) {
  using E = AffineElem<D, SC>;
  const int lane = threadIdx.x, s0 = blockIdx.y * SC;
  const int64_t tile = blockIdx.x, k = tile * kTile + lane;
  if (agg) agg += int64_t(blockIdx.y) * a.stride;
  E e = E::identity();
  if (k < a.n) {
    double z[D * SC];
    const int64_t row = a.ident[k];
#pragma unroll
    for (int q = 0; q < SC; ++q)
#pragma unroll
      for (int i = 0; i < D; ++i) z[i * SC + q] = s0 + q < a.ns ? a.z[(int64_t(s0 + q) * a.n + row) * D + i] : 0.0;
    e = E::build_prior(m, k == 0, k == 0 ? 0.0 : a.t[k] - a.t[k - 1], z);
  }
  e = tile_finish<E, MODE>(e, lane, tile, agg, nagg);
  if (MODE == DOWN && k < a.n) {
#pragma unroll
    for (int q = 0; q < SC; ++q)
      if (s0 + q < a.ns) a.ft[int64_t(s0 + q) * a.n + k] = e.v[E::oc + q];
  }
}

// level 1 of the scan of the residual's filtered means: the gain from the filtered covariance of point k - 1.  DOWN writes mf
template <int D, int SC, int MODE>
__global__ void __launch_bounds__(kTile) ss_fmean_kernel(Model m, SsSample a, double* __restrict__ agg, int64_t nagg) {
  using E = AffineElem<D, SC>;
  const int lane = threadIdx.x, s0 = blockIdx.y * SC;
  const int64_t tile = blockIdx.x, k = tile * kTile + lane;
  if (agg) agg += int64_t(blockIdx.y) * a.stride;
  E e = E::identity();
  if (k < a.n) {
    double Pp[E::TRI], ft[SC], eps[SC];
#pragma unroll
    for (int c = 0; c < E::TRI; ++c) Pp[c] = k > 0 ? a.fm[(D + c) * a.n + k - 1] : 0.0;
    const double rk = a.r[k];
    const bool obs = rk >= 0.0;
    const int64_t row = a.ident[k];   // < N where obs
#pragma unroll
    for (int q = 0; q < SC; ++q) {
      const bool on = s0 + q < a.ns;
      ft[q] = on ? a.ft[int64_t(s0 + q) * a.n + k] : 0.0;
      eps[q] = on && obs ? a.eps[int64_t(s0 + q) * a.N + row] : 0.0;
    }
    e = E::build_filter(m, k == 0, k == 0 ? 0.0 : a.t[k] - a.t[k - 1], Pp, rk, a.dl[k], ft, eps);
  }
  e = tile_finish<E, MODE>(e, lane, tile, agg, nagg);
  if (MODE == DOWN && k < a.n) {
#pragma unroll
    for (int q = 0; q < SC; ++q)
      if (s0 + q < a.ns) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.mf[(int64_t(s0 + q) * D + i) * a.n + k] = e.v[E::oc + i * SC + q];
      }
  }
}

// level 1 of the scan of the smoothed means, position p = point n - 1 - p.  DOWN writes the path ft + smoothed mean + mean_const of
// every sample at the test points' slots
template <int D, int SC, int MODE>
__global__ void __launch_bounds__(kTile) ss_smean_kernel(Model m, SsSample a, double* __restrict__ agg, int64_t nagg) {
  using E = AffineElem<D, SC>;
  const int lane = threadIdx.x, s0 = blockIdx.y * SC;
  const int64_t tile = blockIdx.x, p = tile * kTile + lane, k = a.n - 1 - p;
  if (agg) agg += int64_t(blockIdx.y) * a.stride;
  E e = E::identity();
  if (p < a.n) {
    double Pk[E::TRI], mk[D * SC];
#pragma unroll
    for (int c = 0; c < E::TRI; ++c) Pk[c] = a.fm[(D + c) * a.n + k];
#pragma unroll
    for (int q = 0; q < SC; ++q)
#pragma unroll
      for (int i = 0; i < D; ++i) mk[i * SC + q] = s0 + q < a.ns ? a.mf[(int64_t(s0 + q) * D + i) * a.n + k] : 0.0;
    e = E::build_smooth(m, k == a.n - 1, k == a.n - 1 ? 0.0 : a.t[k + 1] - a.t[k], Pk, mk);
  }
  e = tile_finish<E, MODE>(e, lane, tile, agg, nagg);
  if (MODE == DOWN && p < a.n) {
    const int j = a.slot[k];
    if (j >= 0) {
#pragma unroll
      for (int q = 0; q < SC; ++q)
        if (s0 + q < a.ns) {
          const double f = a.ft[int64_t(s0 + q) * a.n + k] + e.v[E::oc + q] + a.mean_const;
          if (a.f32) static_cast<float*>(a.out)[int64_t(s0 + q) * a.nt + j] = float(f);
          else static_cast<double*>(a.out)[int64_t(s0 + q) * a.nt + j] = f;
        }
    }
  }
}

// the levels above, per chunk: ss_elem_kernel over the chunk's stored elements at blockIdx.y * stride
template <class E, int MODE>
__global__ void __launch_bounds__(kTile) ss_chunk_elem_kernel(double* __restrict__ buf, int64_t n, double* __restrict__ agg, int64_t nagg,
                                                              int64_t stride) {
  const int lane = threadIdx.x;
  const int64_t tile = blockIdx.x, i = tile * kTile + lane;
  buf += int64_t(blockIdx.y) * stride;
  if (agg) agg += int64_t(blockIdx.y) * stride;
  E e = E::identity();
  if (i < n) e = load_elem<E>(buf, n, i);
  e = tile_finish<E, MODE>(e, lane, tile, agg, nagg);
  if (MODE == DOWN && i < n) store_elem<E>(buf, n, i, e);
}

template <class E> void scan_stored_chunks(hipStream_t s, double* buf, int64_t n, double* work, int64_t stride, unsigned chunks) {
  if (n <= kTile) {
    hipLaunchKernelGGL((ss_chunk_elem_kernel<E, DOWN>), dim3(1, chunks), dim3(kTile), 0, s, buf, n, (double*)nullptr, int64_t(0), stride);
    return;
  }
  const int64_t m = tiles_of(n);
  hipLaunchKernelGGL((ss_chunk_elem_kernel<E, REDUCE>), dim3((unsigned)m, chunks), dim3(kTile), 0, s, buf, n, work, m, stride);
  scan_stored_chunks<E>(s, work, m, work + m * E::NV, stride, chunks);
  hipLaunchKernelGGL((ss_chunk_elem_kernel<E, DOWN>), dim3((unsigned)m, chunks), dim3(kTile), 0, s, buf, n, work, m, stride);
}

#define SS_SAMPLE_SCAN(KERNEL)                                                                                              \
  do {                                                                                                                      \
    if (agg) {                                                                                                              \
      hipLaunchKernelGGL((KERNEL<D, kSampleChunk, REDUCE>), grid, dim3(kTile), 0, s, m, a, agg, nt);                         \
      scan_stored_chunks<E>(s, agg, nt, agg + nt * E::NV, a.stride, chunks);                                                \
    }                                                                                                                       \
    hipLaunchKernelGGL((KERNEL<D, kSampleChunk, DOWN>), grid, dim3(kTile), 0, s, m, a, agg, nt);                             \
  } while (0)

template <int D> void sample_scans(hipStream_t s, const Model& m, const SsSample& a) {
  using E = AffineElem<D, kSampleChunk>;
  const int64_t nt = tiles_of(a.n);
  const unsigned chunks = (unsigned)((a.ns + kSampleChunk - 1) / kSampleChunk);
  const dim3 grid((unsigned)nt, chunks);
  double* agg = nt > 1 ? a.work : nullptr;
  SS_SAMPLE_SCAN(ss_prior_kernel);
  SS_SAMPLE_SCAN(ss_fmean_kernel);
  SS_SAMPLE_SCAN(ss_smean_kernel);
}
#undef SS_SAMPLE_SCAN

}  // namespace

int ss_tile() { return ss::kTile; }

int ss_scan_levels(int64_t n) {
  int levels = 1;
  for (int64_t m = tiles_of(n); m > 1; m = tiles_of(m)) {
    ++levels;
    if (m <= ss::kTile) break;
  }
  return levels;
}

size_t ss_scan_work_doubles(int64_t n) {
  size_t total = 0;
  for (int64_t m = tiles_of(n); m > 1; m = tiles_of(m)) {
    total += size_t(m) * ss::FiltElem<3>::NV;
    if (m <= ss::kTile) break;
  }
  return total + 1;
}

void launch_ss_check_sorted(int dtype, hipStream_t s, const void* x, int64_t n, int* flag) {
  const dim3 g((unsigned)((n + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(ss_check_sorted_kernel<double>, g, dim3(256), 0, s, (const double*)x, n, flag);
  else hipLaunchKernelGGL(ss_check_sorted_kernel<float>, g, dim3(256), 0, s, (const float*)x, n, flag);
}

void launch_ss_stage(int dtype, hipStream_t s, const void* x, const void* y, const double* delta, const void* sv, int64_t n, double diag,
                     double mean_const, double* t, double* dl, double* r, int* flag) {
  const dim3 g((unsigned)((n + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(ss_stage_kernel<double>, g, dim3(256), 0, s, (const double*)x, (const double*)y, delta, (const double*)sv, n, diag, mean_const, t, dl, r, flag);
  else hipLaunchKernelGGL(ss_stage_kernel<float>, g, dim3(256), 0, s, (const float*)x, (const float*)y, delta, (const float*)sv, n, diag, mean_const, t, dl, r, flag);
}

void launch_ss_merge(int dtype, hipStream_t s, const double* t, const double* dl, const double* r, int64_t N, const void* ts, int64_t n,
                     double* tm, double* dm, double* rm, int* slot) {
  const dim3 g((unsigned)((N + n + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(ss_merge_kernel<double>, g, dim3(256), 0, s, t, dl, r, N, (const double*)ts, n, tm, dm, rm, slot);
  else hipLaunchKernelGGL(ss_merge_kernel<float>, g, dim3(256), 0, s, t, dl, r, N, (const float*)ts, n, tm, dm, rm, slot);
}

void launch_ss_filter(hipStream_t s, int family, double variance, double inv_lengthscale, const double* t, const double* dl, const double* r,
                      int64_t n, double* work, double* fm, int64_t ld) {
  const Model m = model_of(family, variance, inv_lengthscale);
  if (family == 1) filter_scan<2>(s, m, t, dl, r, n, work, fm, ld);
  else filter_scan<3>(s, m, t, dl, r, n, work, fm, ld);
}

void launch_ss_lml(hipStream_t s, int family, double variance, double inv_lengthscale, const double* t, const double* dl, const double* r,
                   int64_t n, const double* fm, int64_t ld, double* partial, double* out) {
  const Model m = model_of(family, variance, inv_lengthscale);
  const int nb = (int)std::min<int64_t>(kLmlBlocks, (n + kLmlThreads - 1) / kLmlThreads);
  if (family == 1) hipLaunchKernelGGL(ss_lml_kernel<2>, dim3(nb), dim3(kLmlThreads), 0, s, m, t, dl, r, n, fm, ld, partial);
  else hipLaunchKernelGGL(ss_lml_kernel<3>, dim3(nb), dim3(kLmlThreads), 0, s, m, t, dl, r, n, fm, ld, partial);
  hipLaunchKernelGGL(ss_sum_kernel, dim3(1), dim3(kLmlThreads), 0, s, partial, nb, out);
}

void launch_ss_smooth(hipStream_t s, int family, double variance, double inv_lengthscale, const double* t, int64_t n, const double* fm, int64_t ld,
                      double* work, const int* slot, double mean_const, int dtype, void* mean_out, void* var_out) {
  const Model m = model_of(family, variance, inv_lengthscale);
  if (family == 1) smooth_scan<2>(s, m, t, n, fm, ld, work, slot, mean_const, dtype == 1, mean_out, var_out);
  else smooth_scan<3>(s, m, t, n, fm, ld, work, slot, mean_const, dtype == 1, mean_out, var_out);
}

int ss_sample_chunk() { return kSampleChunk; }

size_t ss_sample_work_doubles(int64_t n) {
  size_t total = 0;
  for (int64_t m = tiles_of(n); m > 1; m = tiles_of(m)) {
    total += size_t(m) * ss::AffineElem<3, kSampleChunk>::NV;
    if (m <= ss::kTile) break;
  }
  return total + 1;
}

void launch_ss_ident(int dtype, hipStream_t s, const double* tm, const int* slot, const void* ts, int64_t n, int64_t N, int* ident) {
  const dim3 g((unsigned)((N + n + 255) / 256));
  if (dtype == 0) hipLaunchKernelGGL(ss_ident_kernel<double>, g, dim3(256), 0, s, tm, slot, (const double*)ts, n, N, ident);
  else hipLaunchKernelGGL(ss_ident_kernel<float>, g, dim3(256), 0, s, tm, slot, (const float*)ts, n, N, ident);
}

void launch_ss_sample(hipStream_t s, int family, double variance, double inv_lengthscale, SsSample a) {
  const Model m = model_of(family, variance, inv_lengthscale);
  a.stride = (int64_t)ss_sample_work_doubles(a.n);
  if (family == 1) sample_scans<2>(s, m, a);
  else sample_scans<3>(s, m, a);
}

}  // namespace svgp
