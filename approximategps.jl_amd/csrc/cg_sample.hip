// cg_sample.hip — pathwise function samples of the exact GP and their input gradients (svgp_cg_sampler_*: cg_api.hip holds the host side).
//   f_s(x) = mean_const + sum_l phi_l(x) w_sl + sum_j k(x, X_j) V_js,      V_s = Khat^-1 (delta - Phi(X) w_s - sigma eps_s)
//   d f_s / d x_c = invl_c [ - sum_l sin(phase_l) omega_lc amp w_sl + 2 sum_j g(r_j^2) (xs_c - Xs_jc) V_js ]
// cg_sample_kernel walks the L features against the resident amp W (sample_eval_kernel's feature chunks: same phase, same kcos), then
// the N data rows against the global N x S panel V (kmv_kernel's chunks): every 16 x 16 tile is generated TRANSPOSED on the MFMA, the
// function is applied in registers and the C/D registers are the B operand of the second product.  No tile reaches LDS or memory; the
// fp32 d <= 8 by-differences path of both kernels is kept.  The gradient form (CB > 0) follows sample_grad_kernel: cos and -sin, kappa
// and 2 g from one argument, the coordinate difference per ENTRY before the product, no division by r; its value chain is the value
// form's own, so its values are bitwise the value form's.
// The evaluation that matters is a few hundred points against 1e5 rows, so the grid is (point workgroups) x (row segments): workgroup
// (bx, seg) walks the chunks of its segment (segment 0 the features first) and writes its partial sums part[seg][slot][point] in the
// data dtype; cg_sample_sum_kernel adds the segments in ascending order in fp64, adds mean_const (scales by invl_c) and rounds once.
// No atomics.  The segmentation is a function of N ALONE (cg_sample_plan), never of the number of points or columns, and a point's
// partial sums come from its own MFMA column: its value and gradient do not depend on the window, the call, the other points or the
// other columns, bitwise.  Points are processed in rounds of cg_sample_plan's `round` points, which bounds the partial buffer.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {

namespace {

// sample.hip's and sample_grad.hip's own (they keep their copies in unnamed namespaces); the sine on its own, as there
__device__ __forceinline__ double kcos(double v) { return cos(v); }
__device__ __forceinline__ float kcos(float v) { return cosf(v); }
__device__ __forceinline__ double ksin(double v) { return sin(v); }
__device__ __forceinline__ float ksin(float v) { return sinf(v); }

constexpr int kCgsKC = 32;   // contraction rows per LDS chunk (Lp, Np and the segments are multiples of it)

// groups of 16 points a wave owns, for two waves per SIMD (<= 256 VGPRs + AGPRs) without spills: profiles/cg/kernel_resources_sample.txt.
// Value form: kmv_kernel's rule (profile 0).  Gradient form: sample_grad_kernel's rule and coordinate block
template <typename T, int DREG, int NSB>
constexpr int cgs_value_groups() {
  return (sizeof(T) == 8 && NSB > 1 && DREG > 32) ? 1 : (DREG > 16 || NSB > 1) ? 2 : 4;
}
template <typename T, int DREG>
constexpr int cgs_coord_block() {
  return (sizeof(T) == 8 && DREG > 32) ? 4 : 8;
}
template <typename T, int DREG>
constexpr int cgs_grad_groups() {
  return (sizeof(T) == 8 || DREG == 8) ? 1 : 2;
}

// One workgroup = 4 waves; a wave owns PG groups of 16 points of the round.  CB == 0, the value form: NSB 16-column blocks of the panels
// (<= 64 columns), partial slot b 16 + row.  CB > 0, the gradient form: one column block and the coordinates e0 .. e0 + CB - 1, slot
// row for the value (written when a.out is asked for, with the first coordinate block) and (1 + e) 16 + row for coordinate e0 + e.
// The data rows hold -2 xs_j (then xs_j = -rows / 2, exact) or, for fp32 with d <= 8 (DIFF), x_j itself (launch_kmv_prep, raw).
template <typename T, int DREG, int NSB, int CB>
__global__ void __launch_bounds__(256, 2) cg_sample_kernel(CgSampleArgs a) {
  constexpr bool GRAD = CB > 0;
  static_assert(!GRAD || NSB == 1, "the gradient form owns one column block");
  constexpr int KS = DREG / 4, KC = kCgsKC, NW = 4, CBR = GRAD ? CB : 1;
  constexpr int PG = GRAD ? cgs_grad_groups<T, DREG>() : cgs_value_groups<T, DREG, NSB>();
  constexpr int ZLD = KC + 16, PLD = NSB * 16 + 4;
  constexpr bool DIFF = sizeof(T) == 4 && DREG <= 8;
  static_assert(!GRAD || !DIFF || DREG <= CB, "the by-differences form keeps every coordinate in one block");
  using acc_t = typename Mfma16<T>::acc_t;
  __shared__ T zc[DREG * ZLD];   // [f][kk]  rows of the chunk (MFMA A operand of the generation)
  __shared__ T pc[KC * PLD];     // [kk][j]  panel rows of the chunk, the launch's column block
  __shared__ T tc[KC];           // [kk]     bias
  const T* __restrict__ invl = static_cast<const T*>(a.invl);
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
  const int d = a.d, family = a.family, e0 = GRAD ? a.e0 : 0;
  const int ne = GRAD ? (d - e0 < CB ? d - e0 : CB) : 0;   // coordinates of this launch
  const bool val = !GRAD || (a.out != nullptr && e0 == 0);
  const int64_t plen = a.p_len, N = a.N;
  const int ncol = int(a.S - a.s0 < NSB * 16 ? a.S - a.s0 : NSB * 16);   // columns of this launch
  const T variance = T(a.variance);
  const int64_t p0 = (int64_t(blockIdx.x) * NW + wave) * (PG * 16);   // within the round
  const int seg = blockIdx.y;
  const int64_t kbeg = int64_t(seg) * a.seg_rows;
  const int64_t kend = kbeg + a.seg_rows < a.Np ? kbeg + a.seg_rows : a.Np;
  const int64_t nfc = seg == 0 ? a.Lp / KC : 0;               // segment 0 takes the features
  T xb[PG][KS], xn[PG];
  T xall[DIFF ? PG : 1][DIFF ? DREG : 1];                  // DIFF: every feature of point c, unscaled
  T il[DIFF ? DREG : 1];
  [[maybe_unused]] T xsb[(GRAD && !DIFF) ? PG : 1][(GRAD && !DIFF) ? CB : 1];   // gradient, otherwise: the block's scaled coordinates of point c
  if constexpr (DIFF) {
#pragma unroll
    for (int f = 0; f < DREG; ++f) il[f] = (f < d) ? invl[f] : T(0);
  }
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    int64_t pl = p0 + g * 16 + c;
    pl = pl < plen ? pl : plen - 1;
    const int64_t pt = a.off + a.p_base + pl;
    if constexpr (DIFF) {
#pragma unroll
      for (int f = 0; f < DREG; ++f) xall[g][f] = (f < d) ? x[int64_t(f) * a.ldx + pt] : T(0);
    } else if constexpr (GRAD) {
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
  acc_t acc[PG][NSB];
  [[maybe_unused]] acc_t gacc[GRAD ? PG : 1][CBR];
#pragma unroll
  for (int g = 0; g < PG; ++g)
#pragma unroll
    for (int b = 0; b < NSB; ++b) acc[g][b] = acc_t{0, 0, 0, 0};
  if constexpr (GRAD) {
#pragma unroll
    for (int g = 0; g < PG; ++g)
#pragma unroll
      for (int e = 0; e < CB; ++e) gacc[g][e] = acc_t{0, 0, 0, 0};
  }

  // one chunk of 32 rows at k0: features (FEAT) or data rows, never both
  auto chunk = [&](auto featc, const T* __restrict__ rsrc, const T* __restrict__ bsrc, const T* __restrict__ psrc, int64_t rld, int64_t pld,
                   int64_t k0) {
    constexpr bool feat = decltype(featc)::value;
    const int64_t plim = pld;   // rows of the panel that exist: Lp (zero-padded) or N
    __syncthreads();   // the previous chunk has been read
    for (int idx = tid; idx < DREG * KC; idx += 256) {
      const int f = idx / KC, kk = idx % KC;
      zc[f * ZLD + kk] = (f < d) ? rsrc[int64_t(f) * rld + k0 + kk] : T(0);
    }
    for (int idx = tid; idx < KC * NSB * 16; idx += 256) {   // the panels are column-major: kk runs fastest over the threads
      const int j = idx / KC, kk = idx % KC;
      pc[kk * PLD + j] = (j < ncol && (feat || k0 + kk < plim)) ? psrc[int64_t(j) * pld + k0 + kk] : T(0);
    }
    if (tid < KC) tc[tid] = bsrc[k0 + tid];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < KC / 16; ++h) {
      T za[KS], pa[4][NSB], tb[4];
      int kr[4];
#pragma unroll
      for (int q = 0; q < KS; ++q) za[q] = zc[(4 * q + kq) * ZLD + h * 16 + c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        kr[r] = h * 16 + Mfma16<T>::row(lane, r);   // the row this lane's register r holds after the generation
        tb[r] = tc[kr[r]];
#pragma unroll
        for (int b = 0; b < NSB; ++b) pa[r][b] = pc[kr[r] * PLD + b * 16 + c];
      }
      [[maybe_unused]] T zr[DIFF ? 4 : 1][DIFF ? DREG : 1];   // DIFF: every feature of the lane's four rows (the data chunk holds x itself)
      if constexpr (DIFF && !feat) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int f = 0; f < DREG; ++f) zr[r][f] = zc[f * ZLD + kr[r]];
      }
#pragma unroll
      for (int g = 0; g < PG; ++g) {
        if (p0 + g * 16 >= plen) break;   // wave-uniform
        acc_t t;
        [[maybe_unused]] T dfr[(GRAD && DIFF) ? 4 : 1][(GRAD && DIFF) ? DREG : 1];   // DIFF: (x_f - X_f) invl_f of the lane's four entries
        if constexpr (DIFF && !feat) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T s2 = T(0);
#pragma unroll
            for (int f = 0; f < DREG; ++f) {
              const T df = (xall[g][f] - zr[r][f]) * il[f];
              if constexpr (GRAD) dfr[r][f] = df;
              s2 = fma(df, df, s2);
            }
            t[r] = s2;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = feat ? tb[r] : tb[r] + xn[g];
#pragma unroll
          for (int q = 0; q < KS; ++q) t = Mfma16<T>::mma(za[q], xb[g][q], t);
        }
        acc_t tv;
        [[maybe_unused]] acc_t td;   // the value's tile and the gradient's: cos and -sin, or kappa and 2 g
        if constexpr (feat) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            tv[r] = val ? kcos(t[r]) : T(0);
            if constexpr (GRAD) td[r] = -ksin(t[r]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const T r2 = t[r] < T(0) ? T(0) : t[r];
            tv[r] = kappa<T>(family, r2, variance);
            if constexpr (GRAD) td[r] = kappa_2g<T>(family, r2, variance, tv[r]);
          }
        }
        if (val) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < NSB; ++b) acc[g][b] = Mfma16<T>::mma(pa[r][b], tv[r], acc[g][b]);
        }
        if constexpr (GRAD) {
#pragma unroll
          for (int e = 0; e < CB; ++e) {
            if (e >= ne) break;   // wave-uniform
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              T av = pa[r][0], bv = td[r];
              if constexpr (feat) {
                av *= zc[(e0 + e) * ZLD + kr[r]];   // omega_kc
              } else if constexpr (DIFF) {
                bv *= dfr[r][e < DREG ? e : 0];
              } else {
                bv *= fma(T(0.5), zc[(e0 + e) * ZLD + kr[r]], xsb[g][e]);   // xs_c - Xs_kc from the row -2 Xs_kc, rounded once
              }
              gacc[g][e] = Mfma16<T>::mma(av, bv, gacc[g][e]);
            }
          }
        }
      }
    }
  };
  for (int64_t ci = 0; ci < nfc; ++ci)
    chunk(std::true_type{}, static_cast<const T*>(a.frows), static_cast<const T*>(a.fbias), static_cast<const T*>(a.W) + a.s0 * a.Lp, a.Lp, a.Lp, ci * KC);
  for (int64_t k0 = kbeg; k0 < kend; k0 += KC)
    chunk(std::false_type{}, static_cast<const T*>(a.rows), static_cast<const T*>(a.bias), static_cast<const T*>(a.V) + a.s0 * N, a.Np, N, k0);
  T* __restrict__ o = static_cast<T*>(a.part) + int64_t(seg) * a.nq * plen;   // [segment][slot][point of the round]
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    const int64_t pl = p0 + g * 16 + c;
    if (pl >= plen) continue;
    if (val) {
#pragma unroll
      for (int b = 0; b < NSB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int sl = b * 16 + Mfma16<T>::row(lane, r);
          if (sl < ncol) o[int64_t(sl) * plen + pl] = acc[g][b][r];
        }
    }
    if constexpr (GRAD) {
#pragma unroll
      for (int e = 0; e < CB; ++e) {
        if (e >= ne) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int sl = Mfma16<T>::row(lane, r);
          if (sl < ncol) o[int64_t((1 + e) * 16 + sl) * plen + pl] = gacc[g][e][r];
        }
      }
    }
  }
}

// the segments' partial sums of one slot and point, ascending, in fp64; then mean_const + sum (value) or invl_c sum (gradient), rounded once
template <typename T>
__global__ void cg_sample_sum_kernel(CgSampleArgs a) {
  const int64_t pl = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (pl >= a.p_len) return;
  const bool grad = a.grad != nullptr;
  const int64_t s = a.s0 + (grad ? q % 16 : q);
  if (s >= a.S) return;
  const bool value = !grad || q < 16;
  if (value && grad && !(a.out != nullptr && a.e0 == 0)) return;
  const T* __restrict__ part = static_cast<const T*>(a.part);
  double sum = 0.0;
  for (int g = 0; g < a.nseg; ++g) sum += double(part[(int64_t(g) * a.nq + q) * a.p_len + pl]);
  if (value) {
    static_cast<T*>(a.out)[s * a.ldo + a.p_base + pl] = T(a.mean_const + sum);
  } else {
    const int e = a.e0 + q / 16 - 1;
    static_cast<T*>(a.grad)[(s * a.d + e) * a.ldg + a.p_base + pl] = T(double(static_cast<const T*>(a.invl)[e]) * sum);
  }
}

template <typename T, int DREG>
void launch_cgs_d(hipStream_t s, const CgSampleArgs& a0) {
  CgSampleArgs a = a0;
  constexpr int CB = cgs_coord_block<T, DREG>();
  const bool grad = a.grad != nullptr;
  const int64_t rnd = cg_sample_round(a.round, grad);
  for (int64_t pb = 0; pb < a.len; pb += rnd) {
    a.p_base = pb;
    a.p_len = a.len - pb < rnd ? a.len - pb : rnd;
    const dim3 sgrid((unsigned)((a.p_len + 255) / 256));
    if (!grad) {
      for (int64_t s0 = 0; s0 < a.S; s0 += 64) {   // column blocks of at most 64
        a.s0 = s0;
        a.e0 = 0;
        const int64_t nc = a.S - s0 < 64 ? a.S - s0 : 64;
        const bool one = nc <= 16;
        a.nq = int(nc);
        const int64_t per = 4 * 16 * (one ? cgs_value_groups<T, DREG, 1>() : cgs_value_groups<T, DREG, 4>());   // points per workgroup
        const dim3 grid((unsigned)((a.p_len + per - 1) / per), (unsigned)a.nseg);
        if (one) hipLaunchKernelGGL((cg_sample_kernel<T, DREG, 1, 0>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((cg_sample_kernel<T, DREG, 4, 0>), grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(cg_sample_sum_kernel<T>, dim3(sgrid.x, (unsigned)a.nq), dim3(256), 0, s, a);
      }
    } else {
      const int64_t per = 4 * 16 * cgs_grad_groups<T, DREG>();
      const dim3 grid((unsigned)((a.p_len + per - 1) / per), (unsigned)a.nseg);
      for (int64_t s0 = 0; s0 < a.S; s0 += 16)        // one 16-column block of the panels
        for (int e0 = 0; e0 < a.d; e0 += CB) {        // and one block of coordinates per launch
          a.s0 = s0;
          a.e0 = e0;
          const int ne = a.d - e0 < CB ? a.d - e0 : CB;
          a.nq = 16 * (1 + ne);
          hipLaunchKernelGGL((cg_sample_kernel<T, DREG, 1, CB>), grid, dim3(256), 0, s, a);
          hipLaunchKernelGGL(cg_sample_sum_kernel<T>, dim3(sgrid.x, (unsigned)a.nq), dim3(256), 0, s, a);
        }
    }
  }
}

template <typename T>
void launch_cgs_t(hipStream_t s, const CgSampleArgs& a) {   // the DREG of launch_kmv_p: the data rows' layout follows it
  if (a.d <= 4) launch_cgs_d<T, 4>(s, a);
  else if (a.d <= 8) launch_cgs_d<T, 8>(s, a);
  else if (a.d <= 16) launch_cgs_d<T, 16>(s, a);
  else if (a.d <= 32) launch_cgs_d<T, 32>(s, a);
  else launch_cgs_d<T, 64>(s, a);
}

template <typename T>
__global__ void cg_sample_rhs_kernel(const T* __restrict__ delta, const T* __restrict__ phi, const T* __restrict__ eps, double sigma, int64_t N,
                                     T* __restrict__ B, const T* __restrict__ sig2) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, col = blockIdx.y;
  if (i >= N) return;
  const int64_t o = col * N + i;
  if (sig2) sigma = sqrt(double(sig2[i]));   // per-point noise
  B[o] = T((double(delta[i]) - (phi ? double(phi[o]) : 0.0)) - sigma * double(eps[o]));
}

template <typename T>
__global__ void cg_sample_basis_kernel(const T* __restrict__ omega, const T* __restrict__ tau, const T* __restrict__ w, int d, int64_t L, int64_t Lp,
                                       int64_t j0, double amp, T* __restrict__ frows, T* __restrict__ fbias, T* __restrict__ W) {
  const int64_t l = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (l >= Lp) return;
  const int64_t j = j0 + blockIdx.y;   // j < d: a row of frows; j == d: fbias; j > d: column j - d - 1 of W
  if (j < d) frows[j * Lp + l] = l < L ? omega[l * d + j] : T(0);
  else if (j == d) fbias[l] = l < L ? tau[l] : T(0);
  else W[(j - d - 1) * Lp + l] = l < L ? T(amp * double(w[(j - d - 1) * L + l])) : T(0);
}

}  // namespace

// Segments of 16 chunks (512 rows), at most 1024 of them; rounds of about 2^20 / segments points, between 256 and 4096 (DESIGN 5.13:
// both measured at N = 1e5: 8 / 16 / 32 / 64 chunks and 2^17 / 2^19 / 2^20, profiles/cg/cg_sample_sweep.txt).  A function of N alone
void cg_sample_plan(int64_t N, int64_t* seg_rows, int* nseg, int64_t* round) {
  const int64_t chunks = (N + kCgsKC - 1) / kCgsKC;
  int64_t cps = 16;
  const int64_t cap = (chunks + 1023) / 1024;
  if (cps < cap) cps = cap;
  const int64_t ns = chunks > 0 ? (chunks + cps - 1) / cps : 1;
  int64_t r = (int64_t(1) << 20) / ns / 256 * 256;
  r = r < 256 ? 256 : r > 4096 ? 4096 : r;
  *seg_rows = cps * kCgsKC;
  *nseg = int(ns);
  *round = r;
}

void launch_cg_sample(int dtype, hipStream_t s, const CgSampleArgs& a) {
  if (dtype == 0) launch_cgs_t<double>(s, a); else launch_cgs_t<float>(s, a);
}

void launch_cg_sample_rhs(int dtype, hipStream_t s, const void* delta, const void* phi, const void* eps, double sigma, int64_t N, int64_t S, void* B,
                          const void* sig2) {
  for (int64_t c0 = 0; c0 < S; c0 += 32768) {   // (grid.y limit)
    const int64_t nc = S - c0 < 32768 ? S - c0 : 32768;
    const dim3 g((unsigned)((N + 255) / 256), (unsigned)nc);
    if (dtype == 0) hipLaunchKernelGGL(cg_sample_rhs_kernel<double>, g, dim3(256), 0, s, (const double*)delta, phi ? (const double*)phi + c0 * N : nullptr, (const double*)eps + c0 * N, sigma, N, (double*)B + c0 * N, (const double*)sig2);
    else hipLaunchKernelGGL(cg_sample_rhs_kernel<float>, g, dim3(256), 0, s, (const float*)delta, phi ? (const float*)phi + c0 * N : nullptr, (const float*)eps + c0 * N, sigma, N, (float*)B + c0 * N, (const float*)sig2);
  }
}

void launch_cg_sample_basis(int dtype, hipStream_t s, const void* omega, const void* tau, const void* w, int d, int64_t L, int64_t Lp, int64_t S,
                            double amp, void* frows, void* fbias, void* W) {
  if (Lp < 1) return;
  for (int64_t j0 = 0; j0 < d + 1 + S; j0 += 32768) {   // (grid.y limit)
    const int64_t nj = d + 1 + S - j0 < 32768 ? d + 1 + S - j0 : 32768;
    const dim3 g((unsigned)((Lp + 255) / 256), (unsigned)nj);
    if (dtype == 0) hipLaunchKernelGGL(cg_sample_basis_kernel<double>, g, dim3(256), 0, s, (const double*)omega, (const double*)tau, (const double*)w, d, L, Lp, j0, amp, (double*)frows, (double*)fbias, (double*)W);
    else hipLaunchKernelGGL(cg_sample_basis_kernel<float>, g, dim3(256), 0, s, (const float*)omega, (const float*)tau, (const float*)w, d, L, Lp, j0, amp, (float*)frows, (float*)fbias, (float*)W);
  }
}

}  // namespace svgp
