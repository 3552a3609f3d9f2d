// natgrad.hip — one natural-gradient step on q(u) (svgp_natgrad_step / _ext): the M-sized kernels that are NOT the data pass.  The data
// pass is svgp_elbo_grad's, unchanged (api_grad.hip: grad_enqueue_impl): it leaves the split-K slices of A diag(2 scale g_v) A' in the
// gradient's slice buffer and scale A g_mu in its avec.  In whitened coordinates, q(v) = N(m_w, S_w), S_w = B B', Lambda = inv(S_w),
// W = A diag(-2 scale g_v) A', a = scale A g_mu, step length gamma in (0, 1]  (the reference's ELBO, SVA:340-373, in the natural
// parameters theta = (Lambda m_w, -Lambda / 2) and the expectation parameters eta = (m_w, S_w + m_w m_w'): theta' = theta + gamma dL/d eta):
//   Lambda'      = (1 - gamma) Lambda     + gamma (I + W)
//   Lambda' m_w' = (1 - gamma) Lambda m_w + gamma (a + W m_w)   =  Lambda' m_w - gamma m_w + gamma a
//   S_w'         = inv(Lambda')
//   W (fp64, full, exactly symmetric) = - sum of the SYRK's slices, in slice order                  natgrad_gather_w_kernel
//   B, m_w widened to fp64 (identity on the padding), first non-positive diagonal entry of B        natgrad_widen_kernel, natgrad_diag_check_kernel
//   inv of the 128 x 128 diagonal blocks of B (what launch_linv starts from)                        natgrad_diag_inv_kernel
//   Lambda = B^-T B^-1 from the explicit triangular inverse                                         grad.hip launchers, fp64
//   Lambda', its right-hand side                                                                    natgrad_form_kernel, natgrad_rhs_kernel
//   cholesky(Lambda'), m_w', inv(Lambda'), its factor                                               prep.hip / grad.hip launchers, fp64 (the collapsed tail)
//   whether q may be written, the NaN probes                                                        natgrad_status_kernel
//   q in the model's parametrisation and layout                                                     collapsed.hip: collapsed_write_q_kernel
// The tail runs in fp64 whatever the model's dtype: cond(Lambda') grows with num_data, as cond(B) of the collapsed bound does.  At
// gamma = 1 exactly Lambda is neither formed nor read.  Every sum has a fixed split and a fixed order: bitwise repeatable, no
// floating-point atomics.
#include "device_common.hpp"
#include "kernels.hpp"

namespace svgp {
namespace {

// Wm[r][c] = - sum_s G[s][max(r, c)][min(r, c)] (the lower tiles of every slice, in slice order)
template <typename T>
__global__ void __launch_bounds__(k256) natgrad_gather_w_kernel(const T* __restrict__ G, int nslices, int64_t Mp, double* __restrict__ Wm) {
  const int64_t c = int64_t(blockIdx.x) * k256 + threadIdx.x, r = blockIdx.y;
  if (c >= Mp) return;
  const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
  double v = 0.0;
  for (int s = 0; s < nslices; ++s) v += double(G[int64_t(s) * Mp * Mp + hi * Mp + lo]);
  Wm[r * Mp + c] = -v;
}

// Bw (fp64, column-major, lower; identity on the padding) from U = B' (model dtype, column-major upper: U[j + i Mp] = B[i][j]);
// mw = m_w widened.  Bw may be NULL (gamma = 1: B is not read).  gridDim.y = Mp rows i, threads along the columns j.
template <typename T>
__global__ void __launch_bounds__(k256) natgrad_widen_kernel(const T* __restrict__ U, const T* __restrict__ mp, int64_t M, int64_t Mp,
                                                             double* __restrict__ Bw, double* __restrict__ mw) {
  const int64_t j = int64_t(blockIdx.x) * k256 + threadIdx.x, i = blockIdx.y;
  if (j >= Mp) return;
  if (Bw) {
    double v = 0.0;
    if (i < M) v = j <= i ? double(U[j + i * Mp]) : 0.0;
    else v = i == j ? 1.0 : 0.0;
    Bw[i + j * Mp] = v;
  }
  if (i == 0) mw[j] = j < M ? double(mp[j]) : 0.0;
}

// *first_bad = 0, or the 1-based index of the first diagonal entry of Bw that is not positive (NaN included).  One workgroup.
__global__ void __launch_bounds__(k256) natgrad_diag_check_kernel(const double* __restrict__ Bw, int64_t M, int64_t Mp, int* __restrict__ first_bad) {
  __shared__ int sh[k256];
  int bad = 0x7fffffff;
  for (int64_t i = threadIdx.x; i < M; i += k256)
    if (!(Bw[i * (Mp + 1)] > 0.0) && int(i + 1) < bad) bad = int(i + 1);
  sh[threadIdx.x] = bad;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w && sh[threadIdx.x + w] < sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *first_bad = sh[0] == 0x7fffffff ? 0 : sh[0];
}

// Tm's diagonal block p (column-major, zero above the diagonal) = inv(Bw's diagonal block p): thread j solves column j by forward
// substitution, its column of X in LDS (x[k][j]: conflict-free), the entries of B read at wavefront-uniform addresses.  One workgroup of
// kNB threads per block, kNB x kNB doubles of dynamic LDS.
__global__ void __launch_bounds__(kNB) natgrad_diag_inv_kernel(const double* __restrict__ Bw, int64_t Mp, double* __restrict__ Tm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* x = reinterpret_cast<double*>(smem_raw);
  const int j = threadIdx.x;
  const int64_t o = int64_t(blockIdx.x) * kNB * (Mp + 1);
  const double* Bd = Bw + o;
  for (int i = 0; i < kNB; ++i) {
    double acc = i == j ? 1.0 : 0.0;
    for (int k = 0; k < i; ++k) acc = fma(-Bd[i + int64_t(k) * Mp], x[k * kNB + j], acc);   // x[k][j] = 0 for k < j
    const double v = i < j ? 0.0 : acc / Bd[i + int64_t(i) * Mp];
    x[i * kNB + j] = v;
    Tm[o + i + int64_t(j) * Mp] = v;
  }
}

// Bm (fp64, full, exactly symmetric) = (1 - gamma) Lam + gamma (I + Wm); Lam (the full product B^-T B^-1, read at (max, min)) is NULL at
// gamma = 1 and then not read
__global__ void __launch_bounds__(k256) natgrad_form_kernel(const double* __restrict__ Lam, const double* __restrict__ Wm, int64_t Mp, double gamma,
                                                            double* __restrict__ Bm) {
  const int64_t c = int64_t(blockIdx.x) * k256 + threadIdx.x, r = blockIdx.y;
  if (c >= Mp) return;
  const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
  double v = gamma * ((r == c ? 1.0 : 0.0) + Wm[r * Mp + c]);
  if (Lam) v = fma(1.0 - gamma, Lam[hi * Mp + lo], v);
  Bm[r * Mp + c] = v;
}

// cvec[r] = sum_c Bm[c][r] mw[c] - gamma mw[r] + gamma a[r]  (Bm symmetric: read along its rows, coalesced).  Thread (r, g) sums
// c = g, g + 4, ..; the four partial sums meet in a fixed order.  64 rows per workgroup.
__global__ void __launch_bounds__(k256) natgrad_rhs_kernel(const double* __restrict__ Bm, const double* __restrict__ mw, const double* __restrict__ a,
                                                           int64_t Mp, double gamma, double* __restrict__ cvec) {
  __shared__ double sh[4][64];
  const int rl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t r = int64_t(blockIdx.x) * 64 + rl;
  double acc = 0.0;
#pragma unroll 4
  for (int64_t c = g; c < Mp; c += 4) acc = fma(Bm[c * Mp + r], mw[c], acc);
  sh[g][rl] = acc;
  __syncthreads();
  if (g == 0) cvec[r] = (((sh[0][rl] + sh[1][rl]) + sh[2][rl]) + sh[3][rl]) - gamma * mw[r] + gamma * a[r];
}

// Closes the step on the device, ahead of collapsed_write_q_kernel, which writes q unless *info_b or *info_s is set and writes NaN when
// scal[0] or scal[1] is NaN:
//   scal[0] = tr W, scal[1] = sum a   (the NaN probes: a NaN coordinate makes every entry of W NaN, a NaN observation every entry of a)
//   scal[4] = *info_b (cholesky(Lambda')), scal[5] = *info_s (cholesky(inv(Lambda'))), scal[6] = *info_q (diagonal of B; nullable),
//   scal[7] = 1 when the value-and-gradient call itself fails and q must stay: Kuu not positive definite (*kuu_info), or a negative
//             predictive variance (gsums[4] > 0) under the error policy.  Then *info_s is set and the probes are cleared: nothing is written.
// One workgroup.
__global__ void __launch_bounds__(k256) natgrad_status_kernel(const double* __restrict__ Wm, const double* __restrict__ a, int64_t Mp,
                                                              const int* __restrict__ info_b, int* __restrict__ info_s,
                                                              const int* __restrict__ info_q, const int* __restrict__ kuu_info,
                                                              const double* __restrict__ gsums, int neg_var_is_error,
                                                              double* __restrict__ scal) {
  __shared__ double sh[2][k256];
  double tw = 0.0, sa = 0.0;
  for (int64_t i = threadIdx.x; i < Mp; i += k256) {
    tw += Wm[i * (Mp + 1)];
    sa += a[i];
  }
  sh[0][threadIdx.x] = tw;
  sh[1][threadIdx.x] = sa;
  __syncthreads();
  for (int w = k256 / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int iq = info_q ? *info_q : 0;
    const bool blocked = *kuu_info != 0 || (neg_var_is_error && gsums[4] > 0.0);
    scal[0] = blocked ? 0.0 : sh[0][0];
    scal[1] = blocked ? 0.0 : sh[1][0];
    scal[2] = scal[3] = 0.0;
    scal[4] = double(*info_b);
    scal[5] = double(*info_s);
    scal[6] = double(iq);
    scal[7] = blocked ? 1.0 : 0.0;
    if (blocked || iq != 0) *info_s = blocked ? -1 : iq;
  }
}

}  // namespace

void launch_natgrad_gather_w(int dtype, hipStream_t s, const void* G, int nslices, int64_t Mp, double* Wm) {
  const dim3 grid((unsigned)((Mp + k256 - 1) / k256), (unsigned)Mp);
  if (dtype == 0) hipLaunchKernelGGL(natgrad_gather_w_kernel<double>, grid, dim3(k256), 0, s, (const double*)G, nslices, Mp, Wm);
  else hipLaunchKernelGGL(natgrad_gather_w_kernel<float>, grid, dim3(k256), 0, s, (const float*)G, nslices, Mp, Wm);
}

void launch_natgrad_widen(int dtype, hipStream_t s, const void* U, const void* mp, int64_t M, int64_t Mp, double* Bw, double* mw) {
  const dim3 grid((unsigned)((Mp + k256 - 1) / k256), (unsigned)(Bw ? Mp : 1));
  if (dtype == 0) hipLaunchKernelGGL(natgrad_widen_kernel<double>, grid, dim3(k256), 0, s, (const double*)U, (const double*)mp, M, Mp, Bw, mw);
  else hipLaunchKernelGGL(natgrad_widen_kernel<float>, grid, dim3(k256), 0, s, (const float*)U, (const float*)mp, M, Mp, Bw, mw);
}

void launch_natgrad_diag_check(hipStream_t s, const double* Bw, int64_t M, int64_t Mp, int* first_bad) {
  hipLaunchKernelGGL(natgrad_diag_check_kernel, dim3(1), dim3(k256), 0, s, Bw, M, Mp, first_bad);
}

void launch_natgrad_diag_inv(hipStream_t s, const double* Bw, int64_t Mp, double* Tm) {
  constexpr int lds = kNB * kNB * int(sizeof(double));
  set_max_lds(reinterpret_cast<const void*>(natgrad_diag_inv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(natgrad_diag_inv_kernel, dim3((unsigned)(Mp / kNB)), dim3(kNB), lds, s, Bw, Mp, Tm);
}

void launch_natgrad_form(hipStream_t s, const double* Lam, const double* Wm, int64_t Mp, double gamma, double* Bm) {
  const dim3 grid((unsigned)((Mp + k256 - 1) / k256), (unsigned)Mp);
  hipLaunchKernelGGL(natgrad_form_kernel, grid, dim3(k256), 0, s, Lam, Wm, Mp, gamma, Bm);
}

void launch_natgrad_rhs(hipStream_t s, const double* Bm, const double* mw, const double* a, int64_t Mp, double gamma, double* cvec) {
  hipLaunchKernelGGL(natgrad_rhs_kernel, dim3((unsigned)(Mp / 64)), dim3(k256), 0, s, Bm, mw, a, Mp, gamma, cvec);
}

void launch_natgrad_status(hipStream_t s, const double* Wm, const double* a, int64_t Mp, const int* info_b, int* info_s, const int* info_q,
                           const int* kuu_info, const double* gsums, int neg_var_is_error, double* scal) {
  hipLaunchKernelGGL(natgrad_status_kernel, dim3(1), dim3(k256), 0, s, Wm, a, Mp, info_b, info_s, info_q, kuu_info, gsums, neg_var_is_error, scal);
}

}  // namespace svgp
