// Host-visible launch interface of the HIP kernels (implemented in prep.hip / strip.hip).
// dtype: 0 = f64, 1 = f32 (SVGP_F64 / SVGP_F32).  All pointers are device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svgp {

struct KernelParams {
  int family;        // SVGP_KERNEL_*
  int d;
  double variance;
  const void* invl;  // [d] inverse lengthscales, compute dtype
};

constexpr int kLikExternal = -1;
struct LikParams {
  int lik;            // SVGP_LIK_*, or kLikExternal: a likelihood the host evaluated (svgp_elbo_grad_ext) - gh_x / gh_w then hold
                      // the chunk's point gradients dE_i/dmu_i / dE_i/dv_i (unscaled), indexed by the point's position in the chunk
  int gh_n;           // 0 = closed form
  double sigma2;      // likelihood parameter: Gaussian sigma^2, Gamma shape alpha (1 otherwise)
  double digamma_alpha;  // digamma(alpha) for the Gamma likelihood's parameter gradient
  const double* gh_x; // [gh_n] nodes (device)
  const double* gh_w; // [gh_n] weights / sqrt(pi) (device)
  int clamp_neg_var;
  double mean_const;
};

// ---- prep.hip --------------------------------------------------------------------------------
// zs[k][i] = z_k,i * invl[k] for i < M, 0 for M <= i < Mp.  z given per `layout` (SVGP_COLVECS...).
void launch_scale_inputs(int dtype, hipStream_t s, const void* z, int layout, int d, int64_t M, int64_t Mp,
                         const void* invl, void* zs);
// host ColVecs (d x n, point-contiguous) -> feature-major [d][ldx]
void launch_transpose_colvecs(int dtype, hipStream_t s, const void* x_dn, int d, int64_t n, int64_t ldx, void* x_fm);
// Kuu (Mp x Mp col-major): k(z_i, z_j) + jitter*[i==j] on the M x M block, identity on the padding.
void launch_kuu(int dtype, hipStream_t s, const KernelParams& kp, const void* zs, int64_t M, int64_t Mp,
                double jitter, void* Kuu);
// Blocked Cholesky in place (lower).  T receives the inverted 128x128 diagonal blocks AND, since round 3, its panels
// T[I, <I] = -inv(L_II) * L[I, <I] (computed inside the factorisation's own launches); info = 0 or the 1-based order of the
// first non-positive pivot; sync: Mp / 128 zeroed counters (device) for the in-kernel hand-over of the next diagonal block.
// row_events (nullable; Mp / 128 <= potrf_max_row_events() events): event p is recorded on `s` once block row p of T is final
// row hook: called on the host right after row_events[p] is recorded (p = block row of T that has just become final), so that the
// caller can enqueue the work that waits for that event BEHIND the record and still AHEAD of the device (host.hpp: SegRun)
struct RowHook { void (*fn)(void* user, int row) = nullptr; void* user = nullptr; };
void launch_potrf(int dtype, hipStream_t s, void* A, void* T, int64_t Mp, int* info, unsigned* sync, int num_cus, hipEvent_t* row_events = nullptr,
                  const RowHook* hook = nullptr);
int potrf_max_row_events();
// U = Lq' (upper triangular, Mp x Mp col-major, zero padding); also mp[i] = m[i] padded with zeros.
void launch_pack_q(int dtype, hipStream_t s, const void* Lq, const void* m, int64_t M, int64_t Mp, void* U, void* mp);
// scal[0] = sum(Lq.^2 lower), scal[1] = m'm, scal[2] = sum log diag Lq, scal[3] = sum log diag Lk (first M)
void launch_kl_terms(int dtype, hipStream_t s, const void* Lq, const void* m, const void* Lk, int64_t M, int64_t Mp,
                     double* scal);
void launch_pack_q_ld(int dtype, hipStream_t s, const void* Lq, int64_t ldq, const void* m, int64_t M, int64_t Mp, void* U,
                       void* mp);
void launch_kl_terms_ld(int dtype, hipStream_t s, const void* Lq, int64_t ldq, const void* m, const void* Lk, int64_t M,
                        int64_t Mp, double* scal);
// x := L \ x (trans = 0) or L' \ x (trans = 1) for one vector of length Mp, using the inverted diagonal blocks in T
void launch_trsv2(int dtype, hipStream_t s, const void* L, const void* Tm, int64_t Mp, int trans, void* x);
// X := Lk \ X in place for a lower-triangular Mp x Mp column-major X (Centered B = Lk \ Lq, SVA:133)
void launch_trsm_mat(int dtype, hipStream_t s, const void* Tm, int64_t Mp, void* X);
// out (Mp x Mp, ld Mp) = lower triangle of Lq (M x M, ld M), zero elsewhere
void launch_pad_lower(int dtype, hipStream_t s, const void* Lq, int64_t M, int64_t Mp, void* out);
// out[i] = m[i] + shift for i < M, 0 for M <= i < Mp
void launch_shift_vec(int dtype, hipStream_t s, const void* m, double shift, int64_t M, int64_t Mp, void* out);
// out[i] = (m[i] + shift) - mu[i] for i < M, 0 for M <= i < Mp (Centered m - mean_const - muz: svgp_model_set_mean_z)
void launch_shift_sub_vec(int dtype, hipStream_t s, const void* m, double shift, const void* mu, int64_t M, int64_t Mp, void* out);
// copy the lower triangle of the leading M x M block of A (ld Mp) into out (ld M), zero the upper part
void launch_extract_lower(int dtype, hipStream_t s, const void* A, int64_t Mp, int64_t M, void* out);

// ---- strip.hip -------------------------------------------------------------------------------
enum : int { kSegPregen = 1, kSegPhase2 = 2, kSegLoad = 4, kSegStore = 8 };   // StripArgs::seg_flags
struct StripArgs {
  const void* T;     // Mp x Mp col-major: block rows of inv(L_II) * [-L_I,<I | I]
  const void* U;     // Mp x Mp col-major: B' (upper triangular)
  const void* zs;    // [d][Mp] scaled inducing inputs
  const void* mp;    // [Mp] padded mean of q
  const void* x;     // [d][ldx] feature-major inputs
  unsigned* counter; // zeroed before the launch: dynamic strip queue (strips beyond the first gridDim.x)
  void* work;        // grid * Mp * NT elements: per-workgroup A strip
  double* mom_mu;    // [len] posterior mean of every point of the batch      (SVA:250)
  double* mom_var;   // [len] posterior variance, before the 1e-18 of f_post(x) (SVA:251)
  void* A_out;       // nullable: A  = Lk \ Kuf as a k-major [Mp][lda] matrix (predict-cov path)
  void* C_out;       // nullable: B'A
  void* At_out;      // nullable: the same A, point-major [n][Mp] (column-major Julia A): gradient path
  void* Ct_out;      // nullable: B'A point-major
  int64_t lda;
  int64_t ldx, off, len;
  int64_t Mp, M;
  KernelParams kp;
  double mean_const;
  const void* mux;      // nullable: [len] prior mean offsets of the batch's points (data dtype, element j <-> point off + j): the moment
                        // epilogue writes mom_mu[j] = (mean_const + mux[j]) + qm (svgp_*_with_mean)
  // ---- value-and-gradient strips (launch_strip_grad): phase 3 of the same kernel, P = Kuf_bar for the strip's points ----
  const void* R;        // Mp x Mp col-major: Lk^-T (Lq Lq' - I)
  const void* alpha;    // [Mp] Lk^-T m
  void* Pt_out;         // point-major [n][Mp]: the UNSCALED product R A (P = alpha g_mu' + 2 (R A) diag(g_v) is formed by kgrad)
  // (the likelihood gradients g_mu, g_v and the per-block sums come from launch_point_grads, which reads mom_mu / mom_var)
  // ---- segmented forward strips (launch_strip_seg): one launch covers the phase-1 panels [seg_lo, seg_hi) of every strip ----
  int seg_flags;              // kSegPregen 1: generate the Kuf block first; kSegPhase2 2: phase 2 + moments after the panels;
                              // kSegLoad 4 / kSegStore 8: restore / save the threads' fp64 column sums in seg_state
  int seg_lo, seg_hi;
  double* seg_state;          // [nstrips][256][2 NJ]; `work` then holds ONE scratch strip PER STRIP (nstrips x Mp x NT)
  // Split closing launch (segmented strips of a SMALL batch: fewer strips than workgroup slots).  The output panels of phase 3 (value and
  // gradient: dense) and of phase 2 (forward: C_J = sum_{I >= J} U[J, I] A_I) are independent, so the closing launch runs seg_split
  // workgroups per strip - workgroup (strip, part) = blockIdx (part * nstrips + strip) takes the panels [part nP / S, (part + 1) nP / S)
  // of phase 3, or J = part, part + S, .. of phase 2 - and the parts' column sums meet in seg_part ([S][nstrips][3][NT] doubles: sum A^2,
  // mean, variance term); the last part to arrive (seg_cnt[strip], zeroed by the host) adds them in part order and writes the moments.
  // Run-to-run bitwise reproducible; against the unsplit kernel the variance differs by summation order.
  int seg_split;
  double* seg_part;
  unsigned* seg_cnt;
};
int strip_nt(int dtype, int64_t Mp, int64_t len);                 // column-strip width chosen for a problem
size_t strip_work_bytes(int dtype, int64_t Mp, int nt, int grid);  // workspace bytes
int strip_grid(int dtype, int nt, int64_t nstrips, int num_cus);
struct StripPlan {       // regular-width launch over the first `points` points, then an optional half-width tail launch
  int nt, grid;
  int64_t nstrips, points;
  int nt_tail, grid_tail;
  int64_t nstrips_tail;
  bool concurrent_tail;   // the tail launch runs on a second stream BESIDE the main one (last partial round of a large batch)
};
StripPlan strip_plan(int dtype, int64_t Mp, int64_t len, int num_cus);
StripPlan strip_plan_single(int dtype, int64_t Mp, int64_t len, int num_cus);   // never a concurrent tail (paths that write A / C)
void launch_strip(int dtype, hipStream_t s, const StripArgs& a, int nt, int grid, int64_t nstrips);
void launch_strip_seg(int dtype, hipStream_t s, const StripArgs& a, int nt, int grid, int64_t nstrips, bool grad = false);
size_t strip_seg_state_doubles(int dtype, int nt);
// the value-and-gradient form: phase 1 as launch_strip, then phase 3 (a dense Mp x Mp GEMM R A on the strip's A, still in its
// scratch strip, whose epilogue also gives the variance) and the per-point likelihood gradients; writes At_out, Pt_out (R A,
// unscaled), gmu_out, gv_out, part5.  `work` must hold TWO scratch strips per workgroup (2 x strip_work_bytes).
// post = true (round 4): the strips leave their moments in mom_mu / mom_var (like launch_strip) and write no gmu / gv / part5 -
// launch_point_grads, next on the stream, produces those from the moments.  post = false: the round-3 in-kernel forms.
void launch_strip_grad(int dtype, hipStream_t s, const StripArgs& a, int nt, int grid, int64_t nstrips);
// marginals, expected log-likelihood and d E / d (mu, v) (x scale) of the points [off, off + len) of y from their moments: gmu_out /
// gv_out (compute dtype, [len]) and part5[point_grad_blocks(len)][5] = per-block {E, sum g_mu, sum g_v, dE/dsigma2, n_neg}
// gmu_copy (nullable): a second copy of gmu_out[0 .. len) (the prior mean offsets' gradient of svgp_elbo_grad_with_mean)
// the collapsed bound's data pass: phase 1 ALONE (trsm_pm_kernel) - A point-major into a.At_out ([n][Mp]) and sum_k A_kj^2 (fp64) into
// a.mom_var[j]; reads a.T, a.zs, a.x, a.work (ONE scratch strip per workgroup), a.counter; the widths and grids of launch_strip
void launch_trsm_point_major(int dtype, hipStream_t s, const StripArgs& a, int nt, int grid, int64_t nstrips);
int point_grad_blocks(int64_t len);
void launch_point_grads(int dtype, hipStream_t s, const LikParams& lp, const double* mom_mu, const double* mom_var, const void* y,
                        int64_t off, int64_t len, double scale, const double* n_global_dev, double num_data, void* gmu_out,
                        void* gv_out, double* part5, unsigned* strip_queue = nullptr, int64_t pad_to = 0, void* gmu_copy = nullptr);
// marginals + expected log-likelihood of every point (SVA:354-355): per-block sums into partial/negcnt
int expect_blocks(int64_t len);
void launch_expect(int dtype, hipStream_t s, const LikParams& lp, const double* mom_mu, const double* mom_var,
                   const void* y, int64_t off, int64_t len, double* partial, unsigned* negcnt, void* mu_out,
                   void* var_out);
// out[0..8) = {sum(partial[0..n)), n_points, sum(negcnt), *chol_info != 0, 0, 0, 0, 0} in fixed order (deterministic):
// the vector a data-parallel evaluation all-reduces
// out[8..13) (not all-reduced) = this rank's prep scalars prep_scal[0..4) and *chol_info: one read-back per evaluation
void launch_final_reduce(hipStream_t s, const double* partial, const unsigned* negcnt, int64_t n, const int* chol_info,
                         double n_points, double* out, const double* prep_scal);
// predictive.hip: log predictive density and (E[y], Var[y]) of every point from its latent marginal (mom_mu, mom_var + var_shift);
// lp.gh_n is the predictive rule (0: closed form, Gaussian / normcdf Bernoulli only).  part3: [expect_blocks(len)][3] per-block sums,
// sums3[0..3) = {sum lpd, sum (y - E[y])^2, n_neg} in a fixed order.  y (dtype's element type, read at off + i) and each of the
// fp64 per-point outputs may be NULL
void launch_predictive(int dtype, hipStream_t s, const LikParams& lp, const double* mom_mu, const double* mom_var, const void* y,
                       int64_t off, int64_t len, double var_shift, double* part3, double* sums3, double* lpd_out, double* ymean_out,
                       double* yvar_out);
// standalone Kuf (M x len col-major, ld = M)
void launch_kuf(int dtype, hipStream_t s, const KernelParams& kp, const void* zs, int64_t M, int64_t Mp,
                const void* x, int64_t ldx, int64_t off, int64_t len, void* Kuf);
// out(n x n col-major) = kxx - A'A + C'C  from k-major A, C ([Mp][lda]); prior block computed from x.
void launch_cov_assemble(int dtype, hipStream_t s, const KernelParams& kp, const void* xa, int64_t ldxa, int64_t na,
                         const void* xb, int64_t ldxb, int64_t nb, const void* Aa, const void* Ca, int64_t lda,
                         const void* Ab, const void* Cb, int64_t ldb, int64_t Mp, void* out);

// ---- grad.hip (reverse-mode gradient of the NonCentered ELBO) -------------------------------------------
constexpr double kDefaultSigma2 = 1e-18;  // AbstractGPs.default_σ² added by f_post(x) (SVA:354)
int grad_dreg(int d);
int grad_rowblocks(int dtype, int d, int64_t Mp);
void launch_set_f64(hipStream_t s, double* dst, double value);
void launch_setvec_f64(hipStream_t s, double* dst, const double* vals, int n);   // dst[0 .. n) = vals, n <= 64, as kernel arguments (never blocks the host)
void launch_set2_f64(hipStream_t s, double* dst, double a, double b);   // dst[0] = a, dst[1] = b (values travel as kernel arguments: no host buffer to outlive)
// sums[5] = n_points, sums[6] = (*chol_info != 0), sums[7] = 0: the status slots of the all-reduced gradient scalars
// ... and, behind them, a copy of the prep scalars (4) and chol_info (as a double): prep_out[0..5)
void launch_grad_status(hipStream_t s, double* sums, const int* chol_info, double n_points, const double* prep_scal, double* prep_out);
// flags of the M x M x M products (gemm_pm_kernel): all tiles instead of the lower ones; triangular operands (the contraction
// starts / ends at the diagonal tile of the output row (X) or column (Y))
enum : int { kMmFull = 1, kMmXLow = 2, kMmYLow = 4, kMmXUp = 8, kMmYUp = 16 };
void launch_gemm_pm(int dtype, hipStream_t s, const void* Xt, const void* Yt, const void* w, double wscale, int64_t Mp,
                    int64_t n, int64_t slice_len, int nslices, void* out, int overwrite = 0, int flags = 0);
// the data-sized SYRK with UNIFORM weights (Gaussian likelihood): out (+)= wscale * w * scale * At' At over the first n points (slices of
// slice_len); scale = num_data / *n_global_dev when n_global_dev is given.  Rows [n, ceil16(n)) of At must be zero.
void launch_syrk_uniform(int dtype, hipStream_t s, const void* At, double w, double scale, const double* n_global_dev, double num_data,
                         double wscale, int64_t Mp, int64_t n, int64_t slice_len, int nslices, void* out, int overwrite);
// out (lower 128-tiles, or all with full) (+)= the sum of `ns` slice partials written by launch_gemm_pm(..., overwrite = 1)
void launch_sum_slices_lower(int dtype, hipStream_t s, const void* part, int ns, int64_t Mp, void* out, int full = 0, int overwrite = 0);
// Linv = Lk^-1 by recursive doubling from the inverted diagonal blocks in T: LinvRM row-major, LinvCM column-major (only
// the lower block triangle is written / ever read); Ytmp: Mp x Mp scratch
void launch_linv(int dtype, hipStream_t s, const void* L, const void* Tm, int64_t Mp, void* LinvRM, void* LinvCM, void* Ytmp);
// out = Lk^-T v = LinvRM' v; part: (Mp / 128) x Mp doubles of scratch
// vec_f64: v and out are fp64 whatever the matrix dtype (the kernel-gradient reductions keep their sums in fp64)
void launch_linv_t_gemv(int dtype, hipStream_t s, const void* LinvRM, const void* v, int64_t Mp, void* out, double* part, int notrans = 0,
                        int vec_f64 = 0);
// data part: Pt = the strips' unscaled R A, P_ij = alpha_i gmu_j + 2 gv_j Pt_ji formed inside (alpha != nullptr); Kuu part: Pt is
// the matrix itself (alpha = gmu = gv = nullptr); kmb: also the row sums (Kuf g_mu)_i into slot 1 (the caller applies Lk^-1: A g_mu)
void launch_kgrad(int dtype, hipStream_t s, const KernelParams& kp, const void* zs, int64_t Mp, int64_t M, const void* x, int64_t ldx,
                  int64_t xoff, int prescaled, int64_t n, int64_t nvalid, const void* Pt, const void* gmu,
                  const void* gv, const void* alpha, int64_t slice_len, int nslices, double* rowpart, double* scalpart, int kmb = 0);
// d elbo / d x of the chunk's n points from the same P (launch_kgrad's data part): out[f * ldo + ooff + j], j < n, feature-major
void launch_xgrad(int dtype, hipStream_t s, const KernelParams& kp, const void* zs, int64_t Mp, int64_t M, const void* x, int64_t ldx,
                  int64_t xoff, int64_t n, const void* Pt, const void* gmu, const void* gv, const void* alpha, void* out, int64_t ldo,
                  int64_t ooff);
// fused gradient path: sums of the per-strip partials, W = A diag(2 g_v) A' from its split-K lower tiles, (A g_mu), and the
// assembly of Lq_bar / Lk_bar from G1 = 2 W Lq, G2 = 2 R W and the rank-one term alpha (A g_mu)'
void launch_sum5(hipStream_t s, const double* partial, int nblocks, double* sums);
void launch_sym_from_lower(int dtype, hipStream_t s, const void* G, int nslices, int64_t Mp, double eye, void* out);
void launch_avec(hipStream_t s, const double* rp_uf, int ns, int64_t stride, int64_t Mp, double* avec);
void launch_finish_mm2(int dtype, hipStream_t s, const void* G1, const void* G2, const void* alpha, const double* avec, int64_t Mp,
                       int64_t M, const void* Lq, int64_t ldq, double klw, void* Lq_bar, void* BbarRM, void* LkbarRM);
void launch_lower_to_rowmajor(int dtype, hipStream_t s, const void* L, int64_t Mp, void* out);
void launch_symmetrize(int dtype, hipStream_t s, const void* St, int64_t Mp, void* H);
void launch_phi(int dtype, hipStream_t s, void* X, int64_t Mp);
void launch_mbar(int dtype, hipStream_t s, const double* avec, const void* mt, double klw, int64_t M, int64_t Mp, void* vec);
void launch_lbar_adjust(int dtype, hipStream_t s, void* LkbarRM, const void* RBt, const void* rbar, const void* mt, int64_t Mp);
void launch_cm_tril_to_user(int dtype, hipStream_t s, const void* R, int64_t Mp, int64_t M, void* out);   // R column-major
void launch_add_f64(hipStream_t s, double* p, double v);   // *p += v
// {head entries | M x M column-major lower-triangular block} <-> {head entries | its M (M + 1) / 2 packed entries}; dir 0 packs
void launch_pack_tril(int dtype, hipStream_t s, void* gblk, void* packed, int64_t head, int64_t M, int dir);
void launch_finish_kgrad(int dtype, hipStream_t s, int d, int64_t M, int64_t Mp, const void* zs, const double* invl,
                         const double* rp_uf, int ns_uf, const double* rp_uu, int ns_uu, const double* sp_uf, int nsp_uf,
                         const double* sp_uu, int nsp_uu, const void* m, double klw, int layout_z, double variance,
                         void* z_bar, void* m_bar, double* scal_out, double* red, const double* avec);

// ---- collapsed.hip (the collapsed bound and the optimal q: svgp_collapsed_*) ---------------------------------------------
constexpr int kCollapsedSplit = 64;   // point splits of the b / rr / t reductions: a constant, so the summation order never depends on the chip
// bpart[kCollapsedSplit][Mp] (+)= A r, spart[kCollapsedSplit][2] (+)= {r'r, sum ssq} over the n points of the resident point-major
// chunk At ([n][Mp]); r_j = y[off + j] - mean_const; ssq[j] = sum_k A_kj^2 (fp64); first != 0 overwrites
void launch_collapsed_reduce(int dtype, hipStream_t s, const void* At, const void* y, const double* ssq, int64_t Mp, int64_t off, int64_t n,
                             double mean_const, int first, double* bpart, double* spart);
// *first_bad = 0 or the 1-based index of the first pivot of Lk at or below its rounding noise 4 eps (i + 1) kdiag (model dtype's eps)
void launch_collapsed_pivot_check(int dtype, hipStream_t s, const void* Lk, int64_t M, int64_t Mp, double kdiag, int* first_bad);
// Bm (fp64, full) = I + sum(slices of G: the SYRK's lower tiles, model dtype) / sigma2; cvec = b / sigma2; scal[0] = r'r, scal[1] = sum A^2
void launch_collapsed_form_b(int dtype, hipStream_t s, const void* G, int nslices, int64_t Mp, double sigma2, const double* bpart,
                             const double* spart, double* Bm, double* cvec, double* scal);
// scal[2] = sum log diag LB, scal[3] = c'c, scal[4] = *info_b, scal[5] = *info_s (info_s nullable)
void launch_collapsed_scal(hipStream_t s, const double* LB, const double* c, int64_t Mp, const int* info_b, const int* info_s, double* scal);
// the optimal q in the model's parametrisation into m_out [M] / Lq_out (M x M column-major, upper zeroed), model dtype
void launch_collapsed_write_q(int dtype, hipStream_t s, const double* Lqw, const double* mw, const void* Lk, int64_t M, int64_t Mp, int centered,
                              double mean_const, const double* scal, const int* info_b, const int* info_s, const void* muz, void* m_out,
                              void* Lq_out);   // muz (nullable, [M], model dtype): added to the Centered m
// per-point noise (svgp_collapsed_*_with_noise): w[j] = 1 / (sigma2 + sv[j]) for j < n in the model's dtype and in fp64 (wd), zeros
// on [n, pad_to); *nbad (zeroed by the caller) += the number of sigma2 + sv[j] <= 0
void launch_collapsed_weights(int dtype, hipStream_t s, const void* sv, double sigma2, int64_t n, int64_t pad_to, void* w, double* wd, int* nbad);
// launch_collapsed_reduce with r_j = y[off + j] - mean_const - mux[j] and weights wd[j] (mux, sv, wd nullable, indexed by the point's
// place in the chunk): bpart (+)= A (w r), spart (+)= {sum w r^2, sum w ssq}, spart2[kCollapsedSplit][2] (+)= {sum log(sigma2 + sv), sum w}
void launch_collapsed_reduce_w(int dtype, hipStream_t s, const void* At, const void* y, const void* mux, const void* sv, const double* wd,
                               const double* ssq, int64_t Mp, int64_t off, int64_t n, double mean_const, double sigma2, int first,
                               double* bpart, double* spart, double* spart2);
// scal[6] = sum log sigma_j^2, scal[7] = sum w_j from spart2, in split order
void launch_collapsed_extra(hipStream_t s, const double* spart2, double* scal);
// launch_point_grads for the Gaussian likelihood (closed form) with a per-point noise variance: point i is evaluated with
// sigma_i^2 = sigma2 + noise[i] (noise nullable, compute dtype, [len]); the same outputs in the same layout, plus noise_bar[i] =
// scale dE_i/dsigma_i^2 (nullable).  strip.hip stays as it is: the strips' translation unit is not rebuilt differently for this
void launch_point_grads_noise(int dtype, hipStream_t s, double sigma2, int clamp_neg_var, const double* mom_mu, const double* mom_var,
                              const void* y, int64_t off, int64_t len, double scale, const void* noise, void* gmu_out, void* gv_out,
                              double* part5, unsigned* strip_queue, int64_t pad_to, void* gmu_copy, void* noise_bar);

// ---- natgrad.hip (one natural-gradient step on q: svgp_natgrad_step*) -----------------------------------------------------
// Wm (fp64, full, symmetric) = - sum(slices of G: the SYRK's lower tiles of A diag(2 scale g_v) A', model dtype), in slice order
void launch_natgrad_gather_w(int dtype, hipStream_t s, const void* G, int nslices, int64_t Mp, double* Wm);
// Bw (fp64 column-major lower, identity on the padding; NULL: skipped) from U = B' (model dtype); mw = the padded m_w widened
void launch_natgrad_widen(int dtype, hipStream_t s, const void* U, const void* mp, int64_t M, int64_t Mp, double* Bw, double* mw);
// *first_bad = 0 or the 1-based index of the first diagonal entry of Bw that is not positive
void launch_natgrad_diag_check(hipStream_t s, const double* Bw, int64_t M, int64_t Mp, int* first_bad);
// the diagonal 128-blocks of Tm = the inverses of those of the lower-triangular Bw (zero above the diagonal): what launch_linv starts from
void launch_natgrad_diag_inv(hipStream_t s, const double* Bw, int64_t Mp, double* Tm);
// Bm = (1 - gamma) Lam + gamma (I + Wm), full and symmetric; Lam NULL (gamma = 1): not read
void launch_natgrad_form(hipStream_t s, const double* Lam, const double* Wm, int64_t Mp, double gamma, double* Bm);
// cvec = Bm mw - gamma mw + gamma a
void launch_natgrad_rhs(hipStream_t s, const double* Bm, const double* mw, const double* a, int64_t Mp, double gamma, double* cvec);
// scal[0..8) = {tr W, sum a (NaN probes), 0, 0, *info_b, *info_s, *info_q, blocked}; sets *info_s when q must not be written
void launch_natgrad_status(hipStream_t s, const double* Wm, const double* a, int64_t Mp, const int* info_b, int* info_s, const int* info_q,
                           const int* kuu_info, const double* gsums, int neg_var_is_error, double* scal);

// ---- sample.hip (pathwise posterior function samples: svgp_sampler_*) ------------------------------------------------------
// the data stage: out[s * ldo + j] = (mean_const + mux[j]) + sum_k panel[k][s] g_k(x_{off + j}), j < len, s < S, where row k < Lp is the
// feature cos(rows[.][k] . xs + bias[k]) and row Lp + i the kernel value kappa(|xs|^2 + bias + rows[.][k] . xs) of inducing point i
// (xs = invl o x; rows = -2 zs, bias = |zs|^2 there).  Lp and Mp are multiples of 32, Sp = S rounded up to 16; all arrays in `dtype`
struct SampleEvalArgs {
  const void* rows;    // [d][Lp + Mp]
  const void* bias;    // [Lp + Mp]
  const void* panel;   // [Lp + Mp][Sp]: {sqrt(2 variance / L) w | V}, zero on every padding row and column
  const void* invl;    // [d]
  const void* x;       // [d][ldx] feature-major inputs
  const void* mux;     // nullable: [len] prior mean offsets of the window's points
  void* out;
  int64_t ldx, off, len, ldo;
  int64_t Lp, Mp, S, Sp;
  int64_t s0;          // first sample of the launch's column block (set by the launcher)
  int family, d;
  double variance, mean_const;
};
void launch_sample_eval(int dtype, hipStream_t s, const SampleEvalArgs& a);   // one launch per block of <= 64 samples
// sample_grad.hip: grad[(s * d + c) * ldg + j] = d (f_s - mean) / d x_c at x_{off + j}, and, with v.out non-null, the values exactly as
// launch_sample_eval writes them (the same chain: bitwise).  v.mux is read for the values alone
struct SampleGradArgs {
  SampleEvalArgs v;    // v.out nullable: gradient only
  void* grad;
  int64_t ldg;
  int e0;              // first coordinate of the launch's coordinate block (set by the launcher)
};
void launch_sample_grad(int dtype, hipStream_t s, const SampleGradArgs& a);   // one launch per (16 samples, 8 coordinates)
// the M-sized stage, fp64 from the model-dtype inputs (dtype names the type of z, omega, tau, w, eps, m, Lq, muz and of rows / bias / panel)
void launch_sample_widen_z(int dtype, hipStream_t s, const void* z, int layout, int d, int64_t M, int64_t Mp, const double* invl64, double* zs64);
// z, layout, M: the model's own inducing inputs, which the by-differences kernels (fp32, d <= 8) read unscaled
void launch_sample_rows(int dtype, hipStream_t s, const double* zs64, const void* z, int layout, int64_t M, const void* omega, const void* tau, int d,
                        int64_t L, int64_t Lp, int64_t Mp, void* rows, void* bias);
// rhs[s][Mp] = u_s - mean(z) (zero padding), u[s][M] = u_s; tmp: S x Mp doubles of scratch; Lk: the fp64 factor of Kuu (ld Mp)
void launch_sample_u(int dtype, hipStream_t s, const void* m, const void* Lq, const void* eps, const void* muz, const double* Lk, int64_t M,
                     int64_t Mp, int64_t S, int centered, double mean_const, double* tmp, double* rhs, double* u);
// rhs[s][i] -= (Phi(z) w_s)_i, amp = sqrt(2 variance / L)
void launch_sample_phiz(int dtype, hipStream_t s, const double* zs64, const void* omega, const void* tau, const void* w, int d, int64_t M, int64_t L,
                        int64_t S, int64_t Mp, double amp, double* rhs);
void launch_sample_panel(int dtype, hipStream_t s, const void* w, const double* V, int64_t L, int64_t Lp, int64_t M, int64_t Mp, int64_t S, int64_t Sp,
                         double amp, void* panel);

// cg.hip: out[s * ldo + i] = sum_j prof(r^2(P_i, R_j)) V[s * ldv + j] (+ diag addv[s * lda + i]) for the n points P and the N rows R;
// with dvec the added term's factor is per point: + dvec[i] addv[s * lda + i]
struct KmvArgs {
  const void* rows;    // [d][Np] the rows R as launch_kmv_prep wrote them
  const void* bias;    // [Np]
  const void* invl;    // [d]
  const void* px;      // [d][ldp] the points P, feature-major, unscaled
  const void* V;       // N x S panel, column-major
  const void* addv;    // nullable: n x S, column-major
  const void* dvec;    // nullable: [n] the per-point factor of addv (per-point noise), read only with addv; NULL: diag for every point
  void* out;           // n x S, column-major
  int64_t ldp, n, N, Np, ldv, lda, ldo, S;
  int64_t s0;          // first column of the launch's column block (set by the launcher)
  int family, d;
  int profile;         // 0: kappa;  1: 2 g(r^2) (xs_ic - xs_jc)^2 of the coordinate `coord`, g = d kappa / d(r^2)
  int coord;
  int self;            // 1: P is R itself (point i is row i): r^2 of the diagonal is exactly 0
  double variance, diag;
};
void launch_kmv(int dtype, hipStream_t s, const KmvArgs& a);   // one launch per block of <= 64 columns
void launch_kmv_prep(int dtype, hipStream_t s, const void* x, int64_t ldx, const void* invl, int d, int64_t N, int64_t Np, void* rows, void* bias);
// the fp64 state of one column block of the solver (<= 64 columns), on the device
struct CgState {
  enum : int { BB = 0, RR = 64, A = 128, BE = 192, IT = 256, ACT = 320, BAD = 384, WORDS = 392 };   // the host reads [ACT, WORDS) per iteration
};
int cg_dot_blocks(int64_t N);   // blocks of the first stage of a column dot: a function of N alone
// partial[col * cg_dot_blocks(N) + blk] of sum_i a[i, col] b[i, col] (fp64), then their sums blk ascending
void launch_cg_dot(int dtype, hipStream_t s, const void* a, int64_t lda, const void* b, int64_t ldb, int64_t N, int64_t ncols, double* partial);
void launch_cg_colsum(hipStream_t s, const double* partial, int64_t N, int64_t ncols, double* out);
// rho (the preconditioned recurrence, modes 3 - 5 and the step length of mode 1): 128 fp64 words, r'z per column and its initial value
void launch_cg_coef(hipStream_t s, int mode, double* st, const double* partial, int64_t N, int ncols, int k, double tol2, double* hist_a, double* hist_b,
                    double* rho = nullptr);
void launch_cg_update_xr(int dtype, hipStream_t s, const double* st, int64_t N, int ncols, void* x, void* r, const void* p, const void* q);
void launch_cg_update_p(int dtype, hipStream_t s, const double* st, int64_t N, int ncols, const void* r, void* p);
// dst = alpha src + beta, column by column (src in fp64 with src_f64, otherwise in the data dtype)
void launch_cg_affine(int dtype, hipStream_t s, const void* src, int src_f64, int64_t lds, int64_t N, int64_t ncols, double alpha, double beta, void* dst, int64_t ldd);
void launch_cg_kcols(int dtype, hipStream_t s, const void* x, int64_t ldx, int64_t N, const void* xt, int64_t ldt, int64_t nt, const void* invl, int d,
                     int family, double variance, void* out, int64_t ldo);
// the Nystrom preconditioner.  launch_kmv_split: launch_kmv (profile 0, no addv) for FEW points a.n against the N rows, the rows split
// into kmv_split_segments(N, n) segments of *seg_rows rows (whole chunks; a function of N and n alone); part: segments x 64 x n elements
int kmv_split_segments(int64_t N, int64_t n, int64_t* seg_rows);
void launch_kmv_split(int dtype, hipStream_t s, const KmvArgs& a, void* part);
// its k-sized stage, fp64 whatever the data dtype (kernels of cg.hip; the factorisations are launch_kuu / _potrf / _linv / _gemm_pm)
void launch_cg_widen(int dtype, hipStream_t s, const void* src, int64_t lds, int64_t n, int64_t ncols, double* dst, int64_t ldd);
void launch_cg_pc_scale(hipStream_t s, const double* z, int64_t ldz, const double* invl, int d, int64_t k, int64_t Mp, double* zs);
void launch_cg_pc_form_b(hipStream_t s, const double* A, int64_t Mp, double sigma2, double* Bm);   // I + sym(A) / sigma2
void launch_cg_pc_logdet(hipStream_t s, const double* L, int64_t Mp, int64_t k, double* out);       // 2 sum log L_ii
// out (dtype's element type, ld ldo, zero on rows [k, rows_out)) = alpha Mt' v for the k x k block of Mt (ld Mp); v fp64 or dtype's type
void launch_cg_pc_mm(int dtype, hipStream_t s, const double* Mt, int64_t Mp, int64_t k, const void* v, int v_f64, int64_t ldv, int64_t ncols, double alpha,
                     void* out, int64_t ldo, int64_t rows_out);
// per-point noise variances (svgp_cg_set_noise): sigma_i^2 = T(diag) + s_i in the data dtype T with one rounding.
// launch_cg_noise_min: out[0] = min_i s_i in fp64, NaN if any s_i is NaN (one workgroup, a fixed tree)
void launch_cg_noise_min(int dtype, hipStream_t s, const void* sv, int64_t N, double* out);
// sig2[i] = T(diag) + s[i]; isig2 = T(1 / sig2), ssig2 = T(sqrt(sig2)) (formed in fp64, rounded once); isig64 = 1 / double(sig2)
void launch_cg_noise_prep(int dtype, hipStream_t s, const void* sv, int64_t N, double diag, void* sig2, void* isig2, void* ssig2, double* isig64);
// dst[col * ldd + i] = src[col * lds + i] vec[i] (in place allowed); dtype 0 / 1: the data dtype, 2: fp64 arrays whatever the data dtype
void launch_cg_rowscale(int dtype, hipStream_t s, const void* src, int64_t lds, const void* vec, int64_t N, int64_t ncols, void* dst, int64_t ldd);
// sbar[i] = T( 1/2 U[i, 0] P[i, 0] - (1 / 2T) sum_{t = 1..T} U[i, t] P[i, t] ), t ascending in fp64, rounded once; NaN with T = 0
// (U = [alpha, w_t], P = [alpha, p_t], N x (T + 1), ld N)
void launch_cg_sbar(int dtype, hipStream_t s, const void* U, const void* P, int64_t N, int T, void* sbar);
// the first stage (cg_dot_blocks(N) partials, fp64) of sum_i log sig2[i] (b NULL) or sum_i sig2[i] b[i]; launch_cg_colsum adds them
void launch_cg_noise_sum(int dtype, hipStream_t s, const void* sig2, const void* b, int64_t N, double* partial);

// ---- cg_sample.hip (pathwise function samples of the exact GP: svgp_cg_sampler_*) -----------------------------------------------
//   out[s * ldo + j] = mean_const + sum_l cos(frows[.][l] . xs_j + fbias[l]) W[l, s] + sum_i kappa(r^2(x_j, X_i)) V[i, s],   xs = invl o x
//   grad[(s * d + c) * ldg + j] = invl_c [ - sum_l sin(phase_l) frows[c][l] W[l, s] + 2 sum_i g(r_i^2) (xs_jc - Xs_ic) V[i, s] ]
// for the points j < len of the window [off, off + len) of x.  The grid is (point workgroups) x (row segments): cg_sample_plan gives
// the segments (whole chunks of 32 rows; a function of N alone) and the round, the number of points one set of launches covers
struct CgSampleArgs {
  const void* frows;   // [d][Lp] omega, zero on the padding
  const void* fbias;   // [Lp] tau
  const void* W;       // Lp x S column-major (ld Lp): amp w, zero on the padding rows
  const void* rows;    // [d][Np] the data rows as launch_kmv_prep wrote them
  const void* bias;    // [Np]
  const void* V;       // N x S column-major (ld N)
  const void* invl;    // [d]
  const void* x;       // [d][ldx] feature-major inputs
  void* part;          // nseg x (144 grad | 64 value) x min(round, len) elements of the data dtype
  void* out;           // nullable in the gradient form
  void* grad;          // NULL: the value form
  int64_t ldx, off, len, ldo, ldg;
  int64_t Lp, N, Np, S;     // N = Np = 0: the features alone
  int64_t seg_rows, round;  // cg_sample_plan(N)
  int nseg;
  int family, d;
  double variance, mean_const;
  // set by the launcher: the column block, the coordinate block, the round's points [p_base, p_base + p_len), the partial slots
  int64_t s0, p_base, p_len;
  int e0, nq;
};
void cg_sample_plan(int64_t N, int64_t* seg_rows, int* nseg, int64_t* round);
// the points of one set of launches: the plan's round, a quarter of it (at least 256) in the gradient form, whose partial sums have
// 144 slots a point against at most 64.  It enters no value
inline int64_t cg_sample_round(int64_t round, bool grad) { return !grad ? round : round / 4 < 256 ? 256 : round / 4; }
void launch_cg_sample(int dtype, hipStream_t s, const CgSampleArgs& a);
// B[s * N + i] = delta[i] - phi[s * N + i] - sigma eps[s * N + i], formed in fp64 and rounded once (phi nullable: no features)
// sig2 non-null (per-point noise): sigma_i = sqrt(double(sig2[i])) takes the place of sigma
void launch_cg_sample_rhs(int dtype, hipStream_t s, const void* delta, const void* phi, const void* eps, double sigma, int64_t N, int64_t S, void* B,
                          const void* sig2 = nullptr);
// W[s * Lp + l] = amp w[s * L + l] (l < L), 0 on the padding; frows[f][l] = omega[l * d + f], fbias[l] = tau[l], 0 on the padding
void launch_cg_sample_basis(int dtype, hipStream_t s, const void* omega, const void* tau, const void* w, int d, int64_t L, int64_t Lp, int64_t S,
                            double amp, void* frows, void* fbias, void* W);

// ---- cg_xgrad.hip (d lml / d x of the exact GP: svgp_cg_lml_grad_inputs) -----------------------------------------------------------
//   out[c * ldo + i] = invl_c sum_s Lp[i, s] sum_j 2 g(r^2(x_i, x_j)) (xs_ic - xs_jc) Rp[j, s],   g = d kappa / d(r^2), xs = invl o x
// over the N data points against themselves (r^2 of the diagonal is exactly 0).  One launch per (16 columns, coordinate block); the
// column blocks' partial sums part[block][c][i] (fp64) are added in ascending order, scaled and rounded once to the data dtype
struct CgXgradArgs {
  const void* rows;    // [d][Np] the data rows as launch_kmv_prep wrote them
  const void* bias;    // [Np]
  const void* invl;    // [d]
  const void* x;       // [d][ldx] the data, feature-major, unscaled
  const void* Lp;      // N x S column-major (ld N): the left panel
  const void* Rp;      // N x S column-major (ld N): the right panel
  void* part;          // ceil(S / 16) x d x N doubles
  int64_t ldx, N, Np, S;
  int family, d;
  double variance;
  // set by the launcher: the column block and the coordinate block
  int64_t s0;
  int blk, e0;
};
void launch_cg_xgrad(int dtype, hipStream_t s, const CgXgradArgs& a, void* out, int64_t ldo);

}  // namespace svgp
