// predict_grad.hpp — what predict_grad.hip (the kernels) and predict_grad_api.hip (svgp_predictor_*) share.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctx.hpp"

// svgp_predictor_create's snapshot of a model's predictive distribution: everything svgp_predictor_eval reads, so that the model it
// was made from may change or go
struct svgp_predictor {
  int dtype = 0, d = 0, family = 0, device = 0;
  size_t es = 8;
  int64_t M = 0, Mp = 0;
  double variance = 0, mean_const = 0;
  svgp::DevBuf invl, rows, bias, G, beta;   // model dtype (PredictGradArgs)
  svgp::DevBuf G64, beta64;                 // fp64, before the rounding (svgp_predictor_state)
};

namespace svgp {

// the data stage: for the points j < len of the window [off, off + len) of x, with k_i = kappa(r_i^2), D_ic = 2 g(r_i^2) (xs_c - zs_ic):
//   mean[j] = (mean_const + mux[j]) + sum_i k_i beta_i            var[j] = (variance + sum_i k_i (G k)_i) + 1e-18
//   mgrad[c * ldg + j] = invl_c sum_i D_ic beta_i                 vgrad[c * ldg + j] = 2 invl_c sum_i D_ic (G k)_i
// rows / bias as launch_sample_rows writes them without features (Lp = 0); Mp a multiple of 128; all arrays in `dtype`
struct PredictGradArgs {
  const void* rows;    // [d][Mp]
  const void* bias;    // [Mp]
  const void* G;       // Mp x Mp, exactly symmetric, zero on the padding
  const void* beta;    // [Mp], zero on the padding
  const void* invl;    // [d]
  const void* x;       // [d][ldx] feature-major inputs
  const void* mux;     // nullable: [len] prior mean offsets of the window's points
  void *mean, *var, *mgrad, *vgrad;   // each nullable
  int64_t ldx, off, len, ldg, Mp;
  int family, d;
  int e0;              // first coordinate of the launch's coordinate block (set by the launcher)
  double variance, mean_const;
};
void launch_predict_grad(int dtype, hipStream_t s, const PredictGradArgs& a);   // one launch per coordinate block

// the M-sized stage, fp64 whatever the model's dtype (column-major Mp x Mp, ld Mp)
// Lq64 = the lower triangle of Lq (M x M, ld M) widened, zero elsewhere; mv[i] = m_i (NonCentered) or (m_i - mean_const) - muz_i
// (Centered; muz nullable), zero on the padding
void launch_pg_widen_q(int dtype, hipStream_t s, const void* Lq, const void* m, const void* muz, int64_t M, int64_t Mp, int centered,
                       double mean_const, double* Lq64, double* mv);
// C = A' B (- W when W is given); alow / blow: the operand is lower triangular and is read below and on its diagonal only;
// Mvalid >= 0: C is zero outside its leading Mvalid x Mvalid block.  A' A is exactly symmetric (the same products in the same order)
void launch_pg_atb(hipStream_t s, const double* A, const double* B, const double* W, int64_t Mp, int64_t Mvalid, int alow, int blow, double* C);
// G (Mp x Mp) and beta (Mp) rounded once to the model dtype
void launch_pg_round(int dtype, hipStream_t s, const double* G64, const double* beta64, int64_t Mp, void* G, void* beta);

}  // namespace svgp
