// nn_points.hpp — launchers of nn_points.hip: the NearestNeighbors point kernels with per-point noise variances and prior-mean
// offsets (svgp_nn_set_noise / svgp_nn_set_mean), the per-point gradient mode of svgp_nn_lml_grad_points and its gathers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nn_common.hpp"

namespace svgp {

struct NnPointArgs {
  const void *x, *y;      // the data (data dtype)
  const void *sv, *mu;    // N per-point noise variances / mean offsets (data dtype); either may be null: zeros
  double* terms;          // [N][S] per-point slots
  int S;
  int* bad;
  void* Bd;               // modes 1 and 3: b_i, N x P.k column-major (data dtype), F_i, r_i / F_i
  double *Fd, *rF;
  void* Qd;               // mode 3: the per-pair term gF_i b_it^2 - (r_i / F_i) w_it b_it, laid out like Bd, and gF_i
  double* gF;
  const int* nbr;         // the neighbour table, null: the window
};

// mode 0: the lml slots; 1: fit; 2: lml and gradient; 3: 2 and 1 and the per-pair terms (svgp_nn_lml_grad_points)
void launch_nn_point_v(int dtype, int mode, hipStream_t s, const NnParams& P, const NnPointArgs& a);

// nn_local_kernel conditioned on the two vectors (either may be null)
void launch_nn_local_v(int dtype, hipStream_t s, const NnParams& P, const void* x, const void* y, const void* sv, const void* mu,
                       const void* xq, int64_t ldq, int64_t nq, int64_t q0, const int* nbr, int* bad, void* mean, void* var);

// sbar[j] = gF[j] + the sum of Qd over the pairs that name j: the <= kb later rows of the window (off null), or the reverse list
// off / rv of a table, one wavefront per j and a fixed tree.  fp64, no atomics
void launch_nn_sbar(int dtype, hipStream_t s, const void* Qd, const double* gF, int64_t n, int kb, const int64_t* off, const int64_t* rv,
                    double* sbar);

}  // namespace svgp
