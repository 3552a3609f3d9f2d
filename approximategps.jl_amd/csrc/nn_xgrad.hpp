// nn_xgrad.hpp — launchers of nn_xgrad.hip: the NearestNeighbors point kernel of svgp_nn_lml_grad_inputs (everything mode 3 of
// nn_points.hip's kernel does, and the per-pair and own-point terms of d lml / d x) and the gathers that sum them per point.
// Workspace of the call, reserved on the handle: Xd, N x kb x d elements of the data dtype, and Hd, N x d doubles; at N = 1e6,
// k = 30, d = 8 that is 1.9 GB in fp64 and 0.96 GB in fp32 for Xd, 64 MB for Hd.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nn_common.hpp"
#include "nn_points.hpp"

namespace svgp {

// NnPointArgs' mode 3, then Xd[f][t][i] (each coordinate laid out like Bd) = block i's d L_i / d s_{ns(i)_t, f} and
// Hd[f][i] = d L_i / d s_{i, f} (fp64), s = invl .* x
void launch_nn_point_x(int dtype, hipStream_t s, const NnParams& P, const NnPointArgs& a, void* Xd, double* Hd);

// out[f * ldo + j] = invl_f (Hd[f][j] + the sum of Xd[f] over the pairs that name j), rounded once to the data dtype: the <= kb later
// rows of the window (off null), or the reverse list off / rv of a table, one wavefront per j and a fixed tree.  fp64, no atomics
void launch_nn_xbar(int dtype, hipStream_t s, const NnParams& P, const void* Xd, const double* Hd, const int64_t* off, const int64_t* rv,
                    void* out, int64_t ldo);

// out[f * ldo + j] = v for j < n, f < d
void launch_nn_xfill(int dtype, hipStream_t s, int64_t n, int d, double v, void* out, int64_t ldo);

}  // namespace svgp
