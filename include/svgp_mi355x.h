/*
 * svgp_mi355x.h — C-ABI of libsvgp_mi355x.so: the MI355X-native (gfx950) sparse-variational-GP
 * ELBO / posterior path that drops in under ApproximateGPs.jl's
 * SparseVariationalApproximation / elbo / approx_lml / posterior API.
 *
 * The reference has NO FFI boundary today (pure Julia, multiple dispatch on AbstractGPs generics).
 * Each entry point below therefore cites the reference METHOD BODY it replaces
 * (paths relative to the reference repo; SVA = src/SparseVariationalApproximationModule.jl),
 * and INTEGRATION.md shows the Julia `ccall` binding a maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns an int32 status (SVGP_OK == 0) and
 *     never throws, aborts, prints or calls back into the host language.
 *   - all matrices are column-major (Julia layout).  Host pointers are borrowed for the call only.
 *   - array elements are in the compute dtype of the object (SVGP_F64 -> double, SVGP_F32 -> float);
 *     scalars are always double.
 *   - one svgp_ctx is bound to one GPU and one HIP stream; distinct contexts may be used
 *     concurrently from different threads, one context is not re-entrant.  Calls block until
 *     their host-visible results are written.
 *   - multi-GPU: a context may carry one rank of an RCCL communicator (svgp_ctx_attach_comm for one process per
 *     GPU, svgp_group_create for one process driving several GPUs).  svgp_elbo and svgp_elbo_grad are then
 *     COLLECTIVE: every rank evaluates its own shard and the library sums the partial results with one
 *     ncclAllReduce over xGMI on the device (no host hop).  Everything else stays local to the context.
 */
#ifndef SVGP_MI355X_H
#define SVGP_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVGP_MAX_D 64 /* largest input dimension the device path takes (round 3: 32 -> 64); beyond it SVGP_UNSUPPORTED from every entry
                         point that takes a dimension (model, data upload / wrap): the host falls back */
#define SVGP_ABI_VERSION 5 /* 3 = 2 + svgp_marginals, svgp_elbo_grad_ext, SVGP_LIK_BERNOULLI_NORMCDF; 4 = 3 + svgp_offload_advice /
                              svgp_offload_work and svgp_timing.ms_chol; 5 = 4 + svgp_last_timing_sized: svgp_last_timing writes the
                              48-byte v2 / v3 layout again (v4 let it write 56 bytes into a buffer a v3 host sized at 48), the
                              fields appended since are read through the sized call.  Additions only: v2 / v3 callers keep working.
                              Entry points added without a version step (hosts find them by symbol: dlsym / hasattr): svgp_elbo_grad_inputs,
                              svgp_elbo_grad_ext_inputs, svgp_model_set_mean_z, svgp_elbo_with_mean, svgp_marginals_with_mean,
                              svgp_elbo_grad_with_mean, svgp_laplace_*, svgp_nn_*, svgp_collapsed_* */

/* status codes -> Julia exceptions raised by the shim */
enum {
  SVGP_OK = 0,
  SVGP_INVALID_ARG = 1,  /* ArgumentError        (SVA:347-351 prior mismatch is checked Julia-side) */
  SVGP_NOT_POSDEF = 2,   /* PosDefException(info) from cholesky(Kuu)  [LinearAlgebra]; info in svgp_terms */
  SVGP_NEG_VARIANCE = 3, /* DomainError from sqrt(v < 0) inside marginals (SVA:354) */
  SVGP_UNSUPPORTED = 4,  /* shim falls back to the pure-Julia method */
  SVGP_HIP_ERROR = 5,
  SVGP_RCCL_ERROR = 6,
  SVGP_OOM = 7
};

enum { SVGP_F64 = 0, SVGP_F32 = 1 };

/* input layouts [KernelFunctions]: ColVecs(X) X is d×n (a point is contiguous); RowVecs(X) X is n×d
 * (a feature is contiguous); a plain Vector is d = 1. */
enum { SVGP_COLVECS = 0, SVGP_ROWVECS = 1, SVGP_VEC = 2 };

/* kernel families [KernelFunctions]: variance * (Base ∘ ARDTransform(inv_lengthscale)) */
enum { SVGP_KERNEL_SE = 0, SVGP_KERNEL_MATERN32 = 1, SVGP_KERNEL_MATERN52 = 2 };

/* likelihoods [GPLikelihoods]; SVA:307-317 wraps FiniteGP noise as GAUSSIAN(σ² = fx.Σy[1]) */
enum {
  SVGP_LIK_GAUSSIAN = 0,
  SVGP_LIK_BERNOULLI_LOGISTIC = 1,
  SVGP_LIK_POISSON_EXP = 2,      /* PoissonLikelihood(exp):      y ~ Poisson(exp f) */
  SVGP_LIK_EXPONENTIAL_EXP = 3,  /* ExponentialLikelihood(exp):  y ~ Exponential(scale exp f) = Gamma(1, scale exp f) */
  SVGP_LIK_GAMMA_EXP = 4,        /* GammaLikelihood(alpha, exp): y ~ Gamma(shape alpha, scale exp f); alpha in lik_sigma2 */
  SVGP_LIK_BERNOULLI_NORMCDF = 5 /* BernoulliLikelihood(NormalCDFLink()) (probit): y ~ Bernoulli(Phi(f)); Gauss-Hermite */
};

/* SVA:41 Centered, SVA:57 NonCentered (the 2-arg constructor's default, SVA:93-95) */
enum { SVGP_NONCENTERED = 0, SVGP_CENTERED = 1 };

/* what to do when a predictive variance (+1e-18) is negative: the reference throws DomainError */
enum { SVGP_NEGVAR_ERROR = 0, SVGP_NEGVAR_CLAMP = 1 };

typedef struct svgp_ctx svgp_ctx;
typedef struct svgp_data svgp_data;
typedef struct svgp_model svgp_model;
struct svgp_model_desc;

/* Everything a SparseVariationalApproximation + likelihood holds (SVA:59-62):
 *   fz = GP(mean_const, variance * (Base ∘ ARD(inv_lengthscale)))(z, jitter),  q = MvNormal(m, Lq Lq'). */
typedef struct svgp_model_desc {
  int32_t dtype;           /* SVGP_F64 | SVGP_F32: compute dtype AND element type of z, m, Lq */
  int32_t kernel;          /* SVGP_KERNEL_* */
  int32_t parametrization; /* SVGP_NONCENTERED | SVGP_CENTERED */
  int32_t likelihood;      /* SVGP_LIK_* */
  int32_t quadrature_n;    /* 0 = DefaultExpectationMethod (analytic where closed form exists, else GH-20);
                              n > 0 = GaussHermiteExpectation(n) */
  int32_t layout_z;        /* layout of z: SVGP_COLVECS (d×M) | SVGP_ROWVECS (M×d) | SVGP_VEC */
  int32_t neg_var_policy;  /* SVGP_NEGVAR_* */
  int32_t d;               /* input dimension */
  int64_t M;               /* number of inducing points */
  double variance;         /* kernel variance σ_k² */
  const double* inv_lengthscale; /* d entries; isotropic = all equal */
  double mean_const;       /* ConstMean value, 0 for ZeroMean */
  double jitter;           /* fz.Σy (isotropic), part of Kuu (src/utils.jl:17) */
  double lik_sigma2;       /* likelihood parameter: GaussianLikelihood σ², GammaLikelihood shape α; unused otherwise */
  const void* z;           /* inducing inputs */
  const void* m;           /* mean(q), M */
  const void* Lq;          /* _chol_lower(_chol_cov(q)) (src/utils.jl:15,18), M×M, upper triangle ignored */
} svgp_model_desc;

/* Optional breakdown of one ELBO evaluation (SVA:355-359). */
typedef struct svgp_terms {
  double elbo;        /* expectation * scale - kl */
  double expectation; /* Σ_i E_{q(f_i)}[log p(y_i | f_i)], unscaled */
  double kl;          /* _prior_kl(sva)  SVA:362-373 */
  double scale;       /* num_data / n_batch  SVA:357-358 */
  double logdet_kuu;  /* 2 Σ log diag chol(Kuu) */
  int64_t n_points;
  int64_t n_neg_var;  /* points whose variance + 1e-18 was negative */
  int32_t chol_info;  /* 0, or the order of the first non-positive leading minor of Kuu (LAPACK info) */
  int32_t reserved;
} svgp_terms;

/* Device timings of the last call on the context, measured with HIP events on the context's stream. */
typedef struct svgp_timing {
  double ms_total;
  double ms_prep;  /* Kuu, cholesky, diagonal-block inverses, panel products, KL */
  double ms_strip; /* the fused Kuf -> trsm -> trmm strip kernel alone (one launch) */
  double ms_expect;/* marginals + expected log-likelihood + final reduce */
  double ms_kuf;   /* standalone Kuf assembly kernel (svgp_kuf only) */
  int64_t strip_launches;
  /* ---- end of the v2 / v3 layout (SVGP_TIMING_V3_BYTES = 48): svgp_last_timing writes exactly the fields above ---- */
  double ms_chol;  /* (v4) cholesky(Kuu) alone - the blocked factorisation with its T panels - inside ms_prep */
  double ms_overlap; /* (v5) part of ms_prep that ran BESIDE the strips (flag-gated strips on the second stream); 0 when serial */
} svgp_timing;
#define SVGP_TIMING_V3_BYTES 48

/* ---- library / context ------------------------------------------------------------------- */
int32_t svgp_version(void);
int32_t svgp_device_count(void);
/* `stream` is a hipStream_t to run on (e.g. torch's current stream) or NULL to create a private one. */
int32_t svgp_ctx_create(int32_t device_id, void* stream, svgp_ctx** out);
int32_t svgp_ctx_destroy(svgp_ctx* ctx);
/* text of the last error on ctx (owned by the library, valid until the next call on ctx) */
const char* svgp_last_error(const svgp_ctx* ctx);
/* writes the first SVGP_TIMING_V3_BYTES of the timing struct: the layout every ABI version shares.
 * NOTE for hosts compiled against the ABI-v4 header (56-byte struct): v4's svgp_last_timing also wrote ms_chol; since v5 it does NOT
 * (a v3-compiled host had sized its buffer at 48 bytes), so a v4 host reading ms_chol after this call sees whatever its buffer held.
 * The library cannot know the caller's struct size here: v4 hosts must move to svgp_last_timing_sized. */
int32_t svgp_last_timing(const svgp_ctx* ctx, svgp_timing* out);
/* (v5) writes the first min(out_bytes, size of svgp_timing) bytes: a host passes the size of the struct IT was compiled against, so the
 * struct can grow without the library ever writing past the caller's buffer */
int32_t svgp_last_timing_sized(const svgp_ctx* ctx, void* out, int64_t out_bytes);

/* ---- multi-GPU: data-parallel shards of the sum over points (SVA:355-359), SURVEY §8e ----------
 * The expectation term is a plain sum over data points, so each rank holds a shard of (x, y) in its own HBM,
 * replicates the M-sized work (Kuu, cholesky, KL) and the ranks' {sum E, n_points, n_neg_var, status flags}
 * are summed by ONE ncclAllReduce of 8 doubles issued by the library on the context's stream, straight from
 * the device buffer the reduction kernel wrote.  RCCL is loaded with dlopen on first use (no link-time
 * dependency; SVGP_RCCL_LIB overrides the library name); failures map to SVGP_RCCL_ERROR.
 *
 * One process per GPU: rank 0 calls svgp_comm_unique_id, the host transports the 128 bytes to every rank
 * (MPI / torch.distributed / Distributed.jl), every rank calls svgp_ctx_attach_comm on its own context
 * (collective: ncclCommInitRank).  No rank can leave its peers inside a collective:
 *   svgp_elbo / svgp_elbo_host: ONE fixed-size all-reduce (8 doubles); a rank that fails locally - bad arguments, NULL model,
 *     allocation failure, HIP error - enters it with zero contributions and the failure flag; its peers return SVGP_RCCL_ERROR.
 *   svgp_elbo_grad / svgp_elbo_grad_ext: an opening fixed-size all-reduce {batch size, failure flag} every rank enters, whatever
 *     state it is in - a rank that cannot evaluate (also one handed a NULL model) sends the flag, returns its own error and joins
 *     nothing else; every other rank reads the reduced flag before the closing gradient all-reduce (whose size depends on M and d),
 *     skips it and returns SVGP_RCCL_ERROR.  A rank that fails later, inside its backward pass, enters the closing all-reduce with
 *     its failure flag.  The communicator stays usable after either kind of failure.
 * ncclCommAbort is left for the case that a collective itself cannot be issued (an RCCL error).  The one-process group calls
 * (svgp_group_elbo / svgp_group_elbo_grad) validate every member before anything is enqueued and return the first member's
 * error without touching the communicator. */
#define SVGP_COMM_ID_BYTES 128
int32_t svgp_comm_unique_id(void* id_out /* SVGP_COMM_ID_BYTES */);
int32_t svgp_ctx_attach_comm(svgp_ctx* ctx, const void* id, int32_t world_size, int32_t rank);
int32_t svgp_ctx_detach_comm(svgp_ctx* ctx);
int32_t svgp_ctx_comm_info(const svgp_ctx* ctx, int32_t* world_size_out, int32_t* rank_out);

/* One process, several GPUs (the natural shape of a Julia host): a group owns one context per device and their
 * communicator (ncclCommInitAll).  Arrays of handles are indexed by member; svgp_group_ctx(g, i) gives member i's
 * context for the local calls (svgp_predict, svgp_posterior, svgp_*_free ...). */
typedef struct svgp_group svgp_group;
int32_t svgp_group_create(int32_t n_devices, const int32_t* device_ids, svgp_group** out);
int32_t svgp_group_destroy(svgp_group* group);
int32_t svgp_group_size(const svgp_group* group);
svgp_ctx* svgp_group_ctx(svgp_group* group, int32_t member);
const char* svgp_group_last_error(const svgp_group* group);
/* uploads x, y once, sharded contiguously by point index over the members (shards_out: n_devices handles) */
int32_t svgp_group_data_upload(svgp_group* group, int32_t dtype, int32_t layout, int32_t d, int64_t n,
                               const void* x_host, const void* y_host, svgp_data** shards_out);
/* one replica of the model per member (models_out: n_devices handles) */
int32_t svgp_group_model_create(svgp_group* group, const struct svgp_model_desc* desc, svgp_model** models_out);
int32_t svgp_group_model_update(svgp_group* group, svgp_model* const* models, const struct svgp_model_desc* desc);

/* ---- data: x = lfx.fx.x, y (SVA:340-343) kept resident in HBM ------------------------------ */
int32_t svgp_data_upload(svgp_ctx* ctx, int32_t dtype, int32_t layout, int32_t d, int64_t n,
                         const void* x_host, const void* y_host, svgp_data** out);
/* wrap device memory without copying: x_dev is feature-major [d][ldx] (RowVecs storage), y_dev may be NULL */
int32_t svgp_data_wrap_device(svgp_ctx* ctx, int32_t dtype, int32_t d, int64_t n, int64_t ldx,
                              const void* x_dev, const void* y_dev, svgp_data** out);
int32_t svgp_data_free(svgp_ctx* ctx, svgp_data* data);

/* ---- model: SparseVariationalApproximation(fz, q) + likelihood, resident in HBM -------------- */
int32_t svgp_model_create(svgp_ctx* ctx, const svgp_model_desc* desc, svgp_model** out);
/* new parameter values, same M / d / dtype (a training step) */
int32_t svgp_model_update(svgp_ctx* ctx, svgp_model* model, const svgp_model_desc* desc);
int32_t svgp_model_free(svgp_ctx* ctx, svgp_model* model);

/* ---- elbo(sva, lfx, y; num_data, quadrature)  replaces SVA:340-360 (and :307-317, :276-280) --- */
/* evaluates points [batch_off, batch_off + batch_len) of `data`; num_data <= 0 means batch_len.
 * On a context with a communicator: COLLECTIVE — every rank passes its own shard's batch and gets the global
 * ELBO = (sum over all ranks' points) * num_data / n_global - KL; terms_out->n_points = n_global.
 * Non-finite numbers are NOT an error, as in the reference: a NaN coordinate of x gives NaN marginals for that point (and only that
 * point) and a NaN ELBO, an infinite y an infinite ELBO, a zero on the diagonal of Lq KL = +Inf - the status is SVGP_OK and the numbers say
 * it; a NaN in z or in a kernel parameter makes Kuu NaN and cholesky(Kuu) reports SVGP_NOT_POSDEF as LAPACK does (tests/fuzz_errors.py). */
int32_t svgp_elbo(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off,
                  int64_t batch_len, double num_data, double* elbo_out, svgp_terms* terms_out);
/* data-parallel shard: only Σ_i E[log p(y_i|f_i)] over the shard's points (no scale, no KL), so that
 * ranks sum partials with ONE all-reduce and subtract the KL once (SVA:355-359).
 * partial_out[4] = {sum_expectation, n_points, n_neg_var, chol_info}.  Always LOCAL (never a collective): the building
 * block for a host that runs its own all-reduce. */
int32_t svgp_elbo_partial(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off,
                          int64_t batch_len, double partial_out[4]);
/* KL(q || p) and logdet(Kuu) of the model alone: _prior_kl  SVA:362-373 */
int32_t svgp_prior_kl(svgp_ctx* ctx, svgp_model* model, double* kl_out, double* logdet_kuu_out);
/* one-shot variant taking host x, y (the literal drop-in for an ad-hoc elbo(sva, fx, y) call) */
int32_t svgp_elbo_host(svgp_ctx* ctx, const svgp_model_desc* desc, int32_t layout_x, int64_t n,
                       const void* x_host, const void* y_host, double num_data, double* elbo_out,
                       svgp_terms* terms_out);

/* ---- gradient of the ELBO (what Zygote produces for the reference's training loops:
 * examples/a-regression/script.jl:188-194, test/SparseVariationalApproximationModule.jl:170-175).  Both parametrisations
 * (Centered: the adjoint runs on the whitened (Lk \\ (m - c), Lk \\ Lq) and is chained back through Lk).  Every output array is caller-allocated host memory; z, m, Lq gradients have the
 * dtype / layout of the corresponding svgp_model_desc arrays (Lq: lower triangle, upper zeroed); NULL skips one. */
typedef struct svgp_grads {
  double variance;          /* d elbo / d kernel variance */
  double lik_sigma2;        /* d elbo / d likelihood parameter (Gaussian sigma^2, Gamma alpha; 0 otherwise) */
  double mean_const;        /* d elbo / d ConstMean value */
  double* inv_lengthscale;  /* d entries */
  void* z;
  void* m;
  void* Lq;
} svgp_grads;
/* On a context with a communicator: COLLECTIVE — value and gradient of the global ELBO on every rank (the batch size
 * is all-reduced on the device before the backward pass, the gradient by one grouped ncclAllReduce after it).
 * The VALUE this call returns and svgp_elbo's value of the same batch are the same quantity computed along two paths: svgp_elbo takes
 * the posterior variance as k(x,x) - sum A^2 + sum (B'A)^2 (SVA:251, two column sums), the value-and-gradient strips have no B'A product
 * and take it from the algebraically equal k_j' (R A)_j, R = Lk^-T (Lq Lq' - I).  In SVGP_F64 the two agree to ~1e-15 relative.  In
 * SVGP_F32 they differ by rounding: measured |value_grad - value_elbo| / |value_elbo| = 2e-9 ... 3e-7 on the benchmark shapes (H32, C3, C5
 * at full size) and on ill-conditioned posteriors with a marginal variance down to 4.5e-5 of the prior's (profiles/round5/f32_value_gap.log;
 * both are within 1e-6 of the fp64 value there) - a host that logs both should expect agreement to ~1e-6 relative in fp32, not to the last
 * bit (tests/test_gpu_round5.py asserts 2e-6).  The fp32 gradient blocks on those posteriors stay within 5e-5 (m, Lq) / 5e-4 (z, inverse
 * lengthscales) of the fp64 gradient, relative to each block's largest entry. */
int32_t svgp_elbo_grad(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                       double num_data, double* elbo_out, svgp_terms* terms_out, svgp_grads* grads_out);
/* the same two evaluations driven from one process over the members of a group: member i evaluates points
 * [offs[i], offs[i] + lens[i]) of shards[i]; results are the global ones (read from member 0). */
int32_t svgp_group_elbo(svgp_group* group, svgp_model* const* models, const svgp_data* const* shards,
                        const int64_t* offs, const int64_t* lens, double num_data, double* elbo_out,
                        svgp_terms* terms_out);
int32_t svgp_group_elbo_grad(svgp_group* group, svgp_model* const* models, const svgp_data* const* shards,
                             const int64_t* offs, const int64_t* lens, double num_data, double* elbo_out,
                             svgp_terms* terms_out, svgp_grads* grads_out);
/* data-parallel shard of the value-and-gradient (the gradient counterpart of svgp_elbo_partial):
 *   value = scale * Σ_{i in shard} E_{q(f_i)}[log p(y_i|f_i)] - kl_weight * KL   and its gradient.  Always LOCAL.
 * With scale = num_data / n_global and kl_weight = 1 / world_size on every rank, ONE sum all-reduce of
 * (value, gradients) is the global ELBO (SVA:355-359) and its gradient, for both parametrisations
 * (terms_out->elbo holds the same value; terms_out->scale = scale). */
int32_t svgp_elbo_grad_shard(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                             double scale, double kl_weight, double* value_out, svgp_terms* terms_out,
                             svgp_grads* grads_out);

/* ---- any other single-latent likelihood: the host evaluates it on the device-computed marginals ----------------
 * (SURVEY 8 f4 "generic GH for user link functions".)  Only SVA:355, expected_loglikelihood(quadrature, lik, q_f, y),
 * depends on the likelihood, and it is O(n) scalar work; everything O(M^2 n) is likelihood-free.  So for a likelihood
 * the SVGP_LIK_* codes do not enumerate the binding keeps the reference's own GPLikelihoods call and gives it the
 * device's marginals:
 *   svgp_marginals        replaces marginals(f_post(x)) of SVA:354: mean_out[i] = mu_i, var_out[i] = v_i + 1e-18
 *                         (fp64, batch_len each; host); SVGP_NEG_VARIANCE / clamping per neg_var_policy.  Needs no y.
 *   svgp_elbo_grad_ext    value and gradient of  (num_data / batch_len) * sum_e - KL  where the host passes
 *                         sum_e = sum_i E_i and g_mu[i] = dE_i/dmu_i, g_v[i] = dE_i/dv_i (fp64, unscaled, host): the
 *                         same backward pass as svgp_elbo_grad with these in place of the built-in likelihood's;
 *                         grads_out->lik_sigma2 = 0 (the likelihood's own parameters are the host's to differentiate).
 *                         On a context with a communicator it is collective exactly like svgp_elbo_grad (sum_e and the
 *                         point gradients are then this rank's shard's). */
int32_t svgp_marginals(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                       double* mean_out, double* var_out);
int32_t svgp_elbo_grad_ext(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                           double num_data, double sum_e, const double* g_mu, const double* g_v, double* elbo_out,
                           svgp_terms* terms_out, svgp_grads* grads_out);

/* ---- d elbo / d x: the gradient with respect to the data inputs (what Zygote gives the reference's elbo for lfx.fx.x) ----------
 * For a learned feature map in front of the GP (x = NN(theta)(raw)): the host back-propagates x_bar into theta.
 *   svgp_elbo_grad_inputs      = svgp_elbo_grad     + x_bar
 *   svgp_elbo_grad_ext_inputs  = svgp_elbo_grad_ext + x_bar
 * Every other output is the one the call without `_inputs` returns, bitwise, on the same context and inputs.  x_bar covers the batch
 * [batch_off, batch_off + batch_len): element (f, j) at gx->x[f * gx->ld + j] (feature-major: the storage of RowVecs and of
 * svgp_data_wrap_device), in the dtype of the data.  x_bar_j depends on point j alone (and on the model): a NaN coordinate of point j
 * gives NaN in column j only.  On a context with a communicator both calls are collective like their counterparts, and x_bar is NEVER
 * all-reduced: each rank gets its own shard's, with the scale of the global batch size.  fp32: within 5e-4 of the fp64 x_bar relative
 * to its largest entry (the z / inverse-lengthscale tolerance above).  SVGP_INVALID_ARG, before anything is enqueued, for a NULL gx or
 * gx->x, ld < batch_len, on_device not 0 / 1, reserved != 0, or a device gx->x overlapping the data's x storage. */
typedef struct svgp_input_grad {
  void* x;           /* d elbo / d x, d rows of ld elements (columns j >= batch_len are not touched) */
  int64_t ld;        /* >= batch_len */
  int32_t on_device; /* 0: host memory, written before the call returns; 1: device memory of the context's GPU, written on the context's stream */
  int32_t reserved;  /* must be 0 */
} svgp_input_grad;   /* 24 bytes */
int32_t svgp_elbo_grad_inputs(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off,
                              int64_t batch_len, double num_data, double* elbo_out, svgp_terms* terms_out,
                              svgp_grads* grads_out, const svgp_input_grad* gx);
int32_t svgp_elbo_grad_ext_inputs(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off,
                                  int64_t batch_len, double num_data, double sum_e, const double* g_mu,
                                  const double* g_v, double* elbo_out, svgp_terms* terms_out,
                                  svgp_grads* grads_out, const svgp_input_grad* gx);

/* ---- prior mean functions other than ZeroMean / ConstMean: offsets the caller evaluates --------------------------------------
 * For GP(CustomMean(g), k) (a physics trend, a linear trend, a learned mean): the caller evaluates the O(n) mean function, the library
 * does the O(n M^2) work and hands back the adjoint.  A model may carry an offset vector muz at the inducing points
 * (svgp_model_set_mean_z) and a call may carry an offset vector mux at the batch's points (svgp_point_mean).  Both add to mean_const:
 *   mean(f.prior, x_j) = mean_const + mux[j]   for the points [batch_off, batch_off + batch_len)   (SVA:211, 241, 250)
 *   mean(fz)_k         = mean_const + muz[k]   for k < M                                          (SVA:133, 362)
 * Effects:
 *   - posterior marginal mean: mu_j = (mean_const + mux[j]) + (K_xu alpha)_j, in that order of additions (mux = 0: bitwise the
 *     constant-mean mean_const + (K_xu alpha)_j);
 *   - Centered: m~ = Lk \ (m - mean_const - muz), which changes alpha (svgp_posterior's too) and the KL;
 *   - NonCentered: muz has no effect on any output (alpha = Lk' \ m, SVA:182); it is accepted, stored and ignored;
 *   - variances, the 1e-18 of f_post(x) and the SVGP_NEGVAR_* policy: unchanged.
 * Gradients: mux_bar[j] = scale * dE_j/dmu_j, rounded to the data dtype as x_bar is (fp32: within the m tolerance of svgp_elbo_grad,
 * 5e-5 of the fp64 block's largest entry; measured 2.7e-6).  fp32 elsewhere, measured against the fp64 reference on the test problems
 * (tests/test_gpu_prior_mean.py, M = 64): Gaussian likelihood - marginal means within 4.8e-5, m / Lq 5.3e-5, inverse lengthscales 8.2e-4
 * of the block's largest entry; other likelihoods - as the existing calls on the same problem without offsets (up to 9e-3 on z): the
 * rounding of the fp32 strips and adjoint, which the offsets do not change.  muz_bar = -m_bar (Centered: m enters only through m - muz) and 0 (NonCentered); the
 * library does not return it.  grads_out->mean_const keeps its meaning and equals sum_j mux_bar[j] + sum_k muz_bar[k].
 * Non-finite offsets follow the reference's arithmetic: a NaN in mux[j] gives a NaN marginal mean for point j only and a NaN ELBO,
 * status SVGP_OK (the NaN-x rule of svgp_elbo).
 * svgp_predict keeps returning mean_const + K*u alpha: a caller with a mean function adds its own offset at x*.  The group calls
 * (svgp_group_*), svgp_elbo_host and svgp_elbo_partial take no mux: they keep the constant mean (plus muz, if set on the model). */
typedef struct svgp_point_mean {   /* mux: batch_len values in the data's dtype, element j belongs to point batch_off + j */
  const void* mu;
  int32_t on_device;   /* 0: host memory (one copy per call); 1: device memory of the context's GPU, read on the context's stream */
  int32_t reserved;    /* must be 0 */
} svgp_point_mean;     /* 16 bytes */
typedef struct svgp_point_mean_grad {   /* mux_bar: batch_len values in the data's dtype, element j belongs to point batch_off + j */
  void* mu_bar;
  int32_t on_device;   /* 0: host memory, written before the call returns; 1: device memory, written on the context's stream */
  int32_t reserved;    /* must be 0 */
} svgp_point_mean_grad;   /* 16 bytes */
/* muz: M values in the model's dtype (host memory), copied into a model-owned device buffer; NULL removes it.  The model is prepared
 * again (lazily) at its next evaluation; muz persists across svgp_model_update until it is set again. */
int32_t svgp_model_set_mean_z(svgp_ctx* ctx, svgp_model* model, const void* mu_z);
/* svgp_elbo / svgp_marginals with mux.  pm = NULL: exactly the call without `_with_mean` (bitwise; nothing more is launched). */
int32_t svgp_elbo_with_mean(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                            double num_data, const svgp_point_mean* pm, double* elbo_out, svgp_terms* terms_out);
int32_t svgp_marginals_with_mean(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                                 const svgp_point_mean* pm, double* mean_out, double* var_out);
/* Value and gradient with mux, one entry point for four cases: g_mu = g_v = NULL is the built-in likelihood (svgp_elbo_grad), both
 * non-NULL a likelihood the host evaluated on svgp_marginals_with_mean (svgp_elbo_grad_ext: sum_e, g_mu, g_v as there); gx = NULL: no
 * x_bar, else svgp_input_grad as in svgp_elbo_grad_inputs; gpm = NULL: no mux_bar.  pm = NULL with gpm = NULL is exactly the
 * corresponding existing call, bitwise.  Every output other than mux_bar is that call's, evaluated at the shifted prior mean.
 * SVGP_INVALID_ARG, before anything is enqueued: a NULL pm->mu or gpm->mu_bar, on_device not 0 / 1 or reserved != 0 in pm or gpm,
 * a device gpm->mu_bar overlapping the data's storage (x, y) or a device x_bar output, exactly one of g_mu / g_v NULL, and every
 * argument error of the existing calls.  On a context with a communicator all three calls are collective like their counterparts
 * (an argument error goes through the opening handshake); mux is the rank's own shard's, and mux_bar is NEVER all-reduced. */
int32_t svgp_elbo_grad_with_mean(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                                 double num_data, const svgp_point_mean* pm, double sum_e, const double* g_mu, const double* g_v,
                                 double* elbo_out, svgp_terms* terms_out, svgp_grads* grads_out, const svgp_input_grad* gx,
                                 svgp_point_mean_grad* gpm);

/* ---- posterior(sva)  replaces SVA:115-136 (Centered) / SVA:160-187 (NonCentered) -------------
 * fills ApproxPosteriorGP.data = (Kuu = Cholesky(Lk), B, α): Lk_out M×M lower (upper zeroed),
 * alpha_out M, B_out M×M (NULL to skip; NonCentered B is the caller's Lq). */
int32_t svgp_posterior(svgp_ctx* ctx, svgp_model* model, void* Lk_out, void* alpha_out, void* B_out);

/* ---- mean / var / mean_and_var / cov / mean_and_cov  replaces SVA:208-253 ---------------------
 * mean_out, var_out: n (either may be NULL); cov_out: n×n or NULL (SVA:223-228). */
int32_t svgp_predict(svgp_ctx* ctx, svgp_model* model, int32_t layout_x, int64_t n, const void* x_host,
                     void* mean_out, void* var_out, void* cov_out);
/* cross-covariance cov(f, x, y)  replaces SVA:255-264; cov_out is nx×ny */
int32_t svgp_predict_cross_cov(svgp_ctx* ctx, svgp_model* model, int32_t layout, int64_t nx,
                               const void* x_host, int64_t ny, const void* y_host, void* cov_out);

/* ---- Kuf = cov(prior, z, x) alone  (SVA:216), for the "Kuf-assembly HBM GB/s" metric ----------
 * Kuf_out_host: M×batch_len column-major or NULL (result stays in HBM; timing only). */
int32_t svgp_kuf(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off,
                 int64_t batch_len, void* Kuf_out_host);

/* ---- Gauss–Hermite rule used by GH-n (FastGaussQuadrature.gausshermite) ---------------------- */
int32_t svgp_gausshermite(int32_t n, double* nodes_out, double* weights_out);

/* ---- small problems: is the device worth calling? -----------------------------------------------
 * The reference's own workloads are tiny (examples/a-regression/script.jl:33,69,176: N = 10 000, M = 20, minibatch 100;
 * test/SparseVariationalApproximationModule.jl: N <= 100).  A call into this library has a floor that does not depend on the
 * problem - measured on MI355X (profiles/round3/small_problems.md): 160-180 us for svgp_elbo on resident data, ~250 us for the
 * one-shot svgp_elbo_host the un-modified `elbo(sva, lfx, y)` reaches through the hook, ~600 us for value-and-gradient - while
 * the host path costs about 1e-10 s per unit of  work(n, M, d) = n M (2 M + 3 d + 30) + M^3 / 3.  Returns 1 when
 * work >= SVGP_OFFLOAD_MIN_WORK (default 3e6: the measured crossover), else 0; the hooks of the Julia binding (try_elbo,
 * try_posterior, try_predict, the rrule) and the Python mirror decline below it and the pure-Julia method body runs.
 * The environment variable SVGP_OFFLOAD_MIN_WORK overrides the threshold (0: always offload).  Advice only: the explicit
 * resident-handle calls (svgp_elbo, svgp_elbo_grad, ...) never refuse a problem for being small.  No context, no GPU needed. */
int32_t svgp_offload_advice(int64_t n_points, int64_t M, int32_t d, int32_t dtype, int32_t want_gradient);
double svgp_offload_work(int64_t n_points, int64_t M, int32_t d);

/* ---- the Laplace approximation: LaplaceApproximation / posterior / approx_lml  (src/LaplaceApproximationModule.jl) -------------
 * A handle over the x and y of an existing data handle (which must outlive it) holding the N x N work of Newton mode finding
 * (_newton_inner_loop :256-276, RW Alg. 3.1): K = kernelmatrix(k, x) + jitter I, B = I + sW K sW, its Cholesky factor and inverse.
 * The prior mean is zero (_check_laplace_inputs :167-178 asserts it); one latent function per observation.
 *   svgp_laplace_fit       Newton from f_init (NULL: zeros, the reference's mean(fx); else N host values in the data's dtype), or
 *                          with warm_start = 1 and f_init = NULL from the mode of the previous successful fit on the handle (the warm
 *                          start of build_laplace_objective :95-132; a call that returned an error, a rejected argument included,
 *                          leaves the handle without a mode: the next call starts cold, mode / predict return SVGP_INVALID_ARG).  Convergence is isapprox(f, fnew) in the compute dtype,
 *                          |f - fnew| <= sqrt(eps) max(|f|, |fnew|); the loop then KEEPS f, otherwise f = fnew, after maxiter steps f
 *                          is the last fnew.  lml_out = -a'f / 2 + sum log p(y|f) - sum log diag L at that f (laplace_lml :157-165,
 *                          _laplace_lml :250-254).  The handle caches the intermediates at f for the predictions.
 *   svgp_laplace_lml_grad  the same fit, then d lml / d variance and d lml / d inv_lengthscale (d entries): the closed form of RW
 *                          Alg. 5.1 with d3 log p, the total derivative along the Newton fixed point that the reference's
 *                          implicit-function rrule (:330-369) gives Zygote.  Likelihood parameters, y and x are not differentiated.
 *   svgp_laplace_mode      f_opt, d log p / df and W = -d2 log p / df2 at it (N each, data dtype, host; any may be NULL).
 *   svgp_laplace_predict   mean = k(x, x*)' dll (RW 3.21), var = k(x*, x*) - colsum(v.^2), cov = k(x*, x*) - v'v with
 *                          v = L \ (sW k(x, x*)) (RW 3.29, :425-463); n values (mean, var) / n x n column-major (cov), data dtype,
 *                          any may be NULL.  x* in `layout` (SVGP_COLVECS / ROWVECS / VEC) with the data's d.
 *   svgp_laplace_predict_cross_cov  cov(f, x*, y*) = k(x*, y*) - vx' vy, nx x ny column-major (:458-463).
 * fp64 and fp32; SE / Matern-3/2 / Matern-5/2 with ARD, d <= SVGP_MAX_D; 1 <= N <= 8192 (fp64) / 16384 (fp32), the sizes the
 * device Cholesky is tested at - beyond them svgp_laplace_create returns SVGP_UNSUPPORTED.  SVGP_INVALID_ARG, before anything is
 * enqueued: NULL required pointers, data without y, a descriptor whose dtype / d differ from the data's, maxiter < 1, warm_start
 * not 0 / 1, jitter < 0, variance <= 0, a Gaussian sigma^2 or Gamma alpha <= 0, reserved != 0; mode / predict before a successful
 * fit.  SVGP_NOT_POSDEF when cholesky(B) fails (info in svgp_laplace_info.chol_info).  Never collective: on a context with a
 * communicator these calls stay local.  Found by symbol (no ABI version step). */
typedef struct svgp_laplace svgp_laplace;
typedef struct svgp_laplace_desc {
  int32_t dtype;            /* SVGP_F64 | SVGP_F32: must be the data's */
  int32_t kernel;           /* SVGP_KERNEL_* */
  int32_t likelihood;       /* SVGP_LIK_* */
  int32_t d;                /* must be the data's */
  int32_t maxiter;          /* >= 1 (newton_kwargs maxiter, default 100) */
  int32_t warm_start;       /* 1: start from the previous fit's mode when f_init is NULL */
  double variance;          /* kernel variance */
  const double* inv_lengthscale; /* d entries */
  double jitter;            /* cov(fx) = K + jitter I */
  double lik_sigma2;        /* Gaussian sigma^2, Gamma shape alpha; unused otherwise */
  int64_t reserved;         /* must be 0 */
} svgp_laplace_desc;        /* 64 bytes */
typedef struct svgp_laplace_info {
  int32_t iterations;       /* Newton steps taken */
  int32_t converged;        /* 1 when isapprox(f, fnew) stopped the loop */
  int32_t chol_info;        /* 0, or the order of the first non-positive leading minor of B */
  int32_t reserved;
  double lml;
  /* device time of the steps (HIP events; 0 when the context runs without timing): point kernel and B assembly, cholesky(B),
     L^-1, the GEMVs and the convergence reduction */
  double ms_point, ms_chol, ms_linv, ms_gemv;
} svgp_laplace_info;        /* 56 bytes */
int32_t svgp_laplace_create(svgp_ctx* ctx, const svgp_data* data, svgp_laplace** out);
int32_t svgp_laplace_fit(svgp_ctx* ctx, svgp_laplace* la, const svgp_laplace_desc* desc, const void* f_init, double* lml_out,
                         svgp_laplace_info* info);
int32_t svgp_laplace_lml_grad(svgp_ctx* ctx, svgp_laplace* la, const svgp_laplace_desc* desc, const void* f_init, double* lml_out,
                              svgp_laplace_info* info, double* d_variance, double* d_inv_lengthscale);
int32_t svgp_laplace_mode(svgp_ctx* ctx, svgp_laplace* la, void* f_out, void* dll_out, void* W_out);
int32_t svgp_laplace_predict(svgp_ctx* ctx, svgp_laplace* la, int32_t layout, int64_t n, const void* x_host, void* mean_out,
                             void* var_out, void* cov_out);
int32_t svgp_laplace_predict_cross_cov(svgp_ctx* ctx, svgp_laplace* la, int32_t layout, int64_t nx, const void* x_host, int64_t ny,
                                       const void* y_host, void* cov_out);
int32_t svgp_laplace_free(svgp_ctx* ctx, svgp_laplace* la);

/* ---- the NearestNeighbors (Vecchia) approximation: NearestNeighbors(k) / posterior / approx_lml  (src/NearestNeighborsModule.jl) ----
 * p(f) = prod_i p(f_i | f_ns(i)), ns(i) = the m = min(i, k) points BEFORE i in the order of the data handle (the reference's index
 * order; any reordering is the caller's).  Per point (0-based i), C = k(ns, ns) + diag I, c = k(ns, x_i), kd = k(x_i, x_i) + diag:
 *   b_i = C \ c (make_row :27-29),  F_i = kd - c' b_i (make_F :46-61; F_0 = kd),  delta = y - mean_const,  r_i = delta_i - b_i' delta_ns
 *   approx_lml = -1/2 sum_i (log 2 pi + log F_i + r_i^2 / F_i)   (:108-113: logdet(InvRoot(U)) = sum log F_i, alpha' delta = sum r_i^2 / F_i)
 * one dense Cholesky of order <= k per point, one wavefront each; N is bounded by device memory only (no N x N matrix).
 * diag: the reference builds U from the kernel alone and ignores fx.Sigma_y (:100-101): diag = 0 is the reference.  diag = sigma^2
 * gives the Vecchia approximation of logpdf(fx, y) itself (k = N - 1: the exact GP).  The reference solves by LU; here Cholesky, and
 * a block or an F_i that is not positive is reported: SVGP_NOT_POSDEF, svgp_nn_info.first_bad = 1-based index of the first such point,
 * lml = NaN.  "Not positive" is: at or below 4 eps (m + 1) kd, the rounding noise of kd - c' b_i in the data dtype (an exactly repeated
 * point with diag = 0 leaves +-1e-16 of either sign there, not an exact zero).
 *   svgp_nn_lml        the value.  k >= N is k = N - 1; N = 1 is valid.
 *   svgp_nn_lml_grad   value, d / d variance, d / d inv_lengthscale (d entries) and, when d_diag is not NULL, d / d diag: closed form,
 *                      gF = -1/(2F) + r^2/(2F^2), w = C \ delta_ns: kd_bar = gF, c_bar = -2 gF b + (r/F) w,
 *                      C_bar = gF b b' - (r/F) sym(w b').  x, y and mean_const are not differentiated.
 *   svgp_nn_fit        the value, and caches b_i, F_i and alpha = U (U' delta) (:103) on the handle for the calls below.
 *   svgp_nn_factors    B_out: N x kb column-major, kb = min(k, N - 1), B(i, t) = the coefficient of point i on point i - kb + t (zero
 *                      where that index is negative: the rows i < kb are shorter); F_out, alpha_out: N.  Data dtype, any may be NULL.
 *   svgp_nn_predict    PosteriorGP with C = InvRoot(U): mean = mean_const + k(x*, x) alpha, var = k(x*, x*) - colsumsq(V),
 *                      cov = k(x*, x*) - V'V, V = U' k(x, x*): row i = (k(x_i, x*) - sum_j B_ij k(x_j, x*)) / sqrt(F_i).  n values
 *                      (mean, var) / n x n column-major (cov), data dtype, any may be NULL.  x* in `layout` with the data's d.
 *   svgp_nn_predict_cross_cov   cov(x*, y*) = k(x*, y*) - Vx' Vy, nx x ny column-major.
 * Workspace rule of the predictions: V is streamed in row tiles of min(2048, 2^23 / n*p) points (a multiple of 64, at least 64; n*p =
 * n* rounded up to 128) and never held at N x n*; so N * n* is not capped, n* is: 4096 for cov / cross-cov (the n*p x n*p accumulator),
 * 131072 for mean / var in one call - beyond them SVGP_UNSUPPORTED, the caller tiles x*.
 * fp64 and fp32 data (F_i, r_i and every sum over points in fp64 for both); SE / Matern-3/2 / Matern-5/2 with ARD, d <= SVGP_MAX_D;
 * 1 <= min(k, N - 1) <= 64 neighbours (more: SVGP_UNSUPPORTED; k >= N counts as N - 1, so it is valid up to N = 65).  Every result is bitwise repeatable: fixed-order reductions, no floating-point atomics.
 * SVGP_INVALID_ARG, before anything is enqueued: NULL required pointers, data without y, a descriptor whose dtype / d differ from the
 * data's, k < 1, variance <= 0, diag < 0, reserved != 0; factors / predict before a successful fit.  Never collective: on a context
 * with a communicator these calls stay local.  Found by symbol (no ABI version step).
 *
 * Neighbour tables.  A handle may carry a table nbr: N x kb int32, column-major like B, kb = min(k, N - 1) <= 64.  Row i lists the
 * conditioning set of point i: its m_i <= min(i, kb) valid entries first, each in [0, i) and distinct, then -1.  With a table set,
 * ns(i) is row i in place of the window of the previous k points (the Vecchia / NNGP form: GpGp, GPvecchia, Datta et al.'s NNGP);
 * svgp_nn_lml, _lml_grad, _fit, _factors, _predict and _predict_cross_cov use it.  desc->k must give the table's kb (min(desc->k,
 * N - 1) == kb), else SVGP_INVALID_ARG.  svgp_nn_factors then returns B(i, t) = the coefficient of point i on point nbr(i, t), 0 where
 * that entry is -1.  Without a table every call is what it was.  The ordering of the points stays the caller's.
 *   svgp_nn_set_neighbors    uploads a caller's table (N x kb, k as in the descriptor) and validates it on the device; a row that breaks
 *                            the rule above: SVGP_INVALID_ARG, svgp_last_error names the first such row (1-based).
 *   svgp_nn_build_neighbors  the exact k nearest predecessors: for every i the min(i, kb) points j < i with the smallest
 *                            sum_f ((x_j,f - x_i,f) il_f)^2, computed from differences in the data dtype; ties go to the lower index;
 *                            rows in ascending index.  inv_lengthscale: d entries, NULL: ones.  Brute force, N^2 / 2 distances; for
 *                            sorted 1-D inputs the result is the window.  A distance that is not finite is never chosen.
 *   svgp_nn_get_neighbors    *k_out = kb of the handle's table, -1 without one; nbr_out (may be NULL) receives the N x kb table.
 *   svgp_nn_clear_neighbors  back to the window.
 * Setting, building or clearing a table discards the handle's fit: factors / predict return SVGP_INVALID_ARG until the next
 * svgp_nn_fit.  A failed set or build leaves the handle with no table.  N must fit int32 (else SVGP_UNSUPPORTED).
 * The gradient is taken at a FIXED table: a table built with the inverse lengthscales as its metric is piecewise constant in them,
 * and svgp_nn_lml_grad does not (and cannot) differentiate the selection.  Bitwise repeatable like the rest: the search uses no
 * atomics, the reverse lists behind alpha come from a stable sort, the validation from one integer atomicMin.
 *
 * Local predictions (nearest-neighbour kriging: GpGp `predictions`, GPvecchia, spNNGP).  svgp_nn_predict is PosteriorGP with the
 * global U: N kernel evaluations per test point ((kb + 1) N with a table).  svgp_nn_predict_local conditions every test point on
 * its own kq = min(k, N) nearest OBSERVED points instead:
 *   ns* = the kq training points j with the smallest sum_f ((x_j,f - x*_f) il_f)^2 (il: the fit's inverse lengthscales; differences in
 *         the data dtype, ties to the lower index, ascending index, a distance that is not finite is never chosen)
 *   C = k(ns*, ns*) + diag I,  c = k(ns*, x*)
 *   mean(x*) = mean_const + c' C^-1 (y_ns* - mean_const),   var(x*) = k(x*, x*) - c' C^-1 c
 * var is the latent variance like svgp_nn_predict's (k(x*, x*) carries no diag) and is returned as computed: a test point on top of
 * a training point at diag = 0 leaves +- rounding noise there.  The test points are independent of each other (no joint covariance).
 * Cost per test point: N distances (3 d flops, no exp) and one block of order kq, ~ kq^2 (3 d + 20) / 2 + kq^3 / 3; no N x n* object
 * and no fit-time state beyond the data: the call uses the last successful svgp_nn_fit's kernel, variance, inverse lengthscales,
 * diag and mean_const, and neither the handle's table nor B, F or alpha (k is this call's own; setting, building or clearing a
 * table still discards the fit, the rule above, and with it this call).
 *   k >= 1, min(k, N) <= 64 (more: SVGP_UNSUPPORTED; k > N counts as N); N must fit int32 (else SVGP_UNSUPPORTED).
 *   mean_out / var_out: n values, data dtype, either may be NULL.  nbr_out (may be NULL): the n x kq table of the ns*, int32
 *   column-major like the training table, a short row (fewer than kq finite distances) ends in -1.  x* in `layout` with the data's d.
 *   The test points are processed in rounds of 32768, which is the whole workspace (32768 (d + 2) elements and 32768 kq int32):
 *   n is bounded by host memory only, and the rounds change no result bit.
 *   A test point with a coordinate that is not finite: mean = var = NaN for that point (never the prior), SVGP_OK.
 *   A block with a pivot at or below 4 eps (m + 1) (variance + diag) - repeated training points at diag = 0 - is "not positive":
 *   mean = var = NaN for that test point, every other one is still written, SVGP_NOT_POSDEF, and svgp_last_error names the first such
 *   test point (1-based; one integer atomicMin).
 *   SVGP_INVALID_ARG, before anything is enqueued: NULL ctx / nn / x_host, n < 1, k < 1, no successful fit, a bad layout.
 * Never collective.  Bitwise repeatable: the search uses no atomics, F and the mean's sum are accumulated in fp64 in a fixed order.
 *
 * Per-point noise variances and prior-mean offsets.  A handle may carry N noise variances s and N mean offsets mu (svgp_point_noise,
 * svgp_point_mean: the collapsed bound's and the CG handle's structs and convention):
 *   sigma_j^2 = T(desc.diag) + s_j   in the data dtype T with one rounding,      delta_j = y_j - mean_const - mu_j
 *   C = k(ns, ns) + diag(sigma^2_ns),  kd = variance + sigma_i^2;  b, F, r, lml and alpha as above
 * in svgp_nn_lml, _lml_grad, _fit (and with it _factors, _predict, _predict_cross_cov, which read the new alpha, B and F) and in
 * svgp_nn_predict_local (C = k(ns*, ns*) + diag(sigma^2_ns*), mean = mean_const + c' C^-1 delta_ns*), with the window or a table.
 * A mean function's value at x* is the caller's to add (svgp_predict's rule).  Known measurement errors, a fixed-noise model, a
 * learned noise or mean function (AbstractGPs' Diagonal Sigma_y, GPyTorch's FixedNoiseGaussianLikelihood).
 *   svgp_nn_set_noise  N values of the data dtype, host or device memory (pn->on_device), copied into the handle: a snapshot.
 *           pn = NULL removes the vector: every call is then bitwise what it is on a handle that never had one.  Discards the fit,
 *           as a table call does: factors / predict return SVGP_INVALID_ARG until the next fit.  One NaN-propagating min-reduction of
 *           s runs on the device at set time and its result is kept on the host: a later lml / lml_grad / fit / lml_grad_points fails
 *           BEFORE its data pass with SVGP_NOT_POSDEF when T(desc.diag) + min s is < 0 or NaN; lml = NaN, info->first_bad = 0, and
 *           the handle stays healthy.  Zero is allowed, as diag = 0 is.
 *   svgp_nn_set_mean   N offsets mu under the same rules.  A NaN in mu gives lml = NaN with SVGP_OK (the collapsed calls' rule).
 *   "Not positive" becomes: at or below 4 eps (m + 1) (variance + the largest sigma^2 of the block, point i included); without a
 *           vector that is the value above.  d / d variance of svgp_nn_lml_grad becomes (gF (F - sigma_i^2) - sum_t sigma_t^2 q_t) /
 *           variance per point, q_t = gF b_t^2 - (r/F) w_t b_t the diagonal of C_bar; d_diag keeps its meaning, the derivative with
 *           respect to the common term.
 *   svgp_nn_lml_grad_points  svgp_nn_lml_grad's arguments, then d_mean_const, gpm and gpn (each of the three may be NULL):
 *           s_bar_j    = d lml / d sigma_j^2 = gF_j + sum_{(i, t): ns(i)_t = j} (gF_i b_it^2 - (r_i / F_i) w_it b_it)      -> gpn->s_bar
 *           mean_bar_j = d lml / d mu_j      = alpha_j = r_j / F_j - sum_{(i, t): ns(i)_t = j} b_it r_i / F_i              -> gpm->mu_bar
 *           d_mean_const = sum_j alpha_j,   d_diag = sum_j s_bar_j (the scalar is the per-point slots' sum, as in svgp_nn_lml_grad)
 *           N values each in the data dtype, host or device memory (->on_device).  Works with or without vectors set.  The point
 *           kernel stores b_i, F_i, r_i / F_i, gF_i and the per-pair term laid out like B; two gathers follow in a fixed order: the
 *           window over the <= kb later rows, a table over its reverse lists, one wavefront per j, the lanes striding the list, a
 *           fixed tree.  Sums in fp64, rounded once to the data dtype; no floating-point atomics: repeated calls and host / device
 *           output are bitwise equal, and lml, d_variance, d_inv_lengthscale and d_diag are bitwise those of svgp_nn_lml_grad on the
 *           same handle state.  The call leaves the handle FITTED at desc (b_i, F_i and alpha are those of svgp_nn_fit: mean_bar is
 *           the fit's alpha), replacing an earlier fit.  Workspace beyond a fit's: N x kb elements of the data dtype (the per-pair
 *           terms) and three N-vectors (gF and s_bar in fp64, one staging vector).  SVGP_NOT_POSDEF: the vectors are not written.
 * SVGP_INVALID_ARG, before anything is enqueued: NULL pn->s / pm->mu / gpm->mu_bar / gpn->s_bar, on_device not 0 / 1, reserved != 0,
 * and what svgp_nn_lml_grad rejects.  The existing instantiations of the point kernels run whenever no vector is set (lml, lml_grad,
 * fit, predict_local): the vectors and the per-point gradient live in sibling instantiations.  Out of scope: a full noise
 * covariance, gradients with respect to x, the selection of a table.  Found by symbol (no ABI version step). */
typedef struct svgp_nn svgp_nn;
typedef struct svgp_nn_desc {
  int32_t dtype;            /* SVGP_F64 | SVGP_F32: must be the data's */
  int32_t kernel;           /* SVGP_KERNEL_* */
  int32_t d;                /* must be the data's */
  int32_t k;                /* neighbours: >= 1, min(k, N - 1) <= 64 */
  double variance;          /* kernel variance */
  const double* inv_lengthscale; /* d entries */
  double diag;              /* added to every diagonal entry (0: the reference) */
  double mean_const;        /* ConstMean value, 0 for ZeroMean */
  int64_t reserved;         /* must be 0 */
} svgp_nn_desc;             /* 56 bytes */
typedef struct svgp_nn_info {
  int64_t first_bad;        /* 0, or the 1-based index of the first point whose block or F_i is not positive */
  int64_t n_neg_f;          /* number of points with F_i <= 0 */
  double lml;
} svgp_nn_info;             /* 24 bytes */
int32_t svgp_nn_create(svgp_ctx* ctx, const svgp_data* data, svgp_nn** out);
int32_t svgp_nn_lml(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info);
int32_t svgp_nn_lml_grad(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info, double* d_variance,
                         double* d_inv_lengthscale, double* d_diag);
int32_t svgp_nn_fit(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info);
int32_t svgp_nn_factors(svgp_ctx* ctx, svgp_nn* nn, void* B_out, void* F_out, void* alpha_out);
int32_t svgp_nn_predict(svgp_ctx* ctx, svgp_nn* nn, int32_t layout, int64_t n, const void* x_host, void* mean_out, void* var_out,
                        void* cov_out);
int32_t svgp_nn_predict_cross_cov(svgp_ctx* ctx, svgp_nn* nn, int32_t layout, int64_t nx, const void* x_host, int64_t ny,
                                  const void* y_host, void* cov_out);
int32_t svgp_nn_free(svgp_ctx* ctx, svgp_nn* nn);
int32_t svgp_nn_set_neighbors(svgp_ctx* ctx, svgp_nn* nn, int32_t k, const int32_t* nbr_host);
int32_t svgp_nn_build_neighbors(svgp_ctx* ctx, svgp_nn* nn, int32_t k, const double* inv_lengthscale);
int32_t svgp_nn_get_neighbors(svgp_ctx* ctx, svgp_nn* nn, int32_t* k_out, int32_t* nbr_out);
int32_t svgp_nn_clear_neighbors(svgp_ctx* ctx, svgp_nn* nn);
int32_t svgp_nn_predict_local(svgp_ctx* ctx, svgp_nn* nn, int32_t layout, int64_t n, const void* x_host, int32_t k, void* mean_out,
                              void* var_out, int32_t* nbr_out);
struct svgp_point_noise;        /* defined with the collapsed bound below; svgp_point_mean: with svgp_elbo_with_mean above */
struct svgp_point_noise_grad;
int32_t svgp_nn_set_noise(svgp_ctx* ctx, svgp_nn* nn, const struct svgp_point_noise* pn);
int32_t svgp_nn_set_mean(svgp_ctx* ctx, svgp_nn* nn, const svgp_point_mean* pm);
int32_t svgp_nn_lml_grad_points(svgp_ctx* ctx, svgp_nn* nn, const svgp_nn_desc* desc, double* lml_out, svgp_nn_info* info,
                                double* d_variance, double* d_inv_lengthscale, double* d_diag, double* d_mean_const,
                                svgp_point_mean_grad* gpm, struct svgp_point_noise_grad* gpn);

/* ---- the collapsed bound of sparse GP regression and the optimal q(u)  (Titsias 2009, eqs. 11 / 12) ---------------------------------
 * For the Gaussian likelihood the q(u) that maximises the ELBO has a closed form; the reference's tests build it on the host
 * (test/test_utils.jl:7-17, optimal_variational_posterior), its user guide calls it "the optimal form for q(u)", and
 * test/SparseVariationalApproximationModule.jl:99-134 ties the SVGP posterior at that q to AbstractGPs' posterior(VFE(fz), fx, y) and
 * to exact GP regression.  With Kuu = k(z, z) + jitter I = Lk Lk', A = Lk \ Kuf over the window [batch_off, batch_off + batch_len) = n
 * points, r = y - mean_const, C = A A', b = A r, t = tr C, rr = r'r, B = I + C / sigma^2 = LB LB', c = LB \ b / sigma^2:
 *   bound = -n/2 log(2 pi sigma^2) - sum log diag LB - rr / (2 sigma^2) + c'c / 2 - (n variance - t) / (2 sigma^2)
 *         = log N(r | 0, Qff + sigma^2 I)  [fit]  - tr(Kff - Qff) / (2 sigma^2)  [trace]          (the ELBO at the optimal q, num_data = n)
 *   optimal whitened q: m_w = LB' \ c, S_w = inv(B);  Centered: m = mean_const + Lk m_w, Lq = Lk chol(S_w)
 * One data pass (2 M^2 flops per point: a triangular solve and a SYRK, the count of svgp_elbo); only a point-major chunk of A
 * (<= 65 536 points) lives in device memory, Kuf and A of the whole batch never exist.  The M-sized tail - B, its Cholesky factor, c,
 * inv(B) and its factor - runs in fp64 whatever the model's dtype: cond(B) = 1 + lambda_max(C) / sigma^2 grows with n.
 *   svgp_collapsed_bound  the bound and its terms.  The model's q is not read and not changed.
 *   svgp_collapsed_q      also WRITES the optimal q into the model's device-resident m and Lq, in the model's own parametrisation
 *                         (device to device; the model is prepared again, lazily): every later call on the model - svgp_elbo,
 *                         svgp_elbo_grad*, svgp_posterior, svgp_predict*, svgp_marginals - sees it.  m_out (M) / Lq_out (M x M column-major,
 *                         upper triangle zeroed): host arrays in the dtype and layout of the descriptor's m / Lq; either may be NULL.
 *   svgp_collapsed_grad   svgp_collapsed_q, then the existing value-and-gradient at that q with num_data = batch_len.  d elbo / d q = 0
 *                         there, so grads_out holds the TOTAL derivatives of the bound in variance, lik_sigma2, mean_const, the inverse
 *                         lengthscales and z; grads_out->m and grads_out->Lq must be NULL.  gx: as in svgp_elbo_grad_inputs, NULL for no
 *                         x_bar.  bound_out is the collapsed bound (not the second pass's ELBO, which equals it to rounding).
 * A NaN coordinate or observation gives NaN results with SVGP_OK (the rule of svgp_elbo); svgp_collapsed_q then writes NaN.  Results
 * are bitwise repeatable call to call: fixed splits, fixed-order sums, no floating-point atomics.
 * SVGP_INVALID_ARG, before anything is enqueued: a likelihood other than SVGP_LIK_GAUSSIAN, a window outside the data, data without
 * y, a dtype / d that differs from the model's, (grad) a NULL grads_out or non-NULL grads_out->m / ->Lq or a bad gx.
 * SVGP_UNSUPPORTED: a context with a communicator attached, a model carrying muz (prior mean offsets and per-point noise variances:
 * the svgp_collapsed_*_with_noise calls below).  Multi-GPU evaluation is out of scope.  SVGP_NOT_POSDEF: a non-positive pivot of Kuu (chol_info) or of B (chol_info_b); the model's
 * q is then left as it was.  For Kuu "non-positive" includes a pivot at or below its rounding noise, 4 eps (i + 1) (variance + jitter)
 * in the model's dtype: an exactly repeated inducing point at jitter 0 leaves +-1e-16 there, not an exact zero, and A = Lk \\ Kuf
 * built on it would be noise (the existing calls keep LAPACK's rule, pivot <= 0).  Found by symbol (no ABI version step). */
typedef struct svgp_collapsed_terms {
  double bound;        /* fit + trace */
  double fit;          /* log N(r | 0, Qff + sigma^2 I) */
  double trace;        /* -(n variance - tr C) / (2 sigma^2) */
  double logdet_B;     /* 2 sum log diag LB */
  double logdet_kuu;   /* 2 sum log diag Lk */
  int64_t n_points;
  int32_t chol_info;   /* 0, or the order of the first non-positive leading minor of Kuu */
  int32_t chol_info_b; /* 0, or that of B (of inv(B), should its factorisation fail instead) */
  int64_t reserved;    /* 0 */
} svgp_collapsed_terms; /* 64 bytes */
int32_t svgp_collapsed_bound(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                             double* bound_out, svgp_collapsed_terms* terms_out);
int32_t svgp_collapsed_q(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len, void* m_out,
                         void* Lq_out, double* bound_out);
int32_t svgp_collapsed_grad(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                            double* bound_out, svgp_collapsed_terms* terms_out, svgp_grads* grads_out, const svgp_input_grad* gx);

/* ---- the collapsed bound with per-point noise variances and any prior mean ----------------------------------------------------------
 * AbstractGPs' VFE accepts f(x, Sigma_y::Diagonal) (Kuf / chol(Sigma_y).U, trace term sum_j (k_jj - q_jj) / Sigma_y_jj) and any mean
 * function.  The caller evaluates the O(n) functions - the noise vector and the mean at x and at z - and these calls do the
 * O(n M^2) work.  With s = pn->s and mux = pm->mu over the window (each NULL: zeros) and A = Lk \ Kuf:
 *   sigma_j^2 = lik_sigma2 + s_j (the per-point term ADDS to the descriptor's variance, as mux adds to mean_const),  w_j = 1 / sigma_j^2,
 *   r_j = y_j - mean_const - mux_j,  C = sum_j w_j a_j a_j',  b = sum_j w_j a_j r_j,  rr = sum_j w_j r_j^2,
 *   t = sum_j w_j (variance - |a_j|^2),  ld = sum_j log sigma_j^2,  B = I + C = LB LB',  c = LB \ b
 *   bound = -n/2 log 2 pi - ld / 2 - sum log diag LB - rr / 2 + c'c / 2 - t / 2
 *         = log N(r | 0, Qff + diag sigma^2)  [fit]  - 1/2 sum_j (k_jj - q_jj) / sigma_j^2  [trace]
 *   optimal whitened q: m_w = LB' \ c, S_w = inv(B);  Centered: m = mean_const + muz + Lk m_w, Lq = Lk chol(S_w)
 * The bound does not depend on muz (svgp_model_set_mean_z): it enters the Centered m only, and a model carrying it is accepted here
 * (the three calls above keep their SVGP_UNSUPPORTED).  pm, pn, gpm, gpn and gx may each be NULL; with pm = pn = NULL and no muz every
 * output is bitwise that of the corresponding call above (the same launches).  s / s_bar: batch_len values in the data's dtype,
 * element j belongs to point batch_off + j, in host or device memory as svgp_point_mean / _grad; nothing past batch_len is touched.
 *   svgp_collapsed_grad_with_noise  also  s_bar_j = d bound / d sigma_j^2 = -1 / (2 sigma_j^2) + ((r_j - mu~_j)^2 + v_j) / (2 sigma_j^4)
 *                                   into gpn and mux_bar_j = (r_j - mu~_j) / sigma_j^2 into gpm (mu~, v: the marginals of the optimal
 *                                   q without the prior mean); grads_out->lik_sigma2 = sum_j s_bar_j keeps its meaning.
 * With pn the data pass computes C with per-point weights (the weighted SYRK of the non-Gaussian value-and-gradient) and the
 * gradient pass takes that route too; the M-sized tail is unchanged, fp64.  Results stay bitwise repeatable.
 * Statuses: those of the calls above and of svgp_point_mean, before anything is enqueued; SVGP_INVALID_ARG: NULL pn->s or
 * gpn->s_bar, on_device not 0 / 1, reserved != 0; SVGP_NOT_POSDEF with the model's q untouched: any sigma_j^2 <= 0 (the reference
 * throws from cholesky(Sigma_y)), found before the data pass; NaN results with SVGP_OK: a NaN in s, mux, x or y; SVGP_UNSUPPORTED: a
 * communicator attached.  terms_out keeps its struct: fit and trace take the meanings above.  Found by symbol. */
typedef struct svgp_point_noise {        /* s: batch_len values in the data's dtype, element j belongs to point batch_off + j */
  const void* s;
  int32_t on_device;   /* 0: host memory, 1: device memory */
  int32_t reserved;    /* 0 */
} svgp_point_noise;      /* 16 bytes */
typedef struct svgp_point_noise_grad {   /* s_bar: batch_len values in the data's dtype, element j belongs to point batch_off + j */
  void* s_bar;
  int32_t on_device;
  int32_t reserved;
} svgp_point_noise_grad; /* 16 bytes */
int32_t svgp_collapsed_bound_with_noise(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                                        const svgp_point_mean* pm, const svgp_point_noise* pn, double* bound_out,
                                        svgp_collapsed_terms* terms_out);
int32_t svgp_collapsed_q_with_noise(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                                    const svgp_point_mean* pm, const svgp_point_noise* pn, void* m_out, void* Lq_out,
                                    double* bound_out);
int32_t svgp_collapsed_grad_with_noise(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                                       const svgp_point_mean* pm, const svgp_point_noise* pn, double* bound_out,
                                       svgp_collapsed_terms* terms_out, svgp_grads* grads_out, const svgp_input_grad* gx,
                                       svgp_point_mean_grad* gpm, svgp_point_noise_grad* gpn);

/* ---- natural-gradient steps on q(u) -------------------------------------------------------------------------------------------------
 * The reference trains q = N(m, Lq Lq') with the optimiser that trains everything else: svgp_elbo_grad hands it the Euclidean
 * m_bar / Lq_bar of the ELBO (SVA:340-373).  A natural-gradient step moves q along the ELBO's gradient in the expectation parameters
 * instead (Hensman et al. 2013; GPflow's NaturalGradient, GPyTorch's NGD) and costs one value-and-gradient pass plus an M-sized tail.
 * In whitened coordinates - q(v) = N(m_w, S_w), u = mean_const + Lk v, Lambda = inv(S_w) - with A = Lk \ Kuf over the window, the
 * likelihood's point gradients g_mu = dE/dmu, g_v = dE/dv at the marginals of the current q (SVA:354-355) and
 * scale = num_data / batch_len:
 *     W = A diag(-2 scale g_v) A',   a = scale A g_mu
 *     Lambda'      = (1 - gamma) Lambda     + gamma (I + W)
 *     Lambda' m_w' = (1 - gamma) Lambda m_w + gamma (a + W m_w)
 *     S_w'         = inv(Lambda')
 * which is theta' = theta + gamma dL/d eta for the natural parameters theta = (Lambda m_w, -Lambda / 2) and the expectation parameters
 * eta = (m_w, S_w + m_w m_w').  gamma = 1 with the Gaussian likelihood on the full batch is svgp_collapsed_q; any likelihood, any
 * minibatch with num_data and any gamma in (0, 1] are covered here.
 *   svgp_natgrad_step      the data pass of svgp_elbo_grad, unchanged, then the tail.  The new q is WRITTEN into the model's
 *                          device-resident m and Lq, in the model's own parametrisation (NonCentered: m = m_w', Lq = chol(S_w');
 *                          Centered: m = mean_const + Lk m_w', Lq = Lk chol(S_w')), device to device; the model is prepared again, lazily.
 *                          elbo_out, terms_out and every block of grads_out (NULL: none wanted; grads_out->m / ->Lq are allowed) are the
 *                          values at the q the call STARTED from, bitwise what svgp_elbo_grad returns for the same inputs on the same
 *                          context: one call serves an optimiser step on the hyperparameters and moves q.  m_out (M) / Lq_out (M x M
 *                          column-major, upper triangle zeroed): host arrays in the dtype and layout of the descriptor's m / Lq, the new q;
 *                          either may be NULL.
 *   svgp_natgrad_step_ext  the same with the caller's point gradients: the counterpart of svgp_elbo_grad_ext (sum_e, g_mu, g_v as there).
 *   svgp_model_update_keep_q   svgp_model_update with desc->m / desc->Lq ignored (they may be NULL): kernel parameters, z, likelihood
 *                          parameters, jitter and mean_const go up, the device-resident q stays - no M x M upload.  For a Centered model
 *                          the stored q is in u-space and is kept as is (the same u-space q under the new kernel, not the same whitened q).
 * The tail runs in fp64 whatever the model's dtype (cond(Lambda') grows with num_data); Lambda is formed as B^-T B^-1 from the explicit
 * inverse of the whitened factor B, and at gamma = 1 exactly it is neither formed nor read.  Results are bitwise repeatable call to
 * call: fixed splits, fixed-order sums, no floating-point atomics.
 * SVGP_INVALID_ARG, before anything is enqueued: gamma outside (0, 1] or not finite, and everything svgp_elbo_grad / _ext reject.
 * SVGP_UNSUPPORTED: a context with a communicator attached, a model carrying muz (there are no mux variants): multi-GPU evaluation and
 * prior mean offsets are out of scope, as for the collapsed calls.  SVGP_NOT_POSDEF, with q left exactly as it was: Lambda' (or its
 * inverse) not positive definite - possible with a caller's g_v > 0 only, the built-in likelihoods being log-concave in f - or, at
 * gamma < 1, a non-positive diagonal entry of the whitened factor of q; svgp_last_error names the order of the failing minor.  A
 * non-positive pivot of Kuu and SVGP_NEG_VARIANCE (the model's policy) are reported as by svgp_elbo_grad, q untouched.  A NaN coordinate
 * or observation gives NaN outputs with SVGP_OK and q is then written NaN (the rule of svgp_collapsed_q).  Found by symbol (no ABI
 * version step). */
int32_t svgp_natgrad_step(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len, double num_data,
                          double gamma, double* elbo_out, svgp_terms* terms_out, svgp_grads* grads_out, void* m_out, void* Lq_out);
int32_t svgp_natgrad_step_ext(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len, double num_data,
                              double gamma, double sum_e, const double* g_mu, const double* g_v, double* elbo_out, svgp_terms* terms_out,
                              svgp_grads* grads_out, void* m_out, void* Lq_out);
int32_t svgp_model_update_keep_q(svgp_ctx* ctx, svgp_model* model, const svgp_model_desc* desc);

/* ---- the predictive distribution of the OBSERVATION: held-out log density and predictions of y -------------------------------------
 * What svgp_marginals / svgp_predict / svgp_laplace_predict return is the latent marginal N(mu_i, v_i) of f.  These two calls push it
 * through the likelihood on the device (GPflow: predict_y / predict_log_density; GPyTorch: likelihood(model(x))):
 *   lpd_i   = log p(y_i | D) = log int p(y_i | f) N(f; mu_i, v_i) df        the held-out log density; NLPD = -mean(lpd)
 *   ymean_i = E[y_i],  yvar_i = Var[y_i]                                    no y needed
 * lpd_i is NOT the ELBO's E_q[log p(y_i | f_i)], which bounds it from below (Jensen).  Per likelihood, with v_i including the 1e-18 of
 * svgp_marginals and e1 = exp(mu + v / 2):
 *   Gaussian              lpd = log N(y; mu, v + sigma2)                                  (mu, v + sigma2)
 *   Bernoulli, normcdf    lpd = log Phi(+-mu / sqrt(1 + v))                               p = Phi(mu / sqrt(1 + v)):  (p, p (1 - p))
 *   Bernoulli, logistic   lpd by quadrature                                               p = E[sigmoid(f)] by quadrature:  (p, p (1 - p))
 *   Poisson, exp link     lpd by quadrature                                               (e1, e1 + expm1(v) e1^2)
 *   Exponential(scale e^f)  lpd by quadrature                                             (e1, exp(2 mu + 2 v) + expm1(v) e1^2)
 *   Gamma(alpha, scale e^f) lpd by quadrature                                             (alpha e1, alpha exp(2 mu + 2 v) + alpha^2 expm1(v) e1^2)
 * Quadrature is Gauss-Hermite in the log domain, logsumexp_q(log w_q + log p(y | f_q)) with f_q = mu + sqrt(2 v) x_q and a running
 * maximum: finite for a Poisson count of several hundred; weights that underflowed to 0 at high orders are skipped.  quadrature_n > 0
 * forces GH-n for lpd of every likelihood; quadrature_n == 0 means the closed form where one exists (Gaussian, normcdf Bernoulli), else
 * GH-20 - the rule svgp_model_desc documents for the ELBO, except that Poisson / Exponential / Gamma, whose ELBO term is closed, have no
 * closed-form predictive density and take GH-20 here, and that the normcdf Bernoulli, whose ELBO term takes GH-20, is closed here.  The
 * moments use their closed forms whenever they exist, whatever quadrature_n is (logistic: GH-n, or GH-20).
 *   svgp_predictive       data-resident: ONE forward data pass, the one svgp_elbo runs (same prep, same strips, overlapped where svgp_elbo
 *                         overlaps them), then the point stage.  pm: the batch's prior mean offsets as in svgp_marginals_with_mean, or NULL.
 *                         A model carrying muz (svgp_model_set_mean_z) is honoured as svgp_elbo_with_mean honours it.
 *   svgp_lik_predictive   array form, for Laplace / NearestNeighbors / any caller holding latent marginals: no model, no data pass.  mu, var,
 *                         y: n host doubles each; var is the marginal variance itself (svgp_marginals' output holds the 1e-18 already).
 *                         likelihood is a SVGP_LIK_* code, lik_param the Gaussian sigma2 / the Gamma shape alpha (ignored otherwise).
 * Outputs (host, fp64, batch_len / n each; any may be NULL, not all): summary_out, lpd_out, ymean_out, yvar_out.  Without observations -
 * a data object uploaded without y, or y == NULL in the array form - summary_out and lpd_out must be NULL (SVGP_INVALID_ARG before
 * anything is enqueued); ymean_out and yvar_out still work.
 * Both calls are ALWAYS LOCAL, like svgp_elbo_partial: on a context with a communicator nothing is all-reduced, and a data-parallel
 * host adds the ranks' summaries itself.  svgp_elbo on the same model before and after is bitwise unchanged; both calls are bitwise
 * repeatable (fixed-order sums, no atomics).
 * Negative variances follow the model's neg_var_policy exactly as in svgp_elbo: a point with v_i < 0 is counted in n_neg_var; under
 * SVGP_NEGVAR_CLAMP it is evaluated at v_i = 0 (the quadrature then collapses to log p(y_i | mu_i)); under SVGP_NEGVAR_ERROR it is left
 * out of both sums and of n_points, its per-point outputs are NaN, every other point's are valid, and the status is SVGP_NEG_VARIANCE
 * (outputs and summary are written all the same).  svgp_lik_predictive treats var[i] < 0 as the error policy does.  Non-finite inputs give
 * non-finite outputs with SVGP_OK, as in svgp_elbo.  SVGP_NOT_POSDEF as in svgp_elbo.  SVGP_INVALID_ARG, before anything is enqueued:
 * what svgp_marginals_with_mean rejects, no output requested, n < 1, NULL mu / var, quadrature_n outside 0..512, sigma2 / alpha <= 0 where
 * the likelihood reads it; SVGP_UNSUPPORTED: a likelihood code outside SVGP_LIK_*.  svgp_last_timing reports svgp_predictive like a
 * forward evaluation, the point stage in ms_expect; svgp_lik_predictive reports its point stage alone.  fp32 models: the data pass is
 * fp32, the point stage fp64 on its moments.  Found by symbol (no ABI version step). */
typedef struct svgp_pred_summary {
  double sum_lpd;     /* sum_i log p(y_i | D) over the points that counted */
  double sum_sq_err;  /* sum_i (y_i - E[y_i])^2 over the same points: RMSE = sqrt(sum_sq_err / n_points) */
  int64_t n_points;
  int64_t n_neg_var;
} svgp_pred_summary;   /* 32 bytes */
int32_t svgp_predictive(svgp_ctx* ctx, svgp_model* model, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                        const svgp_point_mean* pm, svgp_pred_summary* summary_out, double* lpd_out, double* ymean_out, double* yvar_out);
int32_t svgp_lik_predictive(svgp_ctx* ctx, int32_t likelihood, double lik_param, int32_t quadrature_n, int64_t n, const double* mu,
                            const double* var, const double* y, svgp_pred_summary* summary_out, double* lpd_out, double* ymean_out,
                            double* yvar_out);

/* ---- pathwise posterior function samples (Wilson et al. 2020, Matheron's rule) ---------------------------------------------------
 * S functions drawn from the fitted posterior, each one a FUNCTION that can be evaluated at any points, any number of times:
 *   f_s(x) = mean(x) + sum_l phi_l(x) w_sl + sum_i k(x, z_i) V_is,        V_s = Kuu^-1 (u_s - mean(z) - Phi(z) w_s),   u_s ~ q(u)
 *   phi_l(x) = sqrt(2 variance / L) cos(sum_k omega_lk invl_k x_k + tau_l)
 * The library draws nothing: the caller supplies every random number (svgp_sample_basis), so a result is a deterministic function of its
 * inputs.  omega are frequencies of the UNIT-lengthscale base kernel (SE: N(0, I); Matern-nu: g sqrt(2 nu / chi2_{2 nu}), g ~ N(0, I)); the
 * library applies the model's inverse lengthscales (it scales the point, as it does for z).  tau ~ U[0, 2 pi), w and eps standard normal.
 *   NonCentered: u_s - mean(z) = Lk (m + Lq eps_s);    Centered: u_s - mean(z) = (m - mean(z)) + Lq eps_s;    mean(z) = mean_const + muz.
 * Accuracy: the Fourier part approximates the PRIOR, with a covariance error of O(variance / sqrt(L)); the update term k(., z) V is exact,
 * so at the inducing points f_s(z) + jitter V_s = u_s holds to rounding whatever L is, and the samples' moments approach svgp_predict's as
 * L grows.  L = 0 leaves the update term alone (with eps = 0 as well: the posterior mean).
 *   svgp_sampler_create   the model's usual prep (SVGP_NOT_POSDEF as in svgp_elbo), then the M-sized stage in fp64 for BOTH dtypes: Kuu and
 *                         its Cholesky factor are built again in fp64 from the widened z and parameters (an fp32 factor would lose up to
 *                         1e-2 of the sample at cond(Kuu) ~ 5e3), then u, Phi(z) w and V.  It reads the model's device-resident q - what
 *                         svgp_collapsed_q / svgp_natgrad_step left there counts, fetched or not - mean_const and muz
 *                         (svgp_model_set_mean_z).  The sampler is a SNAPSHOT: it owns copies of the scaled z, the kernel parameters,
 *                         mean_const, omega, tau, W and V (V rounded once to the model dtype); a later svgp_model_update or
 *                         svgp_model_free neither changes nor invalidates it.  The basis arrays are host memory, read before the call returns.
 *   svgp_sampler_eval     out[s * ldo + j] = f_s(x_{batch_off + j}), s < S, j < batch_len, in the model dtype; host memory (written before
 *                         the call returns) or device memory of the context's GPU (out_on_device = 1).  One data pass of one kernel: the Kuf
 *                         tiles and the cosine features are generated and multiplied by the resident (L + M) x S panel, nothing n x n and no
 *                         tile is stored, cost linear in batch_len.  pm: the window's prior mean offsets as in svgp_marginals_with_mean, or
 *                         NULL.  The data may have been uploaded without y.  ALWAYS LOCAL, like svgp_predictive.  The value of a point
 *                         does not depend on the window or the call it is evaluated in, bitwise; repeated calls are bitwise equal
 *                         (fixed-order sums, no atomics).
 *   svgp_sampler_state    u and V in fp64 (V before its rounding), M x S column-major each: element (i, s) at [s * M + i]; either may be NULL.
 * SVGP_INVALID_ARG, before anything is enqueued: n_samples < 1, n_features < 0, NULL eps, NULL omega / tau / w with n_features > 0; in
 * svgp_sampler_eval a d or dtype mismatch between sampler and data, a window outside the data, ldo < batch_len, NULL out, or what
 * svgp_marginals_with_mean rejects in pm.  Non-finite inputs give non-finite outputs with SVGP_OK.  No svgp_elbo result changes by a bit.
 * fp32 models: the M-sized stage is fp64, the data pass fp32 (the phase accumulated by the fp32 MFMA; r^2 by differences for d <= 8,
 * by the MFMA expansion beyond): within 5.5e-6 of the fp64 result relative to its largest entry on the test problems (cond(Kuu) <= 4.9e3,
 * max|V| <= 50; profiles/sample/accuracy.md).  Found by symbol (no ABI version step). */
typedef struct svgp_sample_basis {
  int64_t n_features;  /* L >= 0; 0 = the update term alone */
  int64_t n_samples;   /* S >= 1 */
  const void* omega;   /* [L][d] frequencies of the UNIT-lengthscale base kernel, model dtype; the library applies inv_lengthscale */
  const void* tau;     /* [L] phases in [0, 2 pi), model dtype */
  const void* w;       /* [S][L] standard normal feature weights, model dtype */
  const void* eps;     /* [S][M] standard normal draws for q(u), model dtype */
} svgp_sample_basis;   /* 48 bytes */
typedef struct svgp_sampler svgp_sampler;
int32_t svgp_sampler_create(svgp_ctx* ctx, svgp_model* model, const svgp_sample_basis* basis, svgp_sampler** out);
int32_t svgp_sampler_eval(svgp_ctx* ctx, const svgp_sampler* sampler, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                          const svgp_point_mean* pm, void* out, int64_t ldo, int32_t out_on_device);
int32_t svgp_sampler_state(svgp_ctx* ctx, const svgp_sampler* sampler, double* u_out, double* V_out);
int32_t svgp_sampler_free(svgp_ctx* ctx, svgp_sampler* sampler);

/* ---- input gradients of the function samples --------------------------------------------------------------------------------------
 * With xs = invl o x, phase_l = omega_l . xs + tau_l, amp = sqrt(2 variance / L), r_i^2 = |xs - zs_i|^2 and g = variance dkappa / d(r^2):
 *   d f_s / d x_c (x) = invl_c [ - sum_l sin(phase_l) omega_lc amp w_sl + 2 sum_i g(r_i^2) (xs_c - zs_ic) V_is ]
 *   g:  SE -variance e^{-r^2 / 2} / 2;   Matern-3/2 -(3/2) variance e^{-sqrt(3) r};   Matern-5/2 -(5/6) variance (1 + sqrt(5) r) e^{-sqrt(5) r}
 * No division by r: every family is finite at x = z_i, where that term vanishes.  What a maximiser of a sample needs (Thompson sampling);
 * with n_features = 0 and eps = 0 it is the input gradient of the posterior mean.
 *   grad_out[(s * d + c) * ldg + j] = d f_s / d x_c at point batch_off + j, s < S, c < d, j < batch_len, ldg >= batch_len.
 *   out: the values exactly as svgp_sampler_eval writes them (ldo >= batch_len), or NULL: gradient only.
 * The prior mean offsets pm are evaluated by the caller, so their Jacobian is the caller's too: grad_out is the gradient of f_s - mean,
 * to which the caller adds d mean / d x (nothing for the constant mean); pm enters the values alone and is ignored with out = NULL.
 * Both outputs are in the model dtype and in the same kind of memory (out_on_device).  ALWAYS LOCAL.  Works on any svgp_sampler.
 * (a) the values are bitwise svgp_sampler_eval's on the same window; (b) a point's gradient does not depend on the window, the call or
 * whether out was asked for, repeated calls and host / device output are bitwise equal (fixed-order sums, no atomics); (c) no svgp_elbo,
 * svgp_sampler_eval or svgp_sampler_state result changes by a bit.  One data pass per 16 samples and 8 coordinates.
 * SVGP_INVALID_ARG, before anything is enqueued: everything svgp_sampler_eval rejects (a NULL out excepted, and ldo then unread), NULL
 * grad_out, ldg < batch_len.  Non-finite inputs give non-finite outputs with SVGP_OK.  Found by symbol (no ABI version step). */
int32_t svgp_sampler_eval_grad(svgp_ctx* ctx, const svgp_sampler* sampler, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                               const svgp_point_mean* pm, void* out, int64_t ldo, void* grad_out, int64_t ldg, int32_t out_on_device);

/* ---- the exact GP by matrix-free conjugate gradients -------------------------------------------------------------------------------
 * Khat = K(x, x) + diag I over the N points of a data handle, delta = y - mean_const (or the caller's delta):
 *   alpha = Khat^-1 delta,   lml = -1/2 (delta' alpha + log det Khat + N log 2 pi),   the exact GP regression beyond the dense limit.
 * No entry of K is stored: the only O(N^2) work is one kernel that generates K tile by tile on the MFMA and feeds each tile straight
 * into the product with an N x S panel; memory is O(N S).  SE / Matern-3/2 / Matern-5/2 with ARD, d <= SVGP_MAX_D, fp64 and fp32
 * data; vectors are held in the data dtype, every dot product, norm and CG scalar in fp64.  The handle borrows the data handle, which
 * must outlive it.  ALWAYS LOCAL (never collective).  Found by symbol (no ABI version step).
 *   matvec  out = Khat V for an N x S panel (column-major, ldv / ldo >= N, data dtype; on_device: both are device pointers).
 *   solve   X = Khat^-1 B by batched conjugate gradients, any S >= 1, in column blocks of 64 (workspace: five N x 64 arrays).  A
 *           column stops when |r|_2 <= tol |b|_2 (norms in fp64) and its iterates are frozen from then on: A COLUMN'S SOLUTION AND
 *           ITERATION COUNT DO NOT DEPEND, BITWISE, ON WHICH OTHER COLUMNS SHARE THE CALL (an MFMA output column depends on its own
 *           panel column alone; every sum has a fixed order, there are no floating-point atomics), and repeated calls are bitwise
 *           equal.  b = 0 gives x = 0 in 0 iterations.  Running out of maxiter is SVGP_OK with info->converged = 0: iters_out[s],
 *           relres_out[s] (|r| / |b| per column; both nullable) and info report it.  A curvature p' Khat p that is not > 0, NaN
 *           included, is SVGP_NOT_POSDEF and every output is NaN.  The host reads one array of 64 flags per iteration; the CG
 *           coefficients of every column stay on the device until the block is done.
 *   fit     one batched solve of [delta, z_1 .. z_T]: quad = delta' alpha; logdet ~ (1 / T) sum_t |z_t|^2 e_1' log(T_t) e_1 by stochastic
 *           Lanczos quadrature, T_t the Lanczos tridiagonal rebuilt from column t's CG coefficients (svgp_lanczos_logdet, fp64 on the
 *           host).  probes: N x T host doubles, column-major, drawn by the caller (E z z' = I: Rademacher columns; sqrt(N) e_t for
 *           t = 1 .. N makes the estimate exact); the library draws no random numbers.  delta: N host doubles, or NULL for
 *           y - mean_const.  With T = 0 lml and logdet are NaN and quad is valid.  Caches alpha and the parameter set for predict.
 *   lml_grad  fit, and with w_t = Khat^-1 z_t from the same solve  d lml / d theta = 1/2 alpha' dKhat alpha - (1 / 2T) sum_t w_t' dKhat z_t
 *           for theta = variance, inv_lengthscale[d], diag; d_mean_const = sum alpha.  d_diag and d_mean_const may be NULL.
 *   alpha   the N weights of the last fit, data dtype, host.
 *   predict mean = mean_const + k(x*, X) alpha; var = k** - k*' Khat^-1 k* by a batched solve with k(X, x*) as right-hand sides at the
 *           fit's tol and maxiter, which info reports.  mean_out / var_out: n entries of the data dtype, host, each nullable.  With
 *           var_out, n N <= 2^28 elements; beyond it SVGP_UNSUPPORTED and the caller tiles x*.
 * SVGP_INVALID_ARG, before anything is enqueued: a NULL required pointer; descriptor dtype or d different from the data's; an unknown
 * kernel; data without y when delta is NULL; maxiter < 1, tol <= 0, diag < 0, variance <= 0, reserved != 0 (NaN counts as a violation);
 * S < 1; T < 0, or T > 0 with NULL probes; ldv, ldo, ldb or ldx < N; on_device not 0 / 1; alpha or predict before a successful fit;
 * n < 1.  Preconditioning: the next section; pathwise function samples: the one after it; per-point noise variances
 * (Khat = K + diag(sigma^2)): svgp_cg_set_noise below.  Out of scope: a full (non-diagonal) noise covariance, cov / cross-cov,
 * multi-GPU, the Julia hooks. */
typedef struct svgp_cg svgp_cg;
typedef struct svgp_cg_desc {
  int32_t dtype, kernel, d, maxiter; /* maxiter >= 1 */
  double variance;
  const double* inv_lengthscale;     /* [d] */
  double diag;                       /* >= 0 */
  double mean_const;
  double tol;                        /* > 0: a column stops when |r|_2 <= tol |b|_2, norms in fp64 */
  int64_t reserved;                  /* 0 */
} svgp_cg_desc;                      /* 64 bytes */
typedef struct svgp_cg_info {
  int32_t iterations;                /* max over columns */
  int32_t converged;                 /* 1: every column met tol */
  int32_t n_unconverged, reserved;
  double max_rel_residual, quad, logdet, lml; /* quad, logdet, lml: NaN from the calls that do not form them */
  double ms_matvec, ms_vector;       /* device time of the kmv products / of the vector stage, summed over iterations */
} svgp_cg_info;                      /* 64 bytes */
int32_t svgp_cg_create(svgp_ctx* ctx, const svgp_data* data, svgp_cg** out);
int32_t svgp_cg_free(svgp_ctx* ctx, svgp_cg* cg);
int32_t svgp_cg_matvec(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* V, int64_t ldv, void* out, int64_t ldo,
                       int32_t on_device);
int32_t svgp_cg_solve(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* B, int64_t ldb, void* X, int64_t ldx,
                      int32_t on_device, int32_t* iters_out, double* relres_out, svgp_cg_info* info);
int32_t svgp_cg_fit(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                    double* lml_out, svgp_cg_info* info);
int32_t svgp_cg_lml_grad(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                         double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale, double* d_diag,
                         double* d_mean_const);
int32_t svgp_cg_alpha(svgp_ctx* ctx, svgp_cg* cg, void* alpha_out);
int32_t svgp_cg_predict(svgp_ctx* ctx, svgp_cg* cg, int32_t layout, int64_t n, const void* x_host, void* mean_out, void* var_out,
                        svgp_cg_info* info);
/* ---- the Nystrom preconditioner of the conjugate gradients ---------------------------------------------------------------------------
 * With k points z_p set on a handle, Z = K(X, z_p) (N x k), Kuu = K(z_p, z_p) + jitter variance I = Lu Lu' and sigma^2 = desc.diag:
 *   P = Z Kuu^-1 Z' + sigma^2 I,   P^-1 r = (r - Z W Z' r) / sigma^2,   W = Lu^-T B^-1 Lu^-1 / sigma^2,   B = I + Lu^-1 (Z'Z) Lu^-T / sigma^2,
 *   log det P = N log sigma^2 + log det B.
 * Nothing N x k is stored: Z' r is a row-split form of the kmv kernel (few points, a long reduction: the grid is point workgroups x row
 * segments, each segment's partial sums are written in the data dtype and added in ascending order in fp64; the number of segments
 * depends on N and k alone, so a column's value does not depend on its neighbours and repeated calls are bitwise equal), and Z c is the
 * kmv kernel itself with the k points as its rows, whose epilogue adds r / sigma^2.  The k-sized stage (Kuu, Lu, the Gram Z'Z, B and its
 * factor, W) runs on the device in fp64 for both data dtypes, the Gram accumulated in fp64 from fp64 entries (accumulated in float32, B
 * is not positive definite); it is set up once per call from the call's parameter set, and its device time is added to
 * info->ms_vector, as is the time of every application (two kernel products with N k generated entries each per iteration).
 *   set_preconditioner  k points in `layout` (as svgp_cg_predict's x_host, data dtype, host), 1 <= k <= 2048, jitter >= 0 (times the
 *           variance; 1e-4 is the documented default: very small values lose accuracy with an ill-conditioned Kuu even in fp64).  k = 0
 *           removes the preconditioner: every call is then bitwise what it is on a handle that never had one.  Replaces earlier points.
 *   precond_cross  out (k x S, ldo >= k) = K(z_p, X) V for an N x S panel (ldv >= N): the row-split kernel alone.
 *   precond_apply  out (N x S) = P^-1 R, and log det P (nullable).  out must not be R.
 *   With a preconditioner set, svgp_cg_solve, svgp_cg_predict's variance solve and the T = 0 forms of svgp_cg_fit / svgp_cg_lml_grad run
 *   the preconditioned recurrence z = P^-1 r, rho = r'z, a = rho / p'Khat p, beta = rho_new / rho, p = z + beta p; the stopping test stays
 *   |r|_2 <= tol |b|_2 on the true residual, columns freeze as before, and the column-independence guarantee holds.
 *   fit_precond / lml_grad_precond  svgp_cg_fit / svgp_cg_lml_grad plus probes_k (k x T host doubles, column-major).  The probes need
 *           E z z' = P: from the caller's eps (N x T, `probes`) and xi (k x T), both with identity covariance, the library forms
 *           z_t = sigma eps_t + Z Lu^-T xi_t on the device.  log det Khat = log det P + (1 / T) sum_t (z_t' P^-1 z_t) e_1' log(T_t) e_1, T_t the
 *           Lanczos tridiagonal of P^-1/2 Khat P^-1/2 rebuilt from column t's coefficients; d lml / d theta = 1/2 alpha' dKhat alpha -
 *           (1 / 2T) sum_t w_t' dKhat (P^-1 z_t).  With T = N + k, eps = sqrt(T) [I_N 0] and xi = sqrt(T) [0 I_k] the estimate is exact.
 * SVGP_INVALID_ARG, before anything is enqueued: k outside [0, 2048]; NULL points with k > 0; a bad layout; jitter < 0 or NaN;
 * precond_cross / precond_apply / fit_precond / lml_grad_precond without a preconditioner; NULL probes_k with T > 0; svgp_cg_fit /
 * svgp_cg_lml_grad with T > 0 while a preconditioner is set (the probes need xi); desc.diag == 0 in any call that applies the
 * preconditioner.  SVGP_NOT_POSDEF: Kuu + jitter or B fails to factor, or, in a solve, a product r' P^-1 r of an active column is not
 * > 0 (the applied P^-1 has lost positive definiteness to rounding; handled like a curvature that is not > 0); the outputs are NaN and
 * the context stays healthy.  Memory: 13 fp64 arrays of ceil128(k)^2 and one of N x 64; an fp32 handle also keeps fp64 copies of x (widened
 * once per handle), of its prepared rows and of z_p for the Gram, about three times the bytes of its x.  Found by symbol
 * (no ABI version step). */
int32_t svgp_cg_set_preconditioner(svgp_ctx* ctx, svgp_cg* cg, int32_t layout, int64_t k, const void* z_host, double jitter);
int32_t svgp_cg_precond_cross(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* V, int64_t ldv, void* out, int64_t ldo,
                              int32_t on_device);
int32_t svgp_cg_precond_apply(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, int64_t S, const void* R, int64_t ldr, void* out, int64_t ldo,
                              int32_t on_device, double* logdet_p_out);
int32_t svgp_cg_fit_precond(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                            const double* probes_k, double* lml_out, svgp_cg_info* info);
int32_t svgp_cg_lml_grad_precond(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                                 const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                                 double* d_diag, double* d_mean_const);
/* ---- the gradient of the exact GP's log marginal likelihood with respect to the data inputs --------------------------------------------
 * svgp_cg_lml_grad / svgp_cg_lml_grad_precond, and from the same solve, with p_t = z_t (no preconditioner) or P^-1 z_t, g = d kappa / d(r^2)
 * as in svgp_sampler_eval_grad and il = inv_lengthscale:
 *   x_bar[c, i] = d lml / d x_ic = il_c^2 sum_j 2 g(r_ij^2) (x_ic - x_jc) [ alpha_i alpha_j - (1 / 2T) sum_t (w_it p_jt + w_jt p_it) ]
 * the same trace estimator as the other gradient blocks (unbiased for the exact gradient, exact with unit probes; it is NOT the derivative
 * of the stochastic Lanczos value).  What a learned feature map in front of the kernel (deep kernel learning), input warping or latent
 * inputs need.  With a preconditioner whose points are a subset of the data, the dependence of P on x is ignored: P changes the
 * estimator's variance, not its expectation.  Two identities hold term by term, for any probes: sum_i x_bar[c, i] = 0 (translation) and
 * sum_i x_ic x_bar[c, i] = il_c d_inv_lengthscale[c] (scaling).
 *   gx: svgp_input_grad as in svgp_elbo_grad_inputs over the handle's N points: feature-major gx->x[c * ld + i], ld >= N, host or device
 *       (on_device), data dtype, reserved == 0.
 *   probes_k: NULL exactly when no preconditioner is set on the handle; with one, as in svgp_cg_lml_grad_precond.
 * One data-sized kernel family: with the left panel [alpha, w_t .., p_t ..] and the right panel [alpha, -p_t / 2T .., -w_t / 2T ..] of
 * 2T + 1 columns, every 16 x 16 tile of K(X, X) is generated once per (16 columns, coordinate block) on the MFMA, multiplied into the
 * right panel per coordinate (the coordinate difference per entry, before the product; no division by r; fp32 with d <= 8 by
 * differences), and the accumulators are contracted with the left panel in registers: nothing of size S x d x N is written.  Memory:
 * two N x (2T + 1) panels and ceil((2T + 1) / 16) d N doubles.  ceil((2T + 1) / 16) ceil(d / 8) passes over K (coordinate blocks of 4
 * for fp64 with d > 32).  The diagonal entry has r^2 = 0 exactly and contributes exactly nothing; duplicated points are finite.
 * (a) every other output is bitwise what svgp_cg_lml_grad / svgp_cg_lml_grad_precond returns on the same handle and inputs, and those
 * calls are unchanged by a bit; (b) no atomics, every sum has a fixed order: repeated calls are bitwise equal, and x_bar does not depend
 * on on_device.  T = 0: x_bar is NaN, like the other trace blocks.  SVGP_NOT_POSDEF: x_bar is NaN and the context stays healthy.
 * SVGP_INVALID_ARG, before anything is enqueued: what svgp_cg_lml_grad(_precond) rejects; NULL gx or gx->x; gx->ld < N; on_device not
 * 0 / 1 or reserved != 0; a device gx->x overlapping the data's x; probes_k without a preconditioner.  Found by symbol (no ABI version
 * step). */
int32_t svgp_cg_lml_grad_inputs(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                                const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                                double* d_diag, double* d_mean_const, const svgp_input_grad* gx);
/* ---- per-point noise variances of the exact GP by conjugate gradients ------------------------------------------------------------------
 * The collapsed bound's convention (svgp_point_noise): the per-point term adds to the descriptor's variance,
 *   sigma_i^2 = T(desc.diag) + s_i   in the data dtype T with one rounding,      Khat = K(x, x) + diag(sigma^2)
 * in every call on the handle once a vector is set: svgp_cg_matvec, _solve, _fit(_precond), _lml_grad(_precond / _inputs), _predict (the
 * latent variance), _precond_apply and svgp_cg_sampler_create (right-hand sides delta - Phi(X) w_s - sigma_i eps_si; the sampler stays a
 * snapshot).  svgp_cg_precond_cross is the kernel product alone and does not change.  Known measurement errors, a fixed-noise model or
 * a learned noise function (GPyTorch's FixedNoiseGaussianLikelihood, AbstractGPs' Diagonal Sigma_y).
 *   set_noise  N values of the data dtype, host or device memory (pn->on_device), copied into the handle: a snapshot, handle state like
 *           the preconditioner's points.  pn = NULL removes the vector: every call is then bitwise what it is on a handle that never
 *           had one.  Clears the cached fit: svgp_cg_alpha and svgp_cg_predict need a new one.  One NaN-propagating min-reduction of s
 *           runs on the device at set time and its result is kept on the host: a later call fails BEFORE its data pass with
 *           SVGP_NOT_POSDEF when T(desc.diag) + min s is < 0, or <= 0 with a preconditioner set, or NaN; its outputs are NaN and the
 *           context stays healthy.
 *   The kmv kernel's epilogue reads sigma_i^2 once per output point in place of the scalar.  The preconditioner becomes
 *           P = Z Kuu^-1 Z' + D, D = diag(sigma^2):  P^-1 r = D^-1 r - D^-1 Z W Z' D^-1 r,  W = Lu^-T B^-1 Lu^-1,
 *           B = I + Lu^-1 (Z' D^-1 Z) Lu^-T,  log det P = sum_i log sigma_i^2 + log det B (the sum a fixed two-stage fp64 reduction), the
 *           Gram's weights applied in fp64 to the explicit N x <= 64 block of Z; the two scalings by D^-1 of an application are
 *           streaming passes around the two kernel products.  The probes are z_t = D^1/2 eps_t + Z Lu^-T xi_t.
 *   lml_grad_noise  the superset gradient call: svgp_cg_lml_grad_inputs' arguments with gx nullable, and
 *           s_bar_i = d lml / d sigma_i^2 = 1/2 alpha_i^2 - (1 / 2T) sum_t w_it p_it     (p_t = z_t, or P^-1 z_t with a preconditioner)
 *           the trace estimator of every other block: t ascending in fp64, rounded once to the data dtype; N values, host or device
 *           (gpn->on_device).  Works with or without a vector set.  d_diag keeps its meaning, the derivative with respect to the
 *           common term, = sum_i s_bar_i.  With a vector set d_variance = [1/2 alpha' Khat alpha - (1 / 2T) sum_t w_t' Khat p_t -
 *           sum_i sigma_i^2 s_bar_i] / variance (a fixed two-stage fp64 reduction).  Every other output is bitwise what
 *           svgp_cg_lml_grad(_precond / _inputs) returns on the same handle and inputs.  No atomics, every sum has a fixed order:
 *           repeated calls and host / device output are bitwise equal.  T = 0: s_bar is NaN, like the other trace blocks;
 *           SVGP_NOT_POSDEF: s_bar is NaN.
 * SVGP_INVALID_ARG, before anything is enqueued: NULL pn->s, gpn or gpn->s_bar; on_device not 0 / 1; reserved != 0; a handle on another
 * device than the context; what svgp_cg_lml_grad_inputs rejects (a NULL gx excepted).  With a vector set desc.diag == 0 is allowed with
 * a preconditioner (the variances are diag + s_i).  Memory: six N-vectors on the handle (s, sigma^2, 1 / sigma^2, sqrt(sigma^2)
 * and s_bar in the data dtype, 1 / sigma^2 in fp64).  Found by symbol (no ABI version step). */
int32_t svgp_cg_set_noise(svgp_ctx* ctx, svgp_cg* cg, const svgp_point_noise* pn);
int32_t svgp_cg_lml_grad_noise(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, int32_t T, const double* probes,
                               const double* probes_k, double* lml_out, svgp_cg_info* info, double* d_variance, double* d_inv_lengthscale,
                               double* d_diag, double* d_mean_const, const svgp_input_grad* gx, svgp_point_noise_grad* gpn);
/* ---- pathwise function samples of the exact GP ---------------------------------------------------------------------------------------
 * S draws from the exact posterior by pathwise conditioning (Wilson et al. 2020, 2021) with the CG solve, each one a FUNCTION that can be
 * evaluated at any points, any number of times.  With Khat = K(X, X) + sigma^2 I (sigma^2 = desc.diag), delta = y - mean(X), phi_l as in
 * svgp_sampler_* and eps_s ~ N(0, I_N):
 *   f_s(x) = mean_const + sum_l phi_l(x) w_sl + sum_j k(x, X_j) V_js,      V_s = Khat^-1 (delta - Phi(X) w_s - sigma eps_s)
 *   d f_s / d x_c = invl_c [ - sum_l sin(phase_l) omega_lc amp w_sl + 2 sum_j g(r_j^2) (xs_c - Xs_jc) V_js ]     (g as in svgp_sampler_eval_grad)
 * With n_features = 0 and eps = 0, V_s = alpha and f_s is the posterior mean.  The Fourier part approximates the PRIOR; the update term is
 * exact: f_s(X) + sigma eps_s + sigma^2 V_s = y to the solve's tolerance whatever L is.  The library draws nothing: the caller supplies
 * every random number in a svgp_sample_basis whose eps is [S][N] in the data dtype (omega, tau, w as there, data dtype).
 *   create  forms the S right-hand sides on the device (Phi(X) w through the evaluation kernel over the features alone, then one affine
 *           pass in fp64 rounded once) and runs ONE batched solve over the S columns, preconditioned when the handle has a preconditioner;
 *           info reports it as in svgp_cg_solve (nullable).  Running out of maxiter is SVGP_OK with info->converged = 0.
 *           SVGP_NOT_POSDEF as there: no sampler is made.  delta: N host doubles, or NULL for y - mean_const.  The sampler is a SNAPSHOT:
 *           it owns the prepared rows of X and their bias, the parameters, omega, tau, amp W and V in the data dtype, O(N (d + S)) memory;
 *           later calls on the CG handle, or freeing it or the data handle, change nothing.  It needs no preceding svgp_cg_fit and leaves
 *           the handle's cached fit as it was.  The basis arrays are host memory, read before the call returns.
 *   eval    out[s * ldo + j] = f_s(x_{batch_off + j}), s < S, j < batch_len, data dtype; host memory, or device memory of the context's
 *           GPU (out_on_device = 1).  A non-constant prior mean's offsets are the caller's to add.
 *   eval_grad  grad_out[(s * d + c) * ldg + j] = d f_s / d x_c at point batch_off + j; out: the values, bitwise svgp_cg_sampler_eval's, or
 *           NULL.  Both outputs live in the same kind of memory.
 *   state   V (N x S column-major, data dtype, exactly as evaluated), the per-column iteration counts and relative residuals of the
 *           solve; each output nullable.
 * One data-sized kernel family: the feature and kernel tiles are generated on the MFMA and multiplied by amp W and by the N x S panel V
 * read from global memory; nothing n* x N is stored.  The grid is (point workgroups) x (row segments): every segment's partial sums are
 * written in the data dtype and added in ascending segment order in fp64, no atomics.  THE SEGMENTATION IS A FUNCTION OF N ALONE, so,
 * bitwise: a point's value and gradient do not depend on the window, the call, the other points or the other columns (column s of an
 * S-sample sampler is the 1-sample sampler of the same draws); host and device output agree; repeated calls agree; eval_grad's values
 * are eval's.  Points are processed in rounds (at most 4096 points), which bounds the partial buffer; that buffer belongs to the CONTEXT, the
 * evaluations only read the sampler, so one sampler may serve several contexts of its device (one thread per context, as everywhere).
 * ALWAYS LOCAL.
 * SVGP_INVALID_ARG, before anything is enqueued: everything svgp_cg_solve rejects in the descriptor; n_samples < 1, n_features < 0,
 * NULL eps, NULL omega / tau / w with n_features > 0; data without y when delta is NULL; desc.diag == 0 with a preconditioner set; in
 * the evaluations a d or dtype mismatch between sampler and data, a window outside the data, ldo (with out) or ldg < batch_len, NULL
 * out (eval) or grad_out.  Non-finite inputs give non-finite outputs with SVGP_OK (a right-hand side whose norm is not finite is not
 * solved: V is NaN, info->converged = 0), and the context stays healthy.  No other entry point's result changes by a bit.  Found by
 * symbol (no ABI version step). */
typedef struct svgp_cg_sampler svgp_cg_sampler;
int32_t svgp_cg_sampler_create(svgp_ctx* ctx, svgp_cg* cg, const svgp_cg_desc* desc, const double* delta, const svgp_sample_basis* basis,
                               svgp_cg_sampler** out, svgp_cg_info* info);
int32_t svgp_cg_sampler_eval(svgp_ctx* ctx, const svgp_cg_sampler* sampler, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                             void* out, int64_t ldo, int32_t out_on_device);
int32_t svgp_cg_sampler_eval_grad(svgp_ctx* ctx, const svgp_cg_sampler* sampler, const svgp_data* data, int64_t batch_off, int64_t batch_len,
                                  void* out, int64_t ldo, void* grad_out, int64_t ldg, int32_t out_on_device);
int32_t svgp_cg_sampler_state(svgp_ctx* ctx, const svgp_cg_sampler* sampler, void* V_out, int32_t* iters_out, double* relres_out);
int32_t svgp_cg_sampler_free(svgp_ctx* ctx, svgp_cg_sampler* sampler);
/* host only: the row segmentation and the round of the evaluations for N data rows - segments of seg_rows rows (512; more beyond 1024
 * segments), round_points points per set of launches (about 2^20 / n_segments, a multiple of 256 in [256, 4096]; the gradient form
 * takes a quarter of it, at least 256).  SVGP_INVALID_ARG: N < 0 or a NULL pointer. */
int32_t svgp_cg_sampler_plan(int64_t N, int64_t* seg_rows, int32_t* n_segments, int64_t* round_points);
/* host only, like svgp_gausshermite: out = e_1' log(T) e_1 for the Lanczos tridiagonal of `iters` CG steps with step lengths a[j] and
 * residual ratios b[j] = |r_{j+1}|^2 / |r_j|^2 (diagonal 1 / a_j + b_{j-1} / a_{j-1}, off-diagonal sqrt(b_j) / a_j; b[iters - 1] is not
 * read), by an implicit-shift QL iteration in fp64.  SVGP_INVALID_ARG: NULL pointers, iters < 1; SVGP_NOT_POSDEF (out = NaN): an
 * eigenvalue that is not > 0. */
int32_t svgp_lanczos_logdet(const double* a, const double* b, int32_t iters, double* out);

#ifdef __cplusplus
}
#endif
#endif /* SVGP_MI355X_H */
