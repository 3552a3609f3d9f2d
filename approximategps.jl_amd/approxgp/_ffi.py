"""ctypes binding of libsvgp_mi355x.so (include/svgp_mi355x.h) — the same symbols the Julia shim
`ccall`s.  There is no CPU fallback: a missing library or a missing GPU raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVGP_MI355X_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libsvgp_mi355x.so")

OK, INVALID_ARG, NOT_POSDEF, NEG_VARIANCE, UNSUPPORTED, HIP_ERROR, RCCL_ERROR, OOM = range(8)
F64, F32 = 0, 1
COLVECS, ROWVECS, VEC = 0, 1, 2
KERNEL_SE, KERNEL_MATERN32, KERNEL_MATERN52 = 0, 1, 2
LIK_GAUSSIAN, LIK_BERNOULLI_LOGISTIC, LIK_POISSON_EXP, LIK_EXPONENTIAL_EXP, LIK_GAMMA_EXP, LIK_BERNOULLI_NORMCDF = 0, 1, 2, 3, 4, 5
NONCENTERED, CENTERED = 0, 1
NEGVAR_ERROR, NEGVAR_CLAMP = 0, 1


class ModelDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int32), ("kernel", C.c_int32), ("parametrization", C.c_int32), ("likelihood", C.c_int32),
        ("quadrature_n", C.c_int32), ("layout_z", C.c_int32), ("neg_var_policy", C.c_int32), ("d", C.c_int32),
        ("M", C.c_int64), ("variance", C.c_double), ("inv_lengthscale", C.POINTER(C.c_double)),
        ("mean_const", C.c_double), ("jitter", C.c_double), ("lik_sigma2", C.c_double),
        ("z", C.c_void_p), ("m", C.c_void_p), ("Lq", C.c_void_p),
    ]


class Terms(C.Structure):
    _fields_ = [
        ("elbo", C.c_double), ("expectation", C.c_double), ("kl", C.c_double), ("scale", C.c_double),
        ("logdet_kuu", C.c_double), ("n_points", C.c_int64), ("n_neg_var", C.c_int64),
        ("chol_info", C.c_int32), ("reserved", C.c_int32),
    ]


class Grads(C.Structure):
    _fields_ = [("variance", C.c_double), ("lik_sigma2", C.c_double), ("mean_const", C.c_double),
                ("inv_lengthscale", C.POINTER(C.c_double)), ("z", C.c_void_p), ("m", C.c_void_p), ("Lq", C.c_void_p)]


class InputGrad(C.Structure):
    """svgp_input_grad: where d elbo / d x goes (element (f, j) at x[f * ld + j]; on_device 0: host, 1: device)."""
    _fields_ = [("x", C.c_void_p), ("ld", C.c_int64), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class PointMean(C.Structure):
    """svgp_point_mean: the batch's prior mean offsets mux (data dtype; on_device 0: host, 1: device)."""
    _fields_ = [("mu", C.c_void_p), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class PointMeanGrad(C.Structure):
    """svgp_point_mean_grad: where d elbo / d mux goes (data dtype; on_device 0: host, 1: device)."""
    _fields_ = [("mu_bar", C.c_void_p), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class PointNoise(C.Structure):
    """svgp_point_noise: the batch's per-point noise variances s, added to lik_sigma2 (data dtype; on_device 0: host, 1: device)."""
    _fields_ = [("s", C.c_void_p), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class PointNoiseGrad(C.Structure):
    """svgp_point_noise_grad: where d bound / d sigma_j^2 goes (data dtype; on_device 0: host, 1: device)."""
    _fields_ = [("s_bar", C.c_void_p), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class Timing(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_prep", C.c_double), ("ms_strip", C.c_double), ("ms_expect", C.c_double),
                ("ms_kuf", C.c_double),
                ("strip_launches", C.c_int64),
                # appended since ABI v3 (read through svgp_last_timing_sized): v4 ms_chol, v5 ms_overlap
                ("ms_chol", C.c_double), ("ms_overlap", C.c_double)]


class LaplaceDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("kernel", C.c_int32), ("likelihood", C.c_int32), ("d", C.c_int32),
                ("maxiter", C.c_int32), ("warm_start", C.c_int32), ("variance", C.c_double),
                ("inv_lengthscale", C.POINTER(C.c_double)), ("jitter", C.c_double), ("lik_sigma2", C.c_double),
                ("reserved", C.c_int64)]


class LaplaceInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("chol_info", C.c_int32), ("reserved", C.c_int32),
                ("lml", C.c_double), ("ms_point", C.c_double), ("ms_chol", C.c_double), ("ms_linv", C.c_double),
                ("ms_gemv", C.c_double)]


class NNDesc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("kernel", C.c_int32), ("d", C.c_int32), ("k", C.c_int32), ("variance", C.c_double),
                ("inv_lengthscale", C.POINTER(C.c_double)), ("diag", C.c_double), ("mean_const", C.c_double),
                ("reserved", C.c_int64)]


class NNInfo(C.Structure):
    _fields_ = [("first_bad", C.c_int64), ("n_neg_f", C.c_int64), ("lml", C.c_double)]


class CollapsedTerms(C.Structure):
    """svgp_collapsed_terms: the collapsed (Titsias) bound and its parts."""
    _fields_ = [("bound", C.c_double), ("fit", C.c_double), ("trace", C.c_double), ("logdet_B", C.c_double),
                ("logdet_kuu", C.c_double), ("n_points", C.c_int64), ("chol_info", C.c_int32), ("chol_info_b", C.c_int32),
                ("reserved", C.c_int64)]


class PredSummary(C.Structure):
    """svgp_pred_summary: the sums of svgp_predictive / svgp_lik_predictive over the points that counted."""
    _fields_ = [("sum_lpd", C.c_double), ("sum_sq_err", C.c_double), ("n_points", C.c_int64), ("n_neg_var", C.c_int64)]


class SampleBasis(C.Structure):
    """svgp_sample_basis: the random numbers of S pathwise function samples, all supplied by the caller (host arrays, model dtype):
    omega [L][d] unit-lengthscale frequencies, tau [L] phases, w [S][L] feature weights, eps [S][M] draws for q(u)."""
    _fields_ = [("n_features", C.c_int64), ("n_samples", C.c_int64), ("omega", C.c_void_p), ("tau", C.c_void_p),
                ("w", C.c_void_p), ("eps", C.c_void_p)]


class CGDesc(C.Structure):
    """svgp_cg_desc: one parameter set of the exact GP by conjugate gradients (64 bytes)."""
    _fields_ = [("dtype", C.c_int32), ("kernel", C.c_int32), ("d", C.c_int32), ("maxiter", C.c_int32), ("variance", C.c_double),
                ("inv_lengthscale", C.POINTER(C.c_double)), ("diag", C.c_double), ("mean_const", C.c_double), ("tol", C.c_double),
                ("reserved", C.c_int64)]


class CGInfo(C.Structure):
    """svgp_cg_info: what a batched solve did (64 bytes)."""
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("n_unconverged", C.c_int32), ("reserved", C.c_int32),
                ("max_rel_residual", C.c_double), ("quad", C.c_double), ("logdet", C.c_double), ("lml", C.c_double),
                ("ms_matvec", C.c_double), ("ms_vector", C.c_double)]


# every symbol include/svgp_mi355x.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "svgp_version": (C.c_int32, []),
    "svgp_device_count": (C.c_int32, []),
    "svgp_ctx_create": (C.c_int32, [C.c_int32, _P, C.POINTER(_P)]),
    "svgp_ctx_destroy": (C.c_int32, [_P]),
    "svgp_last_error": (C.c_char_p, [_P]),
    "svgp_last_timing": (C.c_int32, [_P, C.POINTER(Timing)]),
    "svgp_last_timing_sized": (C.c_int32, [_P, _P, C.c_int64]),
    "svgp_data_upload": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _P, _P, C.POINTER(_P)]),
    "svgp_data_wrap_device": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _P, _P, C.POINTER(_P)]),
    "svgp_data_free": (C.c_int32, [_P, _P]),
    "svgp_model_create": (C.c_int32, [_P, C.POINTER(ModelDesc), C.POINTER(_P)]),
    "svgp_model_update": (C.c_int32, [_P, _P, C.POINTER(ModelDesc)]),
    "svgp_model_free": (C.c_int32, [_P, _P]),
    "svgp_elbo": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.POINTER(C.c_double), C.POINTER(Terms)]),
    "svgp_elbo_partial": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(C.c_double)]),
    "svgp_elbo_grad": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.POINTER(C.c_double), C.POINTER(Terms),
                                   C.POINTER(Grads)]),
    "svgp_elbo_grad_shard": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_double),
                                         C.POINTER(Terms), C.POINTER(Grads)]),
    "svgp_marginals": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    "svgp_elbo_grad_ext": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, _P, _P, C.POINTER(C.c_double),
                                       C.POINTER(Terms), C.POINTER(Grads)]),
    "svgp_elbo_grad_inputs": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.POINTER(C.c_double), C.POINTER(Terms),
                                          C.POINTER(Grads), C.POINTER(InputGrad)]),
    "svgp_elbo_grad_ext_inputs": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, _P, _P,
                                              C.POINTER(C.c_double), C.POINTER(Terms), C.POINTER(Grads), C.POINTER(InputGrad)]),
    "svgp_model_set_mean_z": (C.c_int32, [_P, _P, _P]),
    "svgp_elbo_with_mean": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.POINTER(PointMean), C.POINTER(C.c_double),
                                        C.POINTER(Terms)]),
    "svgp_marginals_with_mean": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(PointMean), _P, _P]),
    "svgp_elbo_grad_with_mean": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.POINTER(PointMean), C.c_double, _P, _P,
                                             C.POINTER(C.c_double), C.POINTER(Terms), C.POINTER(Grads), C.POINTER(InputGrad),
                                             C.POINTER(PointMeanGrad)]),
    "svgp_prior_kl": (C.c_int32, [_P, _P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svgp_elbo_host": (C.c_int32, [_P, C.POINTER(ModelDesc), C.c_int32, C.c_int64, _P, _P, C.c_double,
                                   C.POINTER(C.c_double), C.POINTER(Terms)]),
    "svgp_posterior": (C.c_int32, [_P, _P, _P, _P, _P]),
    "svgp_predict": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P, _P]),
    "svgp_predict_cross_cov": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, C.c_int64, _P, _P]),
    "svgp_kuf": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, _P]),
    "svgp_gausshermite": (C.c_int32, [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svgp_offload_advice": (C.c_int32, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "svgp_offload_work": (C.c_double, [C.c_int64, C.c_int64, C.c_int32]),
    # the Laplace approximation
    "svgp_laplace_create": (C.c_int32, [_P, _P, C.POINTER(_P)]),
    "svgp_laplace_fit": (C.c_int32, [_P, _P, C.POINTER(LaplaceDesc), _P, C.POINTER(C.c_double), C.POINTER(LaplaceInfo)]),
    "svgp_laplace_lml_grad": (C.c_int32, [_P, _P, C.POINTER(LaplaceDesc), _P, C.POINTER(C.c_double), C.POINTER(LaplaceInfo),
                                          C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svgp_laplace_mode": (C.c_int32, [_P, _P, _P, _P, _P]),
    "svgp_laplace_predict": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P, _P]),
    "svgp_laplace_predict_cross_cov": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, C.c_int64, _P, _P]),
    "svgp_laplace_free": (C.c_int32, [_P, _P]),
    # the NearestNeighbors (Vecchia) approximation
    "svgp_nn_create": (C.c_int32, [_P, _P, C.POINTER(_P)]),
    "svgp_nn_lml": (C.c_int32, [_P, _P, C.POINTER(NNDesc), C.POINTER(C.c_double), C.POINTER(NNInfo)]),
    "svgp_nn_lml_grad": (C.c_int32, [_P, _P, C.POINTER(NNDesc), C.POINTER(C.c_double), C.POINTER(NNInfo), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svgp_nn_fit": (C.c_int32, [_P, _P, C.POINTER(NNDesc), C.POINTER(C.c_double), C.POINTER(NNInfo)]),
    "svgp_nn_factors": (C.c_int32, [_P, _P, _P, _P, _P]),
    "svgp_nn_predict": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P, _P]),
    "svgp_nn_predict_cross_cov": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, C.c_int64, _P, _P]),
    "svgp_nn_free": (C.c_int32, [_P, _P]),
    "svgp_nn_set_neighbors": (C.c_int32, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    "svgp_nn_build_neighbors": (C.c_int32, [_P, _P, C.c_int32, C.POINTER(C.c_double)]),
    "svgp_nn_get_neighbors": (C.c_int32, [_P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "svgp_nn_clear_neighbors": (C.c_int32, [_P, _P]),
    "svgp_nn_predict_local": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, C.c_int32, _P, _P, C.POINTER(C.c_int32)]),
    "svgp_nn_set_noise": (C.c_int32, [_P, _P, C.POINTER(PointNoise)]),
    "svgp_nn_set_mean": (C.c_int32, [_P, _P, C.POINTER(PointMean)]),
    "svgp_nn_lml_grad_points": (C.c_int32, [_P, _P, C.POINTER(NNDesc), C.POINTER(C.c_double), C.POINTER(NNInfo), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(PointMeanGrad), C.POINTER(PointNoiseGrad)]),
    # the collapsed bound and the optimal q
    "svgp_collapsed_bound": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.POINTER(CollapsedTerms)]),
    "svgp_collapsed_q": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, _P, _P, C.POINTER(C.c_double)]),
    "svgp_collapsed_grad": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.POINTER(CollapsedTerms),
                                        C.POINTER(Grads), C.POINTER(InputGrad)]),
    "svgp_collapsed_bound_with_noise": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(PointMean), C.POINTER(PointNoise),
                                                    C.POINTER(C.c_double), C.POINTER(CollapsedTerms)]),
    "svgp_collapsed_q_with_noise": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(PointMean), C.POINTER(PointNoise), _P, _P,
                                                C.POINTER(C.c_double)]),
    "svgp_collapsed_grad_with_noise": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(PointMean), C.POINTER(PointNoise),
                                                   C.POINTER(C.c_double), C.POINTER(CollapsedTerms), C.POINTER(Grads),
                                                   C.POINTER(InputGrad), C.POINTER(PointMeanGrad), C.POINTER(PointNoiseGrad)]),
    # natural-gradient steps on q
    "svgp_natgrad_step": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(Terms),
                                      C.POINTER(Grads), _P, _P]),
    "svgp_natgrad_step_ext": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, _P, _P,
                                          C.POINTER(C.c_double), C.POINTER(Terms), C.POINTER(Grads), _P, _P]),
    "svgp_model_update_keep_q": (C.c_int32, [_P, _P, C.POINTER(ModelDesc)]),
    # the predictive distribution of the observation
    "svgp_predictive": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(PointMean), C.POINTER(PredSummary), _P, _P, _P]),
    "svgp_lik_predictive": (C.c_int32, [_P, C.c_int32, C.c_double, C.c_int32, C.c_int64, _P, _P, _P, C.POINTER(PredSummary), _P, _P, _P]),
    # pathwise posterior function samples
    "svgp_sampler_create": (C.c_int32, [_P, _P, C.POINTER(SampleBasis), C.POINTER(_P)]),
    "svgp_sampler_eval": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(PointMean), _P, C.c_int64, C.c_int32]),
    "svgp_sampler_eval_grad": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, C.POINTER(PointMean), _P, C.c_int64, _P, C.c_int64, C.c_int32]),
    "svgp_sampler_state": (C.c_int32, [_P, _P, _P, _P]),
    "svgp_sampler_free": (C.c_int32, [_P, _P]),
    # the exact GP by matrix-free conjugate gradients
    "svgp_cg_create": (C.c_int32, [_P, _P, C.POINTER(_P)]),
    "svgp_cg_free": (C.c_int32, [_P, _P]),
    "svgp_cg_matvec": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32]),
    "svgp_cg_solve": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.POINTER(C.c_int32),
                                  C.POINTER(C.c_double), C.POINTER(CGInfo)]),
    "svgp_cg_fit": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                C.POINTER(C.c_double), C.POINTER(CGInfo)]),
    "svgp_cg_lml_grad": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(CGInfo), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svgp_cg_alpha": (C.c_int32, [_P, _P, _P]),
    "svgp_cg_predict": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P, C.POINTER(CGInfo)]),
    "svgp_cg_set_preconditioner": (C.c_int32, [_P, _P, C.c_int32, C.c_int64, _P, C.c_double]),
    "svgp_cg_precond_cross": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32]),
    "svgp_cg_precond_apply": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32,
                                          C.POINTER(C.c_double)]),
    "svgp_cg_fit_precond": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(CGInfo)]),
    "svgp_cg_lml_grad_precond": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(CGInfo), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svgp_cg_lml_grad_inputs": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(CGInfo), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(InputGrad)]),
    "svgp_cg_set_noise": (C.c_int32, [_P, _P, C.POINTER(PointNoise)]),
    "svgp_cg_lml_grad_noise": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(CGInfo), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(InputGrad),
                                           C.POINTER(PointNoiseGrad)]),
    "svgp_cg_sampler_create": (C.c_int32, [_P, _P, C.POINTER(CGDesc), C.POINTER(C.c_double), C.POINTER(SampleBasis), C.POINTER(_P),
                                           C.POINTER(CGInfo)]),
    "svgp_cg_sampler_eval": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int32]),
    "svgp_cg_sampler_eval_grad": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32]),
    "svgp_cg_sampler_state": (C.c_int32, [_P, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "svgp_cg_sampler_free": (C.c_int32, [_P, _P]),
    "svgp_cg_sampler_plan": (C.c_int32, [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "svgp_lanczos_logdet": (C.c_int32, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double)]),
    # multi-GPU
    "svgp_comm_unique_id": (C.c_int32, [_P]),
    "svgp_ctx_attach_comm": (C.c_int32, [_P, _P, C.c_int32, C.c_int32]),
    "svgp_ctx_detach_comm": (C.c_int32, [_P]),
    "svgp_ctx_comm_info": (C.c_int32, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "svgp_group_create": (C.c_int32, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(_P)]),
    "svgp_group_destroy": (C.c_int32, [_P]),
    "svgp_group_size": (C.c_int32, [_P]),
    "svgp_group_ctx": (_P, [_P, C.c_int32]),
    "svgp_group_last_error": (C.c_char_p, [_P]),
    "svgp_group_data_upload": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _P, _P, C.POINTER(_P)]),
    "svgp_group_model_create": (C.c_int32, [_P, C.POINTER(ModelDesc), C.POINTER(_P)]),
    "svgp_group_model_update": (C.c_int32, [_P, C.POINTER(_P), C.POINTER(ModelDesc)]),
    "svgp_group_elbo": (C.c_int32, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_double,
                                    C.POINTER(C.c_double), C.POINTER(Terms)]),
    "svgp_group_elbo_grad": (C.c_int32, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                         C.c_double, C.POINTER(C.c_double), C.POINTER(Terms), C.POINTER(Grads)]),
}
COMM_ID_BYTES = 128

_lib = None


def load_library():
    """dlopen the in-tree library and type every symbol.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with ./build.sh (hipcc --offload-arch=gfx950). "
            "This package has no CPU implementation."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# ---- exceptions mirroring the Julia ones the shim raises --------------------------
class SvgpError(RuntimeError):
    pass


class PosDefException(SvgpError):
    def __init__(self, info, msg=""):
        super().__init__(msg or f"matrix is not positive definite; Cholesky factorization failed (info={info})")
        self.info = info


class DomainError(SvgpError):
    pass


class DeclinedError(SvgpError):
    """The problem is below the library's offload threshold (svgp_offload_advice): the Julia hooks return `nothing` here and
    the reference's own method body runs; the Python mirror has no host path to fall back to and says so."""


def offload_advice(n_points: int, M: int, d: int, dtype=F64, want_gradient=False) -> bool:
    """True when a problem of this size is worth sending to the device (include/svgp_mi355x.h: svgp_offload_advice)."""
    return bool(load_library().svgp_offload_advice(int(n_points), int(M), int(d), int(dtype), int(bool(want_gradient))))


def offload_work(n_points: int, M: int, d: int) -> float:
    return float(load_library().svgp_offload_work(int(n_points), int(M), int(d)))


class UnsupportedError(SvgpError):
    pass


def np_dtype(dtype: int):
    return np.float64 if dtype == F64 else np.float32


def dtype_code(dt) -> int:
    dt = np.dtype(dt)
    if dt == np.float64:
        return F64
    if dt == np.float32:
        return F32
    raise UnsupportedError(f"unsupported element type {dt}; use float64 or float32")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _is_device_tensor(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def point_mean_grad_ptr(dst, n, dtype):
    """Device address for d elbo / d mux of n points: a device tensor (checked: CUDA, contiguous, floating, the data dtype's element
    size, at least n elements - the library writes n of them) or a raw device pointer (the caller's to size: n x dtype size bytes)."""
    if hasattr(dst, "data_ptr"):
        if (not _is_device_tensor(dst) or not dst.is_contiguous() or not dst.is_floating_point()
                or dst.element_size() != np.dtype(np_dtype(dtype)).itemsize or dst.numel() < n):
            raise ValueError("mean_grad: a contiguous device tensor of the data dtype with at least one entry per point of the batch")
        return int(dst.data_ptr())
    if isinstance(dst, (bool, np.bool_)) or not isinstance(dst, (int, np.integer)):
        raise ValueError("mean_grad: True, a device tensor or a device pointer (int)")
    return int(dst)


def point_mean(mu, n, dtype):
    """-> (PointMean, what keeps its memory alive) for prior mean offsets of n points: a host array (converted to the data dtype) or a
    contiguous device tensor of the data dtype (read on the context's stream)."""
    if _is_device_tensor(mu):
        if mu.numel() != n or not mu.is_contiguous() or mu.element_size() != np.dtype(np_dtype(dtype)).itemsize or not mu.is_floating_point():
            raise ValueError("prior_mean: a contiguous device tensor of the data dtype with one entry per point of the batch")
        return PointMean(C.c_void_p(mu.data_ptr()), 1, 0), mu
    buf = np.ascontiguousarray(np.asarray(mu, dtype=np_dtype(dtype)).reshape(-1))
    if buf.shape != (n,):
        raise ValueError("prior_mean: one entry per point of the batch")
    return PointMean(_ptr(buf), 0, 0), buf


def point_noise(s, n, dtype):
    """-> (PointNoise, what keeps its memory alive) for per-point noise variances of n points (added to the model's lik_sigma2): a
    host array (converted to the data dtype) or a contiguous device tensor of the data dtype (read on the context's stream)."""
    if _is_device_tensor(s):
        if s.numel() != n or not s.is_contiguous() or s.element_size() != np.dtype(np_dtype(dtype)).itemsize or not s.is_floating_point():
            raise ValueError("noise: a contiguous device tensor of the data dtype with one entry per point of the batch")
        return PointNoise(C.c_void_p(s.data_ptr()), 1, 0), s
    buf = np.ascontiguousarray(np.asarray(s, dtype=np_dtype(dtype)).reshape(-1))
    if buf.shape != (n,):
        raise ValueError("noise: one entry per point of the batch")
    return PointNoise(_ptr(buf), 0, 0), buf


PRED_WANTS = ("summary", "lpd", "ymean", "yvar")


def _pred_wants(want, has_y):
    """The outputs asked of svgp_predictive / svgp_lik_predictive, checked as the library checks them (before the GPU is touched)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in PRED_WANTS for w in want):
        raise ValueError(f"want: a non-empty selection of {PRED_WANTS}")
    if not has_y and ("summary" in want or "lpd" in want):
        raise ValueError("no observations y: only ymean and yvar are available (summary and lpd need y)")
    return want


def _pred_call(ctx, want, n, call):
    """Allocates the wanted outputs, runs call(summary_ref, lpd_ptr, ymean_ptr, yvar_ptr) -> status and packs the result.  Under the error
    policy a negative variance raises DomainError carrying the (written) outputs as its `outputs` attribute: NaN at the bad points."""
    summary = PredSummary() if "summary" in want else None
    arrs = {k: np.zeros(n) for k in ("lpd", "ymean", "yvar") if k in want}
    rc = call(C.byref(summary) if summary is not None else None, _ptr(arrs.get("lpd")), _ptr(arrs.get("ymean")), _ptr(arrs.get("yvar")))
    res = dict(arrs)
    if summary is not None:
        res["summary"] = summary
    try:
        ctx.check(rc)
    except DomainError as e:
        e.outputs = res
        raise
    return res


def lik_predictive(ctx, lik: int, param: float, quadrature_n: int, mu, var, y=None, want=None):
    """svgp_lik_predictive: log predictive density and (E[y], Var[y]) from latent marginals N(mu_i, var_i) a caller holds (Laplace,
    NearestNeighbors, svgp_marginals' output) -> dict of the wanted outputs (default: all four with y, ymean / yvar without)."""
    mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(-1))
    var = np.ascontiguousarray(np.asarray(var, dtype=np.float64).reshape(-1))
    yb = None if y is None else np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    want = _pred_wants(want if want is not None else (PRED_WANTS if yb is not None else ("ymean", "yvar")), yb is not None)
    n = mu.shape[0]
    if n < 1:
        raise ValueError("n must be >= 1")
    if var.shape != (n,) or (yb is not None and yb.shape != (n,)):
        raise ValueError("mu, var and y must have one entry per point")
    if isinstance(lik, bool) or not isinstance(lik, (int, np.integer)) or not LIK_GAUSSIAN <= lik <= LIK_BERNOULLI_NORMCDF:
        raise ValueError(f"unsupported likelihood code {lik!r}")
    if not 0 <= int(quadrature_n) <= 512:
        raise ValueError("quadrature_n must be in 0..512")
    if lik in (LIK_GAUSSIAN, LIK_GAMMA_EXP) and not float(param) > 0:
        raise ValueError("the Gaussian likelihood needs sigma2 > 0, the Gamma likelihood a shape alpha > 0")
    return _pred_call(ctx, want, n, lambda s, a, b, c: ctx.lib.svgp_lik_predictive(ctx.h, int(lik), float(param), int(quadrature_n), n, _ptr(mu),
                                                                                   _ptr(var), _ptr(yb), s, a, b, c))


class Context:
    """One GPU + one HIP stream.  `stream` may be a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load_library()
        if self.lib.svgp_device_count() < 1:
            raise SvgpError("no HIP device visible: libsvgp_mi355x has no CPU path")
        h = C.c_void_p()
        rc = self.lib.svgp_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != OK:
            raise SvgpError(f"svgp_ctx_create failed with status {rc}")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.svgp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, terms: Terms | None = None):
        if rc == OK:
            return
        msg = (self.lib.svgp_last_error(self.h) or b"").decode()
        if rc == INVALID_ARG:
            raise ValueError(msg)  # Julia ArgumentError
        if rc == NOT_POSDEF:
            raise PosDefException(terms.chol_info if terms is not None else -1, msg)
        if rc == NEG_VARIANCE:
            raise DomainError(msg)
        if rc == UNSUPPORTED:
            raise UnsupportedError(msg)
        if rc == OOM:
            raise MemoryError(msg)
        raise SvgpError(f"status {rc}: {msg}")

    def timing(self) -> Timing:
        t = Timing()
        self.lib.svgp_last_timing_sized(self.h, C.byref(t), C.sizeof(Timing))
        return t

    # ---- multi-GPU: one process per GPU (include/svgp_mi355x.h "multi-GPU") ----
    def attach_comm(self, comm_id: bytes, world_size: int, rank: int):
        """Collective over all ranks (ncclCommInitRank).  Afterwards DeviceModel.elbo / elbo_grad on this context are
        collective and return the GLOBAL ELBO; elbo_partial / elbo_grad(shard=...) stay local."""
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("communicator id must be SVGP_COMM_ID_BYTES long")
        buf = C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self.check(self.lib.svgp_ctx_attach_comm(self.h, C.cast(buf, C.c_void_p), world_size, rank))

    def detach_comm(self):
        self.check(self.lib.svgp_ctx_detach_comm(self.h))

    def comm_info(self):
        w, r = C.c_int32(), C.c_int32()
        self.lib.svgp_ctx_comm_info(self.h, C.byref(w), C.byref(r))
        return w.value, r.value


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it; the host transports the bytes to the other ranks)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load_library().svgp_comm_unique_id(C.cast(buf, C.c_void_p))
    if rc != OK:
        raise SvgpError(f"svgp_comm_unique_id failed with status {rc} (is librccl loadable?)")
    return buf.raw


_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class DeviceData:
    """x = lfx.fx.x and y resident in HBM (svgp_data)."""

    def __init__(self, ctx: Context, x: np.ndarray, y: np.ndarray | None, dtype, layout: int = COLVECS):
        self.ctx = ctx
        dt = np_dtype(dtype_code(dtype))
        x = np.asarray(x, dtype=dt)
        if x.ndim == 1:
            layout, d, n = VEC, 1, x.shape[0]
            xbuf = np.ascontiguousarray(x)
        elif layout == COLVECS:
            d, n = x.shape  # (d, n) numpy view of Julia's d×n column-major matrix: point-contiguous
            xbuf = np.asfortranarray(x)
        else:
            n, d = x.shape  # RowVecs: n×d column-major, feature-contiguous
            xbuf = np.asfortranarray(x)
        self._x = xbuf
        self.layout = layout
        self._y = None if y is None else np.ascontiguousarray(np.asarray(y, dtype=dt))
        if self._y is not None and self._y.shape[0] != n:
            raise ValueError("x and y lengths differ")
        self.n, self.d, self.dtype = n, d, dtype_code(dt)
        self.has_y = self._y is not None
        h = C.c_void_p()
        ctx.check(ctx.lib.svgp_data_upload(ctx.h, self.dtype, layout, d, n, _ptr(self._x), _ptr(self._y), C.byref(h)))
        self.h = h

    @classmethod
    def wrap(cls, ctx: Context, dtype, d: int, n: int, ldx: int, x_ptr: int, y_ptr: int | None):
        self = cls.__new__(cls)
        self.ctx, self.n, self.d, self.dtype = ctx, n, d, dtype_code(dtype)
        self.layout = ROWVECS   # feature-major storage
        self.has_y = bool(y_ptr)
        h = C.c_void_p()
        ctx.check(ctx.lib.svgp_data_wrap_device(ctx.h, self.dtype, d, n, ldx, C.c_void_p(x_ptr),
                                                C.c_void_p(y_ptr) if y_ptr else None, C.byref(h)))
        self.h = h
        return self

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_data_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def make_desc(dtype, kernel, variance, inv_lengthscale, z, m, Lq, jitter, *, parametrization=NONCENTERED,
              likelihood=LIK_GAUSSIAN, lik_sigma2=1.0, quadrature_n=0, mean_const=0.0, neg_var_policy=NEGVAR_ERROR,
              layout_z=COLVECS):
    """Builds a svgp_model_desc plus the numpy buffers it borrows (keep the returned tuple alive)."""
    code = dtype_code(dtype)
    dt = np_dtype(code)
    z = np.asarray(z, dtype=dt)
    if z.ndim == 1:
        layout_z, d, M = VEC, 1, z.shape[0]
        zbuf = np.ascontiguousarray(z)
    elif layout_z == COLVECS:
        d, M = z.shape
        zbuf = np.asfortranarray(z)
    else:
        M, d = z.shape
        zbuf = np.asfortranarray(z)
    il = np.ascontiguousarray(np.broadcast_to(np.asarray(inv_lengthscale, dtype=np.float64), (d,)))
    mbuf = np.ascontiguousarray(np.asarray(m, dtype=dt))
    Lbuf = np.asfortranarray(np.asarray(Lq, dtype=dt))
    if mbuf.shape != (M,) or Lbuf.shape != (M, M):
        raise ValueError("m must have M entries and Lq must be M×M")
    desc = ModelDesc(code, kernel, parametrization, likelihood, quadrature_n, layout_z, neg_var_policy, d, M,
                     float(variance), il.ctypes.data_as(C.POINTER(C.c_double)), float(mean_const), float(jitter),
                     float(lik_sigma2), _ptr(zbuf), _ptr(mbuf), _ptr(Lbuf))
    return desc, (il, zbuf, mbuf, Lbuf)


class DeviceModel:
    """SparseVariationalApproximation(fz, q) + likelihood resident in HBM (svgp_model)."""

    def __init__(self, ctx: Context, desc: ModelDesc, keep):
        self.ctx = ctx
        self.M, self.d, self.dtype = desc.M, desc.d, desc.dtype
        h = C.c_void_p()
        ctx.check(ctx.lib.svgp_model_create(ctx.h, C.byref(desc), C.byref(h)))
        self.h = h
        del keep

    def update(self, desc: ModelDesc, keep):
        self.ctx.check(self.ctx.lib.svgp_model_update(self.ctx.h, self.h, C.byref(desc)))
        del keep

    def update_keep_q(self, desc: ModelDesc, keep):
        """svgp_model_update_keep_q: new kernel parameters, z, likelihood parameters, jitter and mean_const go up; desc.m / desc.Lq are
        ignored (they may be NULL) and the device-resident q - e.g. what natgrad_step wrote - stays."""
        self.ctx.check(self.ctx.lib.svgp_model_update_keep_q(self.ctx.h, self.h, C.byref(desc)))
        del keep

    def set_mean_z(self, mu_z):
        """mean(fz) = mean_const + mu_z (M host values; None removes them): svgp_model_set_mean_z.  Centered models only depend on it."""
        if mu_z is None:
            self.ctx.check(self.ctx.lib.svgp_model_set_mean_z(self.ctx.h, self.h, None))
            return
        buf = np.ascontiguousarray(np.asarray(mu_z, dtype=np_dtype(self.dtype)).reshape(-1))
        if buf.shape != (self.M,):
            raise ValueError("mu_z must have M entries")
        self.ctx.check(self.ctx.lib.svgp_model_set_mean_z(self.ctx.h, self.h, _ptr(buf)))

    def elbo(self, data: DeviceData, off=0, length=None, num_data=0.0, prior_mean=None):
        """prior_mean: the batch's prior mean offsets mux (host array or device tensor; svgp_elbo_with_mean)."""
        length = data.n - off if length is None else length
        out, terms = C.c_double(), Terms()
        if prior_mean is not None:
            pm, _keep = point_mean(prior_mean, length, self.dtype)
            rc = self.ctx.lib.svgp_elbo_with_mean(self.ctx.h, self.h, data.h, off, length, float(num_data), C.byref(pm), C.byref(out),
                                                  C.byref(terms))
        else:
            rc = self.ctx.lib.svgp_elbo(self.ctx.h, self.h, data.h, off, length, float(num_data), C.byref(out), C.byref(terms))
        self.ctx.check(rc, terms)
        return out.value, terms

    def elbo_partial(self, data: DeviceData, off=0, length=None):
        length = data.n - off if length is None else length
        buf = (C.c_double * 4)()
        self.ctx.check(self.ctx.lib.svgp_elbo_partial(self.ctx.h, self.h, data.h, off, length, buf))
        return np.array(buf[:], dtype=np.float64)

    def marginals(self, data: DeviceData, off=0, length=None, prior_mean=None):
        """marginals(f_post(x)) of SVA:354 for the batch: (mu, v + 1e-18) as fp64 arrays (svgp_marginals; with prior_mean, the
        batch's prior mean offsets: svgp_marginals_with_mean)."""
        length = data.n - off if length is None else length
        mu, var = np.zeros(length), np.zeros(length)
        if prior_mean is not None:
            pm, _keep = point_mean(prior_mean, length, self.dtype)
            self.ctx.check(self.ctx.lib.svgp_marginals_with_mean(self.ctx.h, self.h, data.h, off, length, C.byref(pm), _ptr(mu), _ptr(var)))
        else:
            self.ctx.check(self.ctx.lib.svgp_marginals(self.ctx.h, self.h, data.h, off, length, _ptr(mu), _ptr(var)))
        return mu, var

    def predictive(self, data: DeviceData, off=0, length=None, prior_mean=None, want=PRED_WANTS):
        """svgp_predictive: the predictive distribution of the OBSERVATION for the batch, through the model's likelihood -> dict of the
        wanted outputs: "summary" (PredSummary: sum of lpd, sum of (y - E[y])^2, n_points, n_neg_var), "lpd" (log p(y_i | D)), "ymean",
        "yvar" (fp64 arrays).  One forward data pass, local even on a context with a communicator.  Data without y: ymean / yvar only.
        prior_mean: the batch's prior mean offsets, as in marginals."""
        length = data.n - off if length is None else length
        want = _pred_wants(want, bool(getattr(data, "has_y", False)))
        if off < 0 or length < 1 or off + length > data.n:
            raise ValueError("batch range outside the data")
        pm, _keep = point_mean(prior_mean, length, self.dtype) if prior_mean is not None else (None, None)
        ctx = self.ctx
        return _pred_call(ctx, want, length, lambda s, a, b, c: ctx.lib.svgp_predictive(ctx.h, self.h, data.h, off, length,
                                                                                        C.byref(pm) if pm is not None else None, s, a, b, c))

    def elbo_grad(self, data: DeviceData, off=0, length=None, num_data=0.0, z_shape=None, shard=None, ext=None, out=None,
                  inputs=None, prior_mean=None, mean_grad=None):
        """-> (elbo, terms, dict(variance, inv_lengthscale, z, m, Lq, lik_sigma2, mean_const)); z in the layout it was given.
        shard = (scale, kl_weight) evaluates the data-parallel shard form svgp_elbo_grad_shard instead.
        ext = (sum_e, g_mu, g_v): a likelihood the host evaluated on `marginals` (svgp_elbo_grad_ext).
        out = the gradient dict of an earlier call: its arrays are written in place instead of allocating M^2 fresh elements per step
        (a training loop that has consumed the previous gradient; at M = 2048 the first touch of 33 MB of new pages costs ~2 ms).
        inputs = True: also d elbo / d x of the batch as dict["x"], a host array in the data's layout (ColVecs (d, n), RowVecs and
        wrapped device data (n, d), a vector (n,)); inputs = (device_ptr, ld): written to device memory, element (f, j) at
        device_ptr[f * ld + j] on the context's stream (svgp_elbo_grad_inputs / svgp_elbo_grad_ext_inputs).
        prior_mean = the batch's prior mean offsets mux (host array or device tensor); mean_grad = True: also d elbo / d mux as
        dict["mean_x"] (host, data dtype); mean_grad = a device tensor or pointer: written there on the context's stream
        (svgp_elbo_grad_with_mean, which also serves ext and inputs then)."""
        length = data.n - off if length is None else length
        with_mean = prior_mean is not None or (mean_grad is not None and mean_grad is not False)
        if with_mean and shard is not None:
            raise ValueError("prior mean offsets are not available for the shard form (svgp_elbo_grad_shard)")
        gx, xb = None, None
        if inputs is not None and inputs is not False:
            if shard is not None:
                raise ValueError("d elbo / d x is not available for the shard form (svgp_elbo_grad_shard)")
            if inputs is True:
                layout = getattr(data, "layout", COLVECS)
                if layout == VEC:
                    xb = np.zeros(length, dtype=np_dtype(self.dtype))
                elif layout == COLVECS:
                    xb = np.zeros((data.d, length), dtype=np_dtype(self.dtype))              # C order: feature-major, ld = length
                else:
                    xb = np.zeros((length, data.d), dtype=np_dtype(self.dtype), order="F")   # F order: feature-major, ld = length
                gx = InputGrad(_ptr(xb), length, 0, 0)
            else:
                ptr, ld = inputs
                gx = InputGrad(C.c_void_p(int(ptr)), int(ld), 1, 0)
        dt = np_dtype(self.dtype)
        zshape = z_shape if z_shape is not None else ((self.M,) if self.d == 1 else (self.d, self.M))
        if out is not None:
            il, zb, mb, Lb = out["inv_lengthscale"], out["z"], out["m"], out["Lq"]
            ok = (il.dtype == np.float64 and il.shape == (self.d,) and zb.dtype == dt and zb.shape == tuple(zshape) and zb.flags.f_contiguous
                  and mb.dtype == dt and mb.shape == (self.M,) and Lb.dtype == dt and Lb.shape == (self.M, self.M) and Lb.flags.f_contiguous)
            if not ok:
                raise ValueError("out= must be the gradient dict of an earlier call on a model of the same shape and dtype")
        else:
            il = np.zeros(self.d)
            zb = np.zeros(zshape, dtype=dt, order="F")
            mb = np.zeros(self.M, dtype=dt)
            Lb = np.zeros((self.M, self.M), dtype=dt, order="F")
        g = Grads(0.0, 0.0, 0.0, il.ctypes.data_as(C.POINTER(C.c_double)), _ptr(zb), _ptr(mb), _ptr(Lb))
        out, terms = C.c_double(), Terms()
        mxb = None
        if with_mean:
            pm, _keep = point_mean(prior_mean, length, self.dtype) if prior_mean is not None else (None, None)
            gpm = None
            if mean_grad is True:
                mxb = np.zeros(length, dtype=dt)
                gpm = PointMeanGrad(_ptr(mxb), 0, 0)
            elif mean_grad is not None and mean_grad is not False:
                gpm = PointMeanGrad(C.c_void_p(point_mean_grad_ptr(mean_grad, length, self.dtype)), 1, 0)
            sum_e, gmu, gv = 0.0, None, None
            if ext is not None:
                gmu, gv = (np.ascontiguousarray(a, dtype=np.float64) for a in ext[1:])
                if gmu.shape != (length,) or gv.shape != (length,):
                    raise ValueError("one point gradient per point of the batch")
                sum_e = float(ext[0])
            rc = self.ctx.lib.svgp_elbo_grad_with_mean(self.ctx.h, self.h, data.h, off, length, float(num_data),
                                                       C.byref(pm) if pm is not None else None, sum_e, _ptr(gmu), _ptr(gv),
                                                       C.byref(out), C.byref(terms), C.byref(g), C.byref(gx) if gx is not None else None,
                                                       C.byref(gpm) if gpm is not None else None)
        elif ext is not None:
            gmu, gv = (np.ascontiguousarray(a, dtype=np.float64) for a in ext[1:])
            if gmu.shape != (length,) or gv.shape != (length,):
                raise ValueError("one point gradient per point of the batch")
            if gx is not None:
                rc = self.ctx.lib.svgp_elbo_grad_ext_inputs(self.ctx.h, self.h, data.h, off, length, float(num_data), float(ext[0]),
                                                            _ptr(gmu), _ptr(gv), C.byref(out), C.byref(terms), C.byref(g), C.byref(gx))
            else:
                rc = self.ctx.lib.svgp_elbo_grad_ext(self.ctx.h, self.h, data.h, off, length, float(num_data), float(ext[0]),
                                                     _ptr(gmu), _ptr(gv), C.byref(out), C.byref(terms), C.byref(g))
        elif gx is not None:
            rc = self.ctx.lib.svgp_elbo_grad_inputs(self.ctx.h, self.h, data.h, off, length, float(num_data), C.byref(out),
                                                    C.byref(terms), C.byref(g), C.byref(gx))
        elif shard is None:
            rc = self.ctx.lib.svgp_elbo_grad(self.ctx.h, self.h, data.h, off, length, float(num_data), C.byref(out),
                                             C.byref(terms), C.byref(g))
        else:
            rc = self.ctx.lib.svgp_elbo_grad_shard(self.ctx.h, self.h, data.h, off, length, float(shard[0]), float(shard[1]),
                                                   C.byref(out), C.byref(terms), C.byref(g))
        self.ctx.check(rc, terms)
        res = dict(variance=g.variance, inv_lengthscale=il, z=zb, m=mb, Lq=Lb, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const)
        if xb is not None:
            res["x"] = xb
        if mxb is not None:
            res["mean_x"] = mxb
        return out.value, terms, res

    # ---- the collapsed (Titsias) bound and the optimal q (svgp_collapsed_*) ----
    def _collapsed_check(self, rc, terms):
        if rc == NOT_POSDEF and terms is not None:
            msg = (self.ctx.lib.svgp_last_error(self.ctx.h) or b"").decode()
            raise PosDefException(terms.chol_info if terms.chol_info else terms.chol_info_b, msg)
        self.ctx.check(rc)

    def _collapsed_ext(self, length, prior_mean, noise, mean_z):
        """-> (pm, pn, keep-alive) of a svgp_collapsed_*_with_noise call, or None for the plain call (no offsets, no noise vector and
        mean_z false: the two are bitwise equal there, but only the _with_noise calls accept a model that carries muz)."""
        if prior_mean is None and noise is None and not mean_z:
            return None
        pm, k1 = point_mean(prior_mean, length, self.dtype) if prior_mean is not None else (None, None)
        pn, k2 = point_noise(noise, length, self.dtype) if noise is not None else (None, None)
        return pm, pn, (k1, k2)

    def collapsed_bound(self, data: DeviceData, off=0, length=None, prior_mean=None, noise=None, mean_z=False):
        """-> (bound, CollapsedTerms): one data pass; the model's q is neither read nor changed.
        prior_mean = the batch's prior mean offsets mux, noise = its per-point noise variances s (sigma_j^2 = lik_sigma2 + s_j); each
        a host array or a device tensor of the data dtype (svgp_collapsed_bound_with_noise).  mean_z = True: the model carries muz
        (set_mean_z), which only the _with_noise calls accept; it enters the Centered m of collapsed_q, never the bound."""
        length = data.n - off if length is None else length
        out, terms = C.c_double(), CollapsedTerms()
        ext = self._collapsed_ext(length, prior_mean, noise, mean_z)
        if ext is None:
            rc = self.ctx.lib.svgp_collapsed_bound(self.ctx.h, self.h, data.h, off, length, C.byref(out), C.byref(terms))
        else:
            pm, pn, _keep = ext
            rc = self.ctx.lib.svgp_collapsed_bound_with_noise(self.ctx.h, self.h, data.h, off, length, C.byref(pm) if pm is not None else None,
                                                              C.byref(pn) if pn is not None else None, C.byref(out), C.byref(terms))
        self._collapsed_check(rc, terms)
        return out.value, terms

    def collapsed_q(self, data: DeviceData, off=0, length=None, fetch=True, prior_mean=None, noise=None, mean_z=False):
        """Writes the optimal q into the model's device-resident m / Lq (the model's own parametrisation) -> (bound, m, Lq); m and
        Lq are host copies in the model's dtype (Lq lower triangular), None with fetch=False.  prior_mean, noise: as in
        collapsed_bound (svgp_collapsed_q_with_noise)."""
        length = data.n - off if length is None else length
        dt = np_dtype(self.dtype)
        mb = np.zeros(self.M, dtype=dt) if fetch else None
        Lb = np.zeros((self.M, self.M), dtype=dt, order="F") if fetch else None
        out = C.c_double()
        ext = self._collapsed_ext(length, prior_mean, noise, mean_z)
        if ext is None:
            self.ctx.check(self.ctx.lib.svgp_collapsed_q(self.ctx.h, self.h, data.h, off, length, _ptr(mb), _ptr(Lb), C.byref(out)))
        else:
            pm, pn, _keep = ext
            self.ctx.check(self.ctx.lib.svgp_collapsed_q_with_noise(self.ctx.h, self.h, data.h, off, length,
                                                                    C.byref(pm) if pm is not None else None,
                                                                    C.byref(pn) if pn is not None else None, _ptr(mb), _ptr(Lb), C.byref(out)))
        return out.value, mb, Lb

    def collapsed_grad(self, data: DeviceData, off=0, length=None, z_shape=None, inputs=None, prior_mean=None, noise=None,
                       want_mean_grad=None, want_noise_grad=None, mean_z=False):
        """-> (bound, CollapsedTerms, dict(variance, inv_lengthscale, z, lik_sigma2, mean_const[, x][, mean_x][, noise])): the bound's
        total derivatives (svgp_collapsed_q, then the value-and-gradient at that q).  inputs = True: also d bound / d x as dict["x"]
        (host, the data's layout); inputs = (device_ptr, ld): written to device memory as in elbo_grad.
        prior_mean, noise: as in collapsed_bound.  want_mean_grad / want_noise_grad = True: d bound / d mux as dict["mean_x"] and
        d bound / d sigma_j^2 as dict["noise"] (host, data dtype); a device tensor or pointer: written there on the context's stream
        (svgp_collapsed_grad_with_noise)."""
        length = data.n - off if length is None else length
        dt = np_dtype(self.dtype)
        gx, xb = None, None
        if inputs is not None and inputs is not False:
            if inputs is True:
                layout = getattr(data, "layout", COLVECS)
                if layout == VEC:
                    xb = np.zeros(length, dtype=dt)
                elif layout == COLVECS:
                    xb = np.zeros((data.d, length), dtype=dt)
                else:
                    xb = np.zeros((length, data.d), dtype=dt, order="F")
                gx = InputGrad(_ptr(xb), length, 0, 0)
            else:
                ptr, ld = inputs
                gx = InputGrad(C.c_void_p(int(ptr)), int(ld), 1, 0)
        zshape = z_shape if z_shape is not None else ((self.M,) if self.d == 1 else (self.d, self.M))
        il = np.zeros(self.d)
        zb = np.zeros(zshape, dtype=dt, order="F")
        g = Grads(0.0, 0.0, 0.0, il.ctypes.data_as(C.POINTER(C.c_double)), _ptr(zb), None, None)
        out, terms = C.c_double(), CollapsedTerms()
        wants = [w is not None and w is not False for w in (want_mean_grad, want_noise_grad)]
        ext = self._collapsed_ext(length, prior_mean, noise, mean_z)
        mxb = sxb = None
        if ext is None and not any(wants):
            rc = self.ctx.lib.svgp_collapsed_grad(self.ctx.h, self.h, data.h, off, length, C.byref(out), C.byref(terms), C.byref(g),
                                                  C.byref(gx) if gx is not None else None)
        else:
            pm, pn, _keep = ext if ext is not None else (None, None, None)
            gpm = gpn = None
            if want_mean_grad is True:
                mxb = np.zeros(length, dtype=dt)
                gpm = PointMeanGrad(_ptr(mxb), 0, 0)
            elif wants[0]:
                gpm = PointMeanGrad(C.c_void_p(point_mean_grad_ptr(want_mean_grad, length, self.dtype)), 1, 0)
            if want_noise_grad is True:
                sxb = np.zeros(length, dtype=dt)
                gpn = PointNoiseGrad(_ptr(sxb), 0, 0)
            elif wants[1]:
                gpn = PointNoiseGrad(C.c_void_p(point_mean_grad_ptr(want_noise_grad, length, self.dtype)), 1, 0)
            rc = self.ctx.lib.svgp_collapsed_grad_with_noise(self.ctx.h, self.h, data.h, off, length,
                                                             C.byref(pm) if pm is not None else None,
                                                             C.byref(pn) if pn is not None else None, C.byref(out), C.byref(terms),
                                                             C.byref(g), C.byref(gx) if gx is not None else None,
                                                             C.byref(gpm) if gpm is not None else None,
                                                             C.byref(gpn) if gpn is not None else None)
        self._collapsed_check(rc, terms)
        res = dict(variance=g.variance, inv_lengthscale=il, z=zb, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const)
        if xb is not None:
            res["x"] = xb
        if mxb is not None:
            res["mean_x"] = mxb
        if sxb is not None:
            res["noise"] = sxb
        return out.value, terms, res

    # ---- natural-gradient steps on q (svgp_natgrad_step / _ext) ----
    def natgrad_step(self, data: DeviceData, off=0, length=None, num_data=0.0, gamma=1.0, ext=None, want_grads=False, fetch=True,
                     z_shape=None):
        """One natural-gradient step of length gamma in (0, 1] on the model's device-resident q -> (elbo, terms, grads, m, Lq).
        elbo, terms and grads (the dict of elbo_grad with want_grads=True, else None) are the values at the q the call started from;
        m and Lq are host copies of the NEW q in the model's dtype and parametrisation (None with fetch=False).
        ext = (sum_e, g_mu, g_v): a likelihood the host evaluated on `marginals` (svgp_natgrad_step_ext)."""
        length = data.n - off if length is None else length
        dt = np_dtype(self.dtype)
        mb = np.zeros(self.M, dtype=dt) if fetch else None
        Lb = np.zeros((self.M, self.M), dtype=dt, order="F") if fetch else None
        g, res = None, None
        if want_grads:
            zshape = z_shape if z_shape is not None else ((self.M,) if self.d == 1 else (self.d, self.M))
            il = np.zeros(self.d)
            zb = np.zeros(zshape, dtype=dt, order="F")
            gm = np.zeros(self.M, dtype=dt)
            gL = np.zeros((self.M, self.M), dtype=dt, order="F")
            g = Grads(0.0, 0.0, 0.0, il.ctypes.data_as(C.POINTER(C.c_double)), _ptr(zb), _ptr(gm), _ptr(gL))
        out, terms = C.c_double(), Terms()
        gref = C.byref(g) if g is not None else None
        if ext is not None:
            gmu, gv = (np.ascontiguousarray(a, dtype=np.float64) for a in ext[1:])
            if gmu.shape != (length,) or gv.shape != (length,):
                raise ValueError("one point gradient per point of the batch")
            rc = self.ctx.lib.svgp_natgrad_step_ext(self.ctx.h, self.h, data.h, off, length, float(num_data), float(gamma), float(ext[0]),
                                                    _ptr(gmu), _ptr(gv), C.byref(out), C.byref(terms), gref, _ptr(mb), _ptr(Lb))
        else:
            rc = self.ctx.lib.svgp_natgrad_step(self.ctx.h, self.h, data.h, off, length, float(num_data), float(gamma), C.byref(out),
                                                C.byref(terms), gref, _ptr(mb), _ptr(Lb))
        self.ctx.check(rc, terms)
        if g is not None:
            res = dict(variance=g.variance, inv_lengthscale=il, z=zb, m=gm, Lq=gL, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const)
        return out.value, terms, res, mb, Lb

    def prior_kl(self):
        kl, ld = C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.svgp_prior_kl(self.ctx.h, self.h, C.byref(kl), C.byref(ld)))
        return kl.value, ld.value

    def posterior(self):
        dt = np_dtype(self.dtype)
        Lk = np.zeros((self.M, self.M), dtype=dt, order="F")
        alpha = np.zeros(self.M, dtype=dt)
        B = np.zeros((self.M, self.M), dtype=dt, order="F")
        self.ctx.check(self.ctx.lib.svgp_posterior(self.ctx.h, self.h, _ptr(Lk), _ptr(alpha), _ptr(B)))
        return Lk, alpha, B

    def predict(self, x, want_mean=True, want_var=True, want_cov=False, layout=COLVECS):
        dt = np_dtype(self.dtype)
        x = np.asarray(x, dtype=dt)
        if x.ndim == 1:
            layout, n, xb = VEC, x.shape[0], np.ascontiguousarray(x)
        else:
            n = x.shape[1] if layout == COLVECS else x.shape[0]
            xb = np.asfortranarray(x)
        mean = np.zeros(n, dtype=dt) if want_mean else None
        var = np.zeros(n, dtype=dt) if want_var else None
        cov = np.zeros((n, n), dtype=dt, order="F") if want_cov else None
        self.ctx.check(self.ctx.lib.svgp_predict(self.ctx.h, self.h, layout, n, _ptr(xb), _ptr(mean), _ptr(var), _ptr(cov)))
        return mean, var, cov

    def cross_cov(self, x, y, layout=COLVECS):
        dt = np_dtype(self.dtype)
        x, y = np.asarray(x, dtype=dt), np.asarray(y, dtype=dt)
        if x.ndim == 1:
            layout, nx, ny = VEC, x.shape[0], y.shape[0]
            xb, yb = np.ascontiguousarray(x), np.ascontiguousarray(y)
        else:
            nx = x.shape[1] if layout == COLVECS else x.shape[0]
            ny = y.shape[1] if layout == COLVECS else y.shape[0]
            xb, yb = np.asfortranarray(x), np.asfortranarray(y)
        cov = np.zeros((nx, ny), dtype=dt, order="F")
        self.ctx.check(self.ctx.lib.svgp_predict_cross_cov(self.ctx.h, self.h, layout, nx, _ptr(xb), ny, _ptr(yb), _ptr(cov)))
        return cov

    def sampler(self, basis):
        """svgp_sampler_create: S pathwise posterior function samples from `basis` = (omega (L, d), tau (L,), w (S, L), eps (S, M)) - every
        random number is the caller's (approxgp.pathwise.draw_basis draws them).  The DeviceSampler is a snapshot of this model."""
        return DeviceSampler(self, *basis)

    def kuf(self, data: DeviceData, off=0, length=None, fetch=True):
        length = data.n - off if length is None else length
        out = np.zeros((self.M, length), dtype=np_dtype(self.dtype), order="F") if fetch else None
        self.ctx.check(self.ctx.lib.svgp_kuf(self.ctx.h, self.h, data.h, off, length, _ptr(out)))
        return out

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_model_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceSampler:
    """S function samples of a model's posterior, resident in HBM (svgp_sampler): evaluate them anywhere, any number of times."""

    def __init__(self, model: DeviceModel, omega, tau, w, eps):
        self.ctx = ctx = model.ctx
        self.M, self.d, self.dtype = model.M, model.d, model.dtype
        dt = np_dtype(self.dtype)
        eps = np.ascontiguousarray(np.asarray(eps, dtype=dt))
        if eps.ndim != 2 or eps.shape[1] != self.M or eps.shape[0] < 1:
            raise ValueError("eps must be (S, M) with S >= 1")
        S = eps.shape[0]
        w = np.ascontiguousarray(np.asarray(np.zeros((S, 0)) if w is None else w, dtype=dt).reshape(S, -1))
        L = w.shape[1]
        omega = np.ascontiguousarray(np.asarray(omega, dtype=dt).reshape(L, self.d))
        tau = np.ascontiguousarray(np.asarray(tau, dtype=dt).reshape(L))
        self.n_samples, self.n_features = S, L
        basis = SampleBasis(L, S, _ptr(omega) if L else None, _ptr(tau) if L else None, _ptr(w) if L else None, _ptr(eps))
        h = C.c_void_p()
        ctx.check(ctx.lib.svgp_sampler_create(ctx.h, model.h, C.byref(basis), C.byref(h)))
        self.h = h

    def eval(self, data: DeviceData, off=0, length=None, prior_mean=None, out=None, ldo=None):
        """f_s at the points [off, off + length) of `data` -> (S, length) array of the model dtype (row s = sample s).  out: a device
        pointer (int) or a contiguous device tensor to write there instead, rows ldo >= length apart; then nothing is returned."""
        length = data.n - off if length is None else length
        pm, _keep = point_mean(prior_mean, length, self.dtype) if prior_mean is not None else (None, None)
        pmr = C.byref(pm) if pm is not None else None
        ctx = self.ctx
        if out is not None:
            ldo = length if ldo is None else int(ldo)
            ptr = int(out.data_ptr()) if hasattr(out, "data_ptr") else int(out)
            ctx.check(ctx.lib.svgp_sampler_eval(ctx.h, self.h, data.h, off, length, pmr, C.c_void_p(ptr), ldo, 1))
            return None
        ldo = length if ldo is None else int(ldo)
        buf = np.zeros((self.n_samples, max(ldo, 1)), dtype=np_dtype(self.dtype))
        ctx.check(ctx.lib.svgp_sampler_eval(ctx.h, self.h, data.h, off, length, pmr, _ptr(buf), ldo, 0))
        return buf if ldo != length else buf[:, :length]

    def eval_grad(self, data: DeviceData, off=0, length=None, prior_mean=None, values=True, out=None, grad_out=None, ldo=None, ldg=None):
        """svgp_sampler_eval_grad at the points [off, off + length) of `data` -> (F (S, length) or None, G (S, d, length)) in the model
        dtype: G[s, c, j] = d f_s / d x_c at point off + j, the gradient of f_s - mean (the caller adds the Jacobian of its own prior
        mean offsets; they enter the values alone).  values=False: gradient only.  grad_out (and out, when values are wanted): device
        pointers (int) or contiguous device tensors to write there instead, rows ldg (ldo) >= length apart; then nothing is returned."""
        length = data.n - off if length is None else length
        pm, _keep = point_mean(prior_mean, length, self.dtype) if prior_mean is not None else (None, None)
        pmr = C.byref(pm) if pm is not None else None
        ctx, S, d = self.ctx, self.n_samples, self.d
        ldo = length if ldo is None else int(ldo)
        ldg = length if ldg is None else int(ldg)
        if grad_out is not None or out is not None:
            if grad_out is None or (values and out is None):
                raise ValueError("device output: grad_out is required, and out when values are wanted (both live in the same kind of memory)")
            dev = lambda t: C.c_void_p(int(t.data_ptr()) if hasattr(t, "data_ptr") else int(t))
            ctx.check(ctx.lib.svgp_sampler_eval_grad(ctx.h, self.h, data.h, off, length, pmr, dev(out) if values else None, ldo,
                                                     dev(grad_out), ldg, 1))
            return None
        dt = np_dtype(self.dtype)
        F = np.zeros((S, max(ldo, 1)), dtype=dt) if values else None
        G = np.zeros((S, d, max(ldg, 1)), dtype=dt)
        ctx.check(ctx.lib.svgp_sampler_eval_grad(ctx.h, self.h, data.h, off, length, pmr, _ptr(F) if values else None, ldo, _ptr(G), ldg, 0))
        if values and ldo == length:
            F = F[:, :length]
        return F, (G if ldg != length else G[:, :, :length])

    def state(self):
        """(u, V) in fp64, (M, S) each: the draws u_s ~ q(u) and V_s = Kuu^-1 (u_s - mean(z) - Phi(z) w_s)."""
        u = np.zeros((self.M, self.n_samples), order="F")
        V = np.zeros((self.M, self.n_samples), order="F")
        self.ctx.check(self.ctx.lib.svgp_sampler_state(self.ctx.h, self.h, _ptr(u), _ptr(V)))
        return u, V

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_sampler_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def gausshermite(n: int):
    lib = load_library()
    xs = np.zeros(n)
    ws = np.zeros(n)
    rc = lib.svgp_gausshermite(n, xs.ctypes.data_as(C.POINTER(C.c_double)), ws.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != OK:
        raise ValueError(f"svgp_gausshermite({n}) failed with status {rc}")
    return xs, ws


class _Borrowed:
    """A member context of a Group seen through the Context interface (the group owns and destroys it)."""

    check = Context.check
    timing = Context.timing
    comm_info = Context.comm_info

    def __init__(self, lib, h, device):
        self.lib, self.h, self.device = lib, C.c_void_p(h), device


class Group:
    """One process driving several GPUs (svgp_group_*): data sharded over the members, the model replicated, and
    elbo / elbo_grad evaluated on all of them with one RCCL all-reduce issued by the library."""

    def __init__(self, device_ids):
        self.lib = load_library()
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        h = C.c_void_p()
        rc = self.lib.svgp_group_create(len(device_ids), ids, C.byref(h))
        if rc != OK:
            raise SvgpError(f"svgp_group_create failed with status {rc}")
        self.h, self.n = h, len(device_ids)
        self.members = [_Borrowed(self.lib, self.lib.svgp_group_ctx(h, i), device_ids[i]) for i in range(self.n)]
        self._data, self._models = None, None

    def _check(self, rc, terms=None):
        if rc == OK:
            return
        msg = (self.lib.svgp_group_last_error(self.h) or b"").decode()
        if rc == INVALID_ARG:
            raise ValueError(msg)
        if rc == NOT_POSDEF:
            raise PosDefException(terms.chol_info if terms is not None else -1, msg)
        if rc == NEG_VARIANCE:
            raise DomainError(msg)
        raise SvgpError(f"status {rc}: {msg}")

    def upload(self, x, y, dtype, layout=COLVECS):
        dt = np_dtype(dtype_code(dtype))
        x = np.asarray(x, dtype=dt)
        if x.ndim == 1:
            layout, d, n, xb = VEC, 1, x.shape[0], np.ascontiguousarray(x)
        elif layout == COLVECS:
            (d, n), xb = x.shape, np.asfortranarray(x)
        else:
            (n, d), xb = x.shape, np.asfortranarray(x)
        yb = np.ascontiguousarray(np.asarray(y, dtype=dt))
        arr = (C.c_void_p * self.n)()
        self._check(self.lib.svgp_group_data_upload(self.h, dtype_code(dt), layout, d, n, _ptr(xb), _ptr(yb), arr))
        self._data = arr
        base, rem = divmod(n, self.n)
        self.shard_sizes = [base + (1 if i < rem else 0) for i in range(self.n)]
        return arr

    def create_model(self, desc, keep):
        arr = (C.c_void_p * self.n)()
        self._check(self.lib.svgp_group_model_create(self.h, C.byref(desc), arr))
        self._models, self._M, self._d, self._dtype = arr, desc.M, desc.d, desc.dtype
        del keep
        return arr

    def update_model(self, desc, keep):
        self._check(self.lib.svgp_group_model_update(self.h, self._models, C.byref(desc)))
        del keep

    def _ranges(self, offs, lens):
        offs = [0] * self.n if offs is None else list(offs)
        lens = [s - o for s, o in zip(self.shard_sizes, offs)] if lens is None else list(lens)
        return (C.c_int64 * self.n)(*offs), (C.c_int64 * self.n)(*lens)

    def elbo(self, offs=None, lens=None, num_data=0.0):
        o, l = self._ranges(offs, lens)
        out, terms = C.c_double(), Terms()
        self._check(self.lib.svgp_group_elbo(self.h, self._models, self._data, o, l, float(num_data), C.byref(out), C.byref(terms)), terms)
        return out.value, terms

    def elbo_grad(self, offs=None, lens=None, num_data=0.0):
        o, l = self._ranges(offs, lens)
        dt = np_dtype(self._dtype)
        il = np.zeros(self._d)
        zb = np.zeros((self._M,) if self._d == 1 else (self._d, self._M), dtype=dt, order="F")
        mb = np.zeros(self._M, dtype=dt)
        Lb = np.zeros((self._M, self._M), dtype=dt, order="F")
        g = Grads(0.0, 0.0, 0.0, il.ctypes.data_as(C.POINTER(C.c_double)), _ptr(zb), _ptr(mb), _ptr(Lb))
        out, terms = C.c_double(), Terms()
        self._check(self.lib.svgp_group_elbo_grad(self.h, self._models, self._data, o, l, float(num_data), C.byref(out),
                                                  C.byref(terms), C.byref(g)), terms)
        return out.value, terms, dict(variance=g.variance, lik_sigma2=g.lik_sigma2, mean_const=g.mean_const,
                                      inv_lengthscale=il, z=zb, m=mb, Lq=Lb)

    def close(self):
        if getattr(self, "h", None):
            for i in range(self.n):
                if self._models is not None:
                    self.lib.svgp_model_free(self.members[i].h, self._models[i])
                if self._data is not None:
                    self.lib.svgp_data_free(self.members[i].h, self._data[i])
            self._models = self._data = None
            self.lib.svgp_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
