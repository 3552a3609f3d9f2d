"""approxgp — Python host mirror of ApproximateGPs.jl's sparse-variational API over the MI355X HIP library.

    from approxgp import *
    f = GP(1.3 * with_lengthscale(SqExponentialKernel(), 0.3))
    sva = SparseVariationalApproximation(f(z, 1e-5), MvNormal.from_cholesky(m, A))
    elbo(sva, f(x, 0.3), y, num_data=N); posterior(sva).mean_and_var(xs)
"""
from ._ffi import (Context, DeclinedError, DeviceData, DeviceModel, DomainError, PosDefException, SvgpError, UnsupportedError,
                   default_context, gausshermite, load_library, offload_advice, offload_work)
# the predictive distribution of the observation: DeviceModel.predictive for resident data, lik_predictive for latent marginals a caller
# holds; predict_y / log_predictive_density on the three posterior types
from ._ffi import PredSummary, lik_predictive
from .gp import (GP, BernoulliLikelihood, CustomMean, DefaultExpectationMethod, Diagonal, FiniteGP,
                 GaussHermiteExpectation,
                 GaussianLikelihood, LatentFiniteGP, LatentGP, MvNormal, PoissonLikelihood, ExponentialLikelihood,
                 GammaLikelihood, CallerLikelihood, LogisticLink, NormalCDFLink, ProbitLink)
from .kernels import (ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, ScaleTransform, SEKernel,
                      SqExponentialKernel, TransformedKernel, with_lengthscale)
from .sva import (SVGP, ApproxPosteriorGP, Centered, NonCentered, SparseVariationalApproximation, approx_lml, elbo,
                  elbo_and_gradient,
                  inducing_points, posterior, prior_kl)
# LaplaceApproximation; approx_lml and posterior dispatch on the approximation type (the SVGP methods above are unchanged)
from .laplace import (DeviceLaplace, LaplaceApproximation, LaplaceObjective, LaplacePosteriorGP, approx_lml,
                      approx_lml_and_gradient, build_laplace_objective, posterior)
# NearestNeighbors (Vecchia); approx_lml, approx_lml_and_gradient and posterior dispatch on it too (the methods above are unchanged)
from .nearest_neighbors import (DeviceNearestNeighbors, NearestNeighbors, NNPosteriorGP, approx_lml, approx_lml_and_gradient,
                                posterior)
# VFE(fz): the collapsed (Titsias) bound and the optimal q(u); elbo, elbo_and_gradient, approx_lml and posterior dispatch on it too
from .vfe import VFE, approx_lml, elbo, elbo_and_gradient, optimal_variational_posterior, posterior
# natural-gradient steps on q(u) (GPflow's NaturalGradient / GPyTorch's NGD); DeviceModel.natgrad_step / update_keep_q for resident loops
from .natgrad import natural_gradient_step
# pathwise posterior function samples: ApproxPosteriorGP.function_samples, DeviceModel.sampler; draw_basis draws their random numbers
from ._ffi import DeviceSampler, SampleBasis
from .pathwise import FunctionSamples, draw_basis, function_samples
# ConjugateGradients: the exact GP by matrix-free iterative solves; approx_lml, approx_lml_and_gradient and posterior dispatch on it too
from ._ffi import CGDesc, CGInfo
from .iterative import (CGPosteriorGP, ConjugateGradients, DeviceConjugateGradients, approx_lml, approx_lml_and_gradient, draw_probes,
                        posterior)
# pathwise function samples of the exact GP: CGPosteriorGP.function_samples, DeviceConjugateGradients.sampler
from .iterative import CGFunctionSamples, DeviceCGSampler, cg_sample_plan, pack_cg_basis

__all__ = [n for n in dir() if not n.startswith("_")]
