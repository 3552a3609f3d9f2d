"""The collapsed (Titsias 2009) bound of sparse GP regression and the optimal q(u) over the C-ABI (svgp_collapsed_*): the mirror of
AbstractGPs' `VFE(fz)` as the reference's tests use it (test/SparseVariationalApproximationModule.jl:99-134) and of
`optimal_variational_posterior` (test/test_utils.jl:7-17).

    elbo(VFE(f(z, jitter)), f(x, sigma2), y)                  the collapsed bound (one data pass; no q to carry)
    elbo(VFE(fz), f(x, Diagonal(sigma2_vector)), y)           ... with a diagonal, non-isotropic noise covariance (AbstractGPs' VFE
                                                              accepts f(x, Σy::Diagonal)); any prior mean (CustomMean) as well
    elbo_and_gradient(VFE(fz), fx, y)                         the bound and its gradient in the hyperparameters and z
                                                              (wrt_noise / wrt_mean: also in the noise vector and the mean at x)
    posterior(VFE(fz), fx, y)                                 ApproxPosteriorGP at the optimal q
    optimal_variational_posterior(fz, fx, y)                  that q as a SparseVariationalApproximation

`elbo`, `elbo_and_gradient`, `approx_lml` and `posterior` dispatch on the approximation type: anything that is not a VFE goes to the
existing methods with its arguments passed on exactly.  This file only packs parameters and maps status codes to exceptions."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _ffi
from . import nearest_neighbors as _nn
from . import sva as _sva
from .gp import Diagonal, FiniteGP, GaussianLikelihood, LatentFiniteGP, MvNormal
from .sva import ApproxPosteriorGP, Centered, NonCentered, SparseVariationalApproximation

_HOMOSCEDASTIC = ("The observation noise fx.Σy must be homoscedastic.\n"
                  "To avoid this error, construct fx using: f = GP(kernel); fx = f(x, σ²), where σ² is a positive Real.")


@dataclass(eq=False)
class VFE:
    """VFE(fz::FiniteGP): the variational free energy approximation with inducing inputs fz.x and jitter fz.Σy."""

    fz: FiniteGP

    def __post_init__(self):
        if not isinstance(self.fz, FiniteGP):
            raise TypeError("VFE(fz): fz must be a FiniteGP")


def _check(fz, fx, y, small_problems, want_grad, ctx):
    """Every check that needs no GPU, in the order of the SVGP path: -> (the Gaussian LatentFiniteGP of fx, s) with s None or the
    per-point noise variances above lik.sigma2 (Σy = Diagonal(v) maps to sigma2 = min(v), s = v - min(v))."""
    s = None
    if isinstance(fx, LatentFiniteGP):
        if not isinstance(fx.lik, GaussianLikelihood):
            raise ValueError("the collapsed bound needs a Gaussian likelihood: use elbo(sva, lfx, y) for any other")
        lfx = fx
    elif isinstance(fx, FiniteGP):
        if isinstance(fx.Sigma_y, Diagonal):   # AbstractGPs' VFE takes a Diagonal Σy (the SVGP elbo, SVA:319-327, does not)
            sy = np.asarray(fx.Sigma_y.diag, dtype=np.float64)
            if sy.ndim != 1 or sy.shape[0] != fx.n:
                raise ValueError(f"fx.Σy = Diagonal(v) needs a vector with one variance per point ({fx.n}); got shape {sy.shape}")
            if not np.all(sy > 0.0):   # (NaN included) cholesky(Σy) throws in the reference
                raise ValueError("fx.Σy must be positive: every per-point noise variance must be > 0")
            s2 = float(sy.min())
            s = sy - s2
            lfx = LatentFiniteGP(fx, GaussianLikelihood(s2))
        elif not fx.is_isotropic():
            raise RuntimeError(_HOMOSCEDASTIC + "\nFor per-point noise variances v use fx = f(x, Diagonal(v)).")   # a plain vector: SVA:319-327's text
        else:
            lfx = LatentFiniteGP(fx, GaussianLikelihood(float(fx.Sigma_y)))
    else:
        raise TypeError("expected a FiniteGP or a LatentFiniteGP")
    if fz.f is not lfx.fx.f:   # SVA:347-351
        raise ValueError("(Latent)FiniteGP prior is not consistent with SparseVariationalApproximation's")
    _sva._decline_if_small(VFE(fz), lfx, y, small_problems, want_grad, ctx)
    return lfx, s


class _Resident:
    """model (any q: the collapsed calls do not read it) + data on the device for one call."""

    def __init__(self, fz, lfx, y, ctx, dtype, parametrization=NonCentered):
        z = np.asarray(fz.x)
        M = z.shape[0] if z.ndim == 1 else z.shape[1]
        centered = parametrization is Centered or isinstance(parametrization, Centered)
        sva = SparseVariationalApproximation(Centered() if centered else NonCentered(), fz, MvNormal.from_cholesky(np.zeros(M), np.eye(M)))
        desc, keep = _sva._desc(sva, lfx.lik, None, dtype)
        self.ctx = ctx or _ffi.default_context()
        self.n = np.asarray(y).shape[0]
        self.data = _ffi.DeviceData(self.ctx, lfx.fx.x, np.asarray(y), _ffi.np_dtype(desc.dtype))
        try:
            self.model = _sva._device_model(self.ctx, sva, desc, keep)   # (a CustomMean prior: its values at z, set_mean_z)
        except BaseException:
            self.data.free()
            raise
        # a CustomMean prior: its values at x travel with every call; the model then carries muz, which the _with_noise calls accept
        self.mux = lfx.fx.f.mean_offsets(lfx.fx.x)
        self.ext = dict(prior_mean=self.mux, mean_z=self.mux is not None)

    def free(self):
        self.model.free()
        self.data.free()


def elbo(approx, fx, y, **kwargs):
    """elbo(VFE(fz), fx, y; ctx, dtype, return_terms, small_problems): the collapsed bound.  Any other approximation: sva.elbo."""
    if not isinstance(approx, VFE):
        return _sva.elbo(approx, fx, y, **kwargs)
    extra = set(kwargs) - {"ctx", "dtype", "return_terms", "small_problems"}
    if extra:
        raise TypeError(f"elbo() with VFE got unexpected keyword arguments {sorted(extra)}")
    lfx, s = _check(approx.fz, fx, y, kwargs.get("small_problems", "run"), False, kwargs.get("ctx"))
    r = _Resident(approx.fz, lfx, y, kwargs.get("ctx"), kwargs.get("dtype"))
    try:
        val, terms = r.model.collapsed_bound(r.data, 0, r.n, noise=s, **r.ext)
    finally:
        r.free()
    return (val, terms) if kwargs.get("return_terms") else val


def approx_lml(approx, fx, y, **kwargs):
    """approx_lml(VFE(fz), fx, y) = elbo(VFE(fz), fx, y); any other approximation: the existing methods."""
    if isinstance(approx, VFE):
        return elbo(approx, fx, y, **kwargs)
    return _nn.approx_lml(approx, fx, y, **kwargs)


def elbo_and_gradient(approx, fx, y, **kwargs):
    """elbo_and_gradient(VFE(fz), fx, y; ctx, dtype, small_problems, wrt_inputs, wrt_noise, wrt_mean) -> (bound, dict(variance,
    inv_lengthscale, z, lik_sigma2, mean_const[, x][, Sigma_y][, mean_x])): the bound's total derivatives (d elbo / d q = 0 at the
    optimal q).  wrt_noise: "Sigma_y" (n,), d bound / d Σy_jj ("lik_sigma2" is their sum); wrt_mean: "mean_x" (n,), d bound / d
    mean(x_j), for the caller to pull back through a noise or mean function.  Otherwise: sva's."""
    if not isinstance(approx, VFE):
        return _sva.elbo_and_gradient(approx, fx, y, **kwargs)
    extra = set(kwargs) - {"ctx", "dtype", "small_problems", "wrt_inputs", "wrt_noise", "wrt_mean"}
    if extra:
        raise TypeError(f"elbo_and_gradient() with VFE got unexpected keyword arguments {sorted(extra)}")
    lfx, s = _check(approx.fz, fx, y, kwargs.get("small_problems", "run"), True, kwargs.get("ctx"))
    r = _Resident(approx.fz, lfx, y, kwargs.get("ctx"), kwargs.get("dtype"))
    try:
        val, _, grads = r.model.collapsed_grad(r.data, 0, r.n, z_shape=np.asarray(approx.fz.x).shape,
                                               inputs=True if kwargs.get("wrt_inputs") else None, noise=s,
                                               want_noise_grad=True if kwargs.get("wrt_noise") else None,
                                               want_mean_grad=True if kwargs.get("wrt_mean") else None, **r.ext)
    finally:
        r.free()
    if "noise" in grads:
        grads["Sigma_y"] = grads.pop("noise")
    return val, grads


def optimal_variational_posterior(fz, fx, y, parametrization=NonCentered, *, ctx=None, dtype=None, small_problems="run"):
    """optimal_variational_posterior(fz, fx, y) (test/test_utils.jl:7-17): the q(u) that maximises the ELBO, computed on the device,
    as SparseVariationalApproximation(parametrization, fz, q)."""
    lfx, s = _check(fz, fx, y, small_problems, False, ctx)
    r = _Resident(fz, lfx, y, ctx, dtype, parametrization)
    try:
        _, m, Lq = r.model.collapsed_q(r.data, 0, r.n, noise=s, **r.ext)
    finally:
        r.free()
    centered = parametrization is Centered or isinstance(parametrization, Centered)
    return SparseVariationalApproximation(Centered() if centered else NonCentered(), fz, MvNormal.from_cholesky(m, Lq))


def posterior(approx, *args, **kwargs):
    """posterior(VFE(fz), fx, y; ctx, dtype) -> ApproxPosteriorGP at the optimal q; any other approximation: the existing methods."""
    if not isinstance(approx, VFE):
        return _nn.posterior(approx, *args, **kwargs)
    fx, y = args
    extra = set(kwargs) - {"ctx", "dtype", "small_problems"}
    if extra:
        raise TypeError(f"posterior() with VFE got unexpected keyword arguments {sorted(extra)}")
    sva = optimal_variational_posterior(approx.fz, fx, y, ctx=kwargs.get("ctx"), dtype=kwargs.get("dtype"),
                                        small_problems=kwargs.get("small_problems", "run"))
    return ApproxPosteriorGP(sva, ctx=kwargs.get("ctx"), dtype=kwargs.get("dtype"))
