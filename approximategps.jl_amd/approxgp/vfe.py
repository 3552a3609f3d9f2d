"""The collapsed (Titsias 2009) bound of sparse GP regression and the optimal q(u) over the C-ABI (svgp_collapsed_*): the mirror of
AbstractGPs' `VFE(fz)` as the reference's tests use it (test/SparseVariationalApproximationModule.jl:99-134) and of
`optimal_variational_posterior` (test/test_utils.jl:7-17).

    elbo(VFE(f(z, jitter)), f(x, sigma2), y)                  the collapsed bound (one data pass; no q to carry)
    elbo_and_gradient(VFE(fz), fx, y)                         the bound and its gradient in the hyperparameters and z
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
from .gp import FiniteGP, GaussianLikelihood, LatentFiniteGP, MvNormal
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
    """Every check that needs no GPU, in the order of the SVGP path: -> the Gaussian LatentFiniteGP of fx."""
    if isinstance(fx, LatentFiniteGP):
        if not isinstance(fx.lik, GaussianLikelihood):
            raise ValueError("the collapsed bound needs a Gaussian likelihood: use elbo(sva, lfx, y) for any other")
        lfx = fx
    elif isinstance(fx, FiniteGP):
        if not fx.is_isotropic():
            raise RuntimeError(_HOMOSCEDASTIC)   # SVA:319-327
        lfx = LatentFiniteGP(fx, GaussianLikelihood(float(fx.Sigma_y)))
    else:
        raise TypeError("expected a FiniteGP or a LatentFiniteGP")
    if fz.f is not lfx.fx.f:   # SVA:347-351
        raise ValueError("(Latent)FiniteGP prior is not consistent with SparseVariationalApproximation's")
    if fz.f.mean_offsets(fz.x) is not None:
        raise _ffi.UnsupportedError("the collapsed bound takes ZeroMean / ConstMean priors only")
    _sva._decline_if_small(VFE(fz), lfx, y, small_problems, want_grad, ctx)
    return lfx


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
            self.model = _ffi.DeviceModel(self.ctx, desc, keep)
        except BaseException:
            self.data.free()
            raise

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
    lfx = _check(approx.fz, fx, y, kwargs.get("small_problems", "run"), False, kwargs.get("ctx"))
    r = _Resident(approx.fz, lfx, y, kwargs.get("ctx"), kwargs.get("dtype"))
    try:
        val, terms = r.model.collapsed_bound(r.data, 0, r.n)
    finally:
        r.free()
    return (val, terms) if kwargs.get("return_terms") else val


def approx_lml(approx, fx, y, **kwargs):
    """approx_lml(VFE(fz), fx, y) = elbo(VFE(fz), fx, y); any other approximation: the existing methods."""
    if isinstance(approx, VFE):
        return elbo(approx, fx, y, **kwargs)
    return _nn.approx_lml(approx, fx, y, **kwargs)


def elbo_and_gradient(approx, fx, y, **kwargs):
    """elbo_and_gradient(VFE(fz), fx, y; ctx, dtype, small_problems, wrt_inputs) -> (bound, dict(variance, inv_lengthscale, z,
    lik_sigma2, mean_const[, x])): the bound's total derivatives (d elbo / d q = 0 at the optimal q).  Otherwise: sva's."""
    if not isinstance(approx, VFE):
        return _sva.elbo_and_gradient(approx, fx, y, **kwargs)
    extra = set(kwargs) - {"ctx", "dtype", "small_problems", "wrt_inputs"}
    if extra:
        raise TypeError(f"elbo_and_gradient() with VFE got unexpected keyword arguments {sorted(extra)}")
    lfx = _check(approx.fz, fx, y, kwargs.get("small_problems", "run"), True, kwargs.get("ctx"))
    r = _Resident(approx.fz, lfx, y, kwargs.get("ctx"), kwargs.get("dtype"))
    try:
        val, _, grads = r.model.collapsed_grad(r.data, 0, r.n, z_shape=np.asarray(approx.fz.x).shape,
                                               inputs=True if kwargs.get("wrt_inputs") else None)
    finally:
        r.free()
    return val, grads


def optimal_variational_posterior(fz, fx, y, parametrization=NonCentered, *, ctx=None, dtype=None, small_problems="run"):
    """optimal_variational_posterior(fz, fx, y) (test/test_utils.jl:7-17): the q(u) that maximises the ELBO, computed on the device,
    as SparseVariationalApproximation(parametrization, fz, q)."""
    lfx = _check(fz, fx, y, small_problems, False, ctx)
    r = _Resident(fz, lfx, y, ctx, dtype, parametrization)
    try:
        _, m, Lq = r.model.collapsed_q(r.data, 0, r.n)
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
