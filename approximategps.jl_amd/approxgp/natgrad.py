"""Natural-gradient steps on q(u) over the C-ABI (svgp_natgrad_step): what GPflow's NaturalGradient and GPyTorch's NGD do for the
variational distribution while an ordinary optimiser trains the hyperparameters.

    sva, elbo_old = natural_gradient_step(sva, fx, y; step=1.0, num_data=length(y), quadrature)

moves q = N(m, S) of `sva` by one step of length `step` in (0, 1] along the ELBO's gradient in the expectation parameters and returns
the new SparseVariationalApproximation (same fz, same parametrisation) together with the ELBO at the q it started from.  step = 1 with
a Gaussian likelihood on the full batch lands on `optimal_variational_posterior`.  A training loop that keeps its model on the device
calls DeviceModel.natgrad_step / update_keep_q instead (examples/i_natural_gradients.py).  This file only packs parameters."""
from __future__ import annotations

import numpy as np

from . import _ffi
from .gp import CallerLikelihood, FiniteGP, GaussianLikelihood, LatentFiniteGP, MvNormal
from .sva import SparseVariationalApproximation, _desc


def natural_gradient_step(sva: SparseVariationalApproximation, fx, y, *, step=1.0, num_data=None, quadrature=None, ctx=None, dtype=None):
    """-> (SparseVariationalApproximation at the new q, ELBO at the old q).  fx: a FiniteGP (Gaussian likelihood with fx.Σy, which
    must be homoscedastic) or a LatentFiniteGP with one of the built-in likelihoods."""
    if isinstance(fx, FiniteGP):
        if not fx.is_isotropic():
            raise RuntimeError("The observation noise fx.Σy must be homoscedastic.\n"
                               "To avoid this error, construct fx using: f = GP(kernel); fx = f(x, σ²), where σ² is a positive Real.")
        lfx = LatentFiniteGP(fx, GaussianLikelihood(float(fx.Sigma_y)))
    elif isinstance(fx, LatentFiniteGP):
        lfx = fx
    else:
        raise TypeError("natural_gradient_step expects a FiniteGP or a LatentFiniteGP")
    if sva.fz.f is not lfx.fx.f:  # SVA:347-351
        raise ValueError("(Latent)FiniteGP prior is not consistent with SparseVariationalApproximation's")
    if isinstance(lfx.lik, CallerLikelihood):
        raise _ffi.UnsupportedError("natural_gradient_step takes the built-in likelihoods; a caller-evaluated one goes through "
                                    "DeviceModel.natgrad_step(ext=...)")
    if sva.fz.f.mean_offsets(sva.fz.x) is not None or lfx.fx.f.mean_offsets(lfx.fx.x) is not None:
        raise _ffi.UnsupportedError("natural_gradient_step takes ZeroMean / ConstMean priors only")
    if not (0.0 < float(step) <= 1.0):
        raise ValueError("step must lie in (0, 1]")
    desc, keep = _desc(sva, lfx.lik, quadrature, dtype)
    ctx = ctx or _ffi.default_context()
    y = np.asarray(y)
    n = y.shape[0]
    data = _ffi.DeviceData(ctx, lfx.fx.x, y, _ffi.np_dtype(desc.dtype))
    try:
        model = _ffi.DeviceModel(ctx, desc, keep)
        try:
            val, _, _, m, Lq = model.natgrad_step(data, 0, n, float(num_data) if num_data is not None else 0.0, gamma=float(step))
        finally:
            model.free()
    finally:
        data.free()
    return SparseVariationalApproximation(sva.parametrization, sva.fz, MvNormal.from_cholesky(m, Lq)), val
